"""The point stars' model on the CPU (tests/stars_ref.py: the brute-force binary64 reference with a float32 switch) and the
catalogue helpers of bhr_amd.stars.  No GPU."""
import numpy as np
import pytest

import kerr_ref as K
import observer_ref as O
import stars_ref as R


def pinhole(cam, x, y):
    """Unit direction through the fractional pixel position (x, y) of kerr_ref's camera, binary64."""
    cp, cr, cu, cf = (cam[k].astype(np.float64) for k in ("pos", "right", "up", "forward"))
    pw, ph, W, H = float(cam["pw"]), float(cam["ph"]), cam["width"], cam["height"]
    tl = (cp + cf) - (pw * W / 2) * cr + (ph * H / 2) * cu
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d = tl + ((x + 0.5) * pw)[..., None] * cr - ((y + 0.5) * ph)[..., None] * cu - cp
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def frame_stars(cam, n, seed, margin=1.0):
    """n star directions through random positions inside the frame's cells (at least `margin` pixels from the border)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(margin, cam["width"] - 1 - margin, n)
    y = rng.uniform(margin, cam["height"] - 1 - margin, n)
    return pinhole(cam, x, y), rng.uniform(0.2, 1.0, (n, 3))


def test_flat_space_conserves_flux():
    """Escape directions equal to the camera directions: every magnification is 1 and the plane sums to
    sum Phi / (2 Omega_cam(T)) over the star images, to 1e-12 relative."""
    cam = K.build_camera([6.0, 0.0, 0.5], 60.0, 40, 28)
    n = K.pixel_rays(cam)
    status = np.ones((28, 40), dtype=np.int32)
    dirs, flux = frame_stars(cam, 300, 1)
    S, st = R.star_plane(status, n, n, dirs, flux, details=True)
    tri, pairs = st["tri"], st["pairs"]
    assert np.all(tri["mag"] == 1.0) and st["capped"] == 0 and st["skipped_span"] == 0
    assert st["images"] == 300                                      # one image per star (none sits on an edge)
    want = (flux[pairs[:, 1].astype(int)] / (2.0 * tri["o_cam"][pairs[:, 0].astype(int)])[:, None]).sum(axis=0)
    got = S.sum(axis=(0, 1))
    assert np.all(np.abs(got - want) <= 1e-12 * want), (got, want)
    # the prefilter thins pairs and changes nothing: the plane of the every-pair pass is the same bits
    S_all = R.star_plane(status, n, n, dirs[:40], flux[:40], prefilter=False)
    assert np.array_equal(S_all, R.star_plane(status, n, n, dirs[:40], flux[:40]))
    # a star outside the frame leaves nothing
    assert not R.star_plane(status, n, n, -dirs[:5], flux[:5]).any()


def halved(cam, n):
    """The camera directions with the angle from the optical axis halved."""
    f = cam["forward"].astype(np.float64)
    f = f / np.linalg.norm(f)                          # the f32 uniform is a unit vector to 3e-8 only: 1 % of theta^2 near the axis
    c = np.clip(n @ f, -1.0, 1.0)
    perp = n - c[..., None] * f
    pn = np.linalg.norm(perp, axis=-1, keepdims=True)
    th = np.arccos(c)[..., None]
    return np.cos(th / 2) * f + np.sin(th / 2) * perp / np.where(pn > 0, pn, 1.0)


def test_known_map_magnifies_by_four():
    """theta -> theta / 2 about the optical axis maps a camera patch onto a quarter of its solid angle near the axis: the exact
    magnification at image angle theta is sin(theta) d(theta) / (sin(theta / 2) d(theta) / 2) = 4 cos(theta / 2).  A star at
    sky angle t has its image at camera angle 2 t; its deposit is that of a flat-space star at the image's place times the
    magnification of the image's triangle.
    Tolerance.  fov 10 degrees at 64 x 64: a pixel is p = 2.7e-3 rad; the images lie within 4 pixels of the axis along x and
    y, theta <= 6 p.  4 cos(theta / 2) is within theta^2 / 8 = 3.4e-5 of 4.  The flat star's triangle may be the image's
    neighbour, whose Omega_cam (~ cos^3 theta) differs by 3 theta p = 1.4e-4 at most.  A triangle replaces the map by its linear
    interpolant over a pixel, off by the map's cubic term over a pixel: below p^2 = 8e-6 relative.  Sum 1.8e-4; the bar is 2e-4."""
    cam = K.build_camera([6.0, 0.0, 0.5], 10.0, 64, 64)
    n = K.pixel_rays(cam)
    status = np.ones((64, 64), dtype=np.int32)
    rng = np.random.default_rng(2)
    x = 31.5 + rng.uniform(-4, 4, 40)
    y = 31.5 + rng.uniform(-4, 4, 40)
    image_dirs = pinhole(cam, x, y)                    # where the images are: camera directions
    sky_dirs = halved(cam, image_dirs)                 # the stars they are images of
    flux = np.ones((40, 3))
    for k in range(40):
        S4, st = R.star_plane(status, halved(cam, n), n, sky_dirs[k:k + 1], flux[k:k + 1], details=True)
        S1 = R.star_plane(status, n, n, image_dirs[k:k + 1], flux[k:k + 1])
        assert st["images"] == 1
        ratio = S4.sum() / S1.sum()
        assert abs(ratio / 4.0 - 1.0) < 2e-4, (k, ratio)


def test_fold_parity_and_cap():
    """A map folded about a line through the frame: sky column g(i) = c + (i - c0)^2 / s.  Left of c0 the triangles are
    parity-flipped and still make images; the cell that straddles c0 is squeezed beyond the cap."""
    cam = K.build_camera([6.0, 0.0, 0.5], 40.0, 48, 32)
    n = K.pixel_rays(cam)
    status = np.ones((32, 48), dtype=np.int32)
    c, c0, s = 24.0, 20.3, 64.0
    i = np.arange(48, dtype=np.float64)
    jj, ii = np.meshgrid(np.arange(32, dtype=np.float64), c + (i - c0) ** 2 / s, indexing="ij")
    esc = pinhole(cam, ii, jj)
    # a star well off the fold: sky column c + 0.5 has the images i = c0 -+ sqrt(0.5 s), one flipped, one not
    u = pinhole(cam, np.array([c + 0.5]), np.array([15.4]))
    S, st = R.star_plane(status, esc, n, u, np.ones((1, 3)), max_span_deg=60.0, details=True)
    assert st["images"] == 2
    cols = np.sort(st["tri"]["cell"][st["pairs"][:, 0].astype(int), 0] + st["pairs"][:, 2])
    d = np.sqrt(0.5 * s)
    assert abs(cols[0] - (c0 - d)) < 0.05 and abs(cols[1] - (c0 + d)) < 0.05, cols
    assert np.all(np.abs(st["pairs"][:, 4] / (s / (2 * d)) - 1.0) < 0.1)          # magnification 1 / |g'| of each, linearised
    # flipped triangles: the orientation of (e_a, e_b, e_c) left of the fold is the opposite of the camera's
    tri = st["tri"]
    sign_e = np.sign(np.einsum("tk,tk->t", tri["e"][:, 0], np.cross(tri["e"][:, 1], tri["e"][:, 2])))
    sign_n = np.sign(np.einsum("tk,tk->t", tri["n"][:, 0], np.cross(tri["n"][:, 1], tri["n"][:, 2])))
    left = tri["cell"][:, 0] < 19
    assert np.all(sign_e[left] == -sign_n[left]) and np.all(sign_e[tri["cell"][:, 0] > 21] == sign_n[tri["cell"][:, 0] > 21])
    # a star on the fold: sky column c + 0.004 lies inside the straddling cell (columns 20 -> c + 0.0014, 21 -> c + 0.0077),
    # whose magnification 1 / 0.0063 is capped
    u = pinhole(cam, np.array([c + 0.004]), np.array([15.4]))
    S, st = R.star_plane(status, esc, n, u, np.ones((1, 3)), max_magnification=32.0, max_span_deg=60.0, details=True)
    assert st["images"] >= 1 and st["capped"] >= 1
    on_fold = st["tri"]["cell"][st["pairs"][:, 0].astype(int), 0] == 20
    assert on_fold.any() and np.all(st["pairs"][on_fold, 4] == 32.0)
    t_idx = st["pairs"][on_fold, 0].astype(int)
    want = (32.0 / (2.0 * st["tri"]["o_cam"][t_idx])).sum()
    rest = st["pairs"][~on_fold]
    want += (rest[:, 4] / (2.0 * st["tri"]["o_cam"][rest[:, 0].astype(int)])).sum()
    assert abs(S[..., 0].sum() / want - 1.0) < 1e-12


def test_span_rule_and_status():
    """A triangle with a captured corner, or whose escape directions are further apart than max_span, contributes nothing."""
    cam = K.build_camera([6.0, 0.0, 0.5], 60.0, 12, 9)
    n = K.pixel_rays(cam)
    dirs, flux = frame_stars(cam, 60, 3)
    status = np.ones((9, 12), dtype=np.int32)
    status[4, 5] = 0
    S, st = R.star_plane(status, n, n, dirs, flux, details=True)
    assert len(st["tri"]["used"]) == 2 * 11 * 8 - 6                  # six triangles have pixel (5, 4) as a corner
    # pixel pitch here is ~5.5 degrees: under a 3 degree span every triangle is dropped
    S, st = R.star_plane(np.ones((9, 12), dtype=np.int32), n, n, dirs, flux, max_span_deg=3.0, details=True)
    assert not S.any() and st["images"] == 0 and st["skipped_span"] == 2 * 11 * 8


# ---------------------------------------------------------------------------------------------------- the catalogue
def test_catalogue_directions_sample_their_own_texel():
    from bhr_amd import skybox, stars
    t = skybox.sky_tables(512, 256, seed=42, n_stars=500)
    dirs, flux = stars.catalog_from_tables(t, gain=2.0, pixel_solid_angle=1e-4)
    assert dirs.dtype == np.float64 and np.allclose(np.linalg.norm(dirs, axis=1), 1.0, atol=1e-15)
    # sample_skybox's convention: theta = acos(z), phi = atan2(y, x) (+ 2 pi), u = phi / 2 pi W, v = theta / pi H, texel (floor v, floor u)
    theta = np.arccos(np.clip(dirs[:, 2], -1, 1))
    phi = np.arctan2(dirs[:, 1], dirs[:, 0])
    phi = np.where(phi < 0, phi + 2 * np.pi, phi)
    u, v = phi / (2 * np.pi) * 512, theta / np.pi * 256
    assert np.allclose(u, t["cx"].astype(np.float64), atol=1e-9) and np.allclose(v, t["cy"].astype(np.float64), atol=1e-9)
    assert np.array_equal(np.floor(u + 1e-9), np.floor(t["cx"].astype(np.float64)))
    assert np.array_equal(np.floor(v + 1e-9), np.floor(t["cy"].astype(np.float64)))
    # the blob rasterised there has its centre value on that texel: Phi = gain colour brightness solid angle
    centre = int(np.flatnonzero((t["dx"] == 0) & (t["dy"] == 0))[0])
    assert np.allclose(flux, 2.0 * t["colors"].astype(np.float64) * t["vals"][:, centre].astype(np.float64)[:, None] * 1e-4, rtol=1e-15)
    # the starless tables: the same but the blob values
    s = stars.starless_tables(t)
    assert not s["vals"].any() and t["vals"].any() and s["vals"].shape == t["vals"].shape
    assert all(s[k] is t[k] for k in t if k != "vals")
    with pytest.raises(ValueError):
        stars.catalog_from_tables(t, gain=0.0, pixel_solid_angle=1e-4)


def test_binning_loses_and_duplicates_no_star():
    from bhr_amd import skybox, stars
    t = skybox.sky_tables(512, 256, seed=7, n_stars=2000)
    dirs, _ = stars.catalog_from_tables(t, 2.0, 1e-4)
    eps = 1e-7
    special = np.array([[0, 0, 1.0], [0, 0, -1.0], [1.0, 0, 0], [np.cos(2 * np.pi - eps), np.sin(2 * np.pi - eps), 0.0],
                        [np.sin(1e-4), 0, np.cos(1e-4)], [0, 0, 1.0]])            # poles, phi = 0, phi = 2 pi - eps, a duplicate
    dirs = np.concatenate([dirs, special])
    for shape in ((0, 0), (4, 8), (13, 7), (1, 1)):
        off, order = stars.bin_catalog(dirs, *shape)
        nt, np_ = shape if shape[0] else stars.grid_shape(len(dirs))
        assert off[0] == 0 and off[-1] == len(dirs) and len(off) == nt * np_ + 1 and np.all(np.diff(off) >= 0)
        assert np.array_equal(np.sort(order), np.arange(len(dirs)))               # every star once
        d32 = dirs.astype(np.float32).astype(np.float64)
        theta = np.arccos(np.clip(d32[:, 2], -1, 1))
        phi = np.arctan2(d32[:, 1], d32[:, 0]) % (2 * np.pi)
        for b in range(nt * np_):
            members = order[off[b]:off[b + 1]]
            assert np.all(np.diff(members) > 0)                                   # catalogue order inside a bin
            tb, pb = divmod(b, np_)
            lo_t, hi_t = tb * np.pi / nt, (tb + 1) * np.pi / nt
            assert np.all((theta[members] >= lo_t - 1e-12) & ((theta[members] < hi_t + 1e-12) | (tb == nt - 1)))
            lo_p, hi_p = pb * 2 * np.pi / np_, (pb + 1) * 2 * np.pi / np_
            assert np.all((phi[members] >= lo_p - 1e-12) & ((phi[members] < hi_p + 1e-12) | (pb == np_ - 1)))
    off, order = stars.bin_catalog(dirs, 4, 8)
    n0 = len(dirs) - 6
    b_of = np.empty(len(dirs), dtype=int)
    for b in range(32):
        b_of[order[off[b]:off[b + 1]]] = b
    assert b_of[n0] // 8 == 0 and b_of[n0 + 1] // 8 == 3 and b_of[n0 + 2] == 2 * 8 + 0 and b_of[n0 + 3] == 2 * 8 + 7
    assert stars.grid_shape(6000) == (19, 38) and stars.grid_shape(1) == (4, 8) and stars.grid_shape(1 << 22) == (256, 512)


def test_check_catalog_refusals():
    from bhr_amd import stars
    ok_d, ok_f = np.array([[0, 0, 1.0]]), np.array([[1.0, 1.0, 1.0]])
    d, f = stars.check_catalog(ok_d, ok_f)
    assert d.dtype == np.float32 and f.dtype == np.float32 and d.shape == (1, 3)
    for bad_d, bad_f in (([[0, 0, 1.01]], ok_f), ([[np.nan, 0, 1]], ok_f), (ok_d, [[-1e-9, 0, 0]]), (ok_d, [[np.inf, 0, 0]]),
                         (np.zeros((2, 3)) + [0, 0, 1.0], ok_f)):
        with pytest.raises(ValueError):
            stars.check_catalog(bad_d, bad_f)


# ---------------------------------------------------------------------------------------------------- float32 against binary64
VIEWS = [(6.0, 0.0, 0.5), (3.0, 2.0, 0.3), (1.0, 0.0, 6.0)]


def marched_view(pos, width=96, height=64, fov=90.0):
    """(cam, status, normalized f32 escape directions) of the strict f32 march of the view."""
    cam = K.build_camera(pos, fov, width, height)
    d = K.pixel_rays(cam, np.float32).reshape(-1, 3)
    m = O.march(cam["pos"].astype(np.float32), d, 0.1, cam["r_escape"], dtype=np.float32)
    e = m["esc_dir"].astype(np.float32)
    inv = np.float32(1) / np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    e = np.where((m["fate"] == 1)[:, None], inv[:, None] * e, np.float32(0)).astype(np.float32)
    return cam, m["fate"].astype(np.int32).reshape(height, width), e.reshape(height, width, 3)


@pytest.mark.parametrize("pos", VIEWS)
def test_float32_reference_stays_under_the_device_cap(pos):
    """The float32 evaluation of the model against the binary64 one on the same f32 escape directions, 96 x 64, fov 90, the
    6000 procedural stars, flux scaled so that the plane's maximum is about 1: the share of pixels that differ by more than
    1e-3 of the maximum must stay under the device tests' cap of 0.5 %."""
    from bhr_amd import skybox, stars
    cam, status, esc = marched_view(pos)
    dirs, flux = stars.catalog_from_tables(skybox.sky_tables(2048, 1024, 42, 6000), 2.0, float(cam["pw"]) * float(cam["ph"]))
    d32 = dirs.astype(np.float32)
    S64, st = R.star_plane(status, esc, K.pixel_rays(cam, np.float32), d32, flux.astype(np.float32), details=True)
    scale = 1.0 / S64.max()
    S64 = S64 * scale
    S32 = R.star_plane(status, esc, K.pixel_rays(cam, np.float32), d32, (flux * scale).astype(np.float32), dtype=np.float32)
    share, dist = R.outlier_share(S32, S64), R.distance(S32, S64)
    print(f"view {pos}: used {int(st['tri']['used'].sum())} triangles, capped {st['capped']}, skipped {st['skipped_span']}, images {st['images']}; "
          f"f32 vs f64: share beyond 1e-3 of the maximum {share:.5f}, distance {dist:.3e}, largest difference {np.abs(S32 - S64).max():.3e}")
    assert S32.dtype == np.float32 and S64.max() == pytest.approx(1.0)
    assert share < 0.005
