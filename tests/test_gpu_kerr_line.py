"""The Kerr line profile on the device (bhr_set_kerr_line; include/bhr.h "Kerr line profile"): the per-record planes g
and w of a frame from the Kerr ray map against the binary64 reference (tests/kerr_line_ref.py) fed the DEVICE's own records, the
histogram against an integer sum of the device's own planes (an equality), orders and emissivities, that nothing existing moves,
the overflow list, a video's rows, the refusals and the kernel's resources.

The bars.  g within 4 x kerr_line_ref.F32_DISTANCE_G = 4 x 4.32e-7 relative, w within 4 x F32_DISTANCE_W = 4 x 6.54e-6 of the
frame's largest w: the largest |float32 reference - float64 reference| over the records of these views, spins and modes, measured
and asserted on the host (tests/test_kerr_line_ref.py); four times it covers another operation order, FMA contraction and the
device's libm, as the Kerr Stokes test argues.  The histogram has no bar: integer adds commute.

Scenes: scenes.analytic_skybox() and scenes.noisy_disk(), fov 90, the renderer's defaults (r_disk 2 .. 15, step 0.1).  The 1 x 1
frame's one ray is the radial one: it crosses no disk, the planes hold zeros and the histogram is empty.

Measured on an MI355X: largest device difference of g 5.07e-7 ((2.5, 2, 1.2) at 64 x 36; bar 1.73e-6), of w 9.63e-6 of the frame's
largest ((4, 3, 2) at 64 x 36; bar 2.62e-5); at 33 x 9 3.67e-7 / 4.33e-6, at 9 x 7 3.93e-7 / 6.51e-6, at 5 x 3 2.87e-7 / 7.32e-6."""
import ctypes as C
import functools

import numpy as np
import pytest

import kerr_line_ref as L

pytestmark = pytest.mark.gpu

FOV = 90.0
TOL_G = 4 * L.F32_DISTANCE_G
TOL_W = 4 * L.F32_DISTANCE_W
VIEWS = L.VIEWS
SPINS = ((0.0, True), (0.6, False), (-0.9, False), (0.998, False))         # (A, forced)
SIZES = ((64, 36), (33, 9), (9, 7), (5, 3), (1, 1))
CONFIGS = (("powerlaw", "first", 0.0), ("texture", "all", 7.3), ("powerlaw", "all", 7.3), ("texture", "first", 0.0))
TWO_CROSSINGS = (0.998, VIEWS[1], "exact")     # tests/test_kerr_line_ref.py: at least 5 % two-crossing pixels in the host march
BINNINGS = tuple(dict(n_bins=n) for n in (1, 7, 64, 256, 1000, 4096)) + (
    dict(n_bins=4, g_range=(0.0, 8.0)),         # every sample in one bin: the most contention
    dict(n_bins=16, g_range=(-1.0, 0.0)),       # every sample in `over`
    dict(n_bins=32, g_range=(0.8, 1.0)))        # cuts the profile in the middle: `under`, bins and `over`


@functools.lru_cache(maxsize=None)
def _scene():
    from bhr_amd import scenes
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    sky.setflags(write=False)
    tex.setflags(write=False)
    return sky, tex


def _spin(r, A, mode, force=False):
    r.set_redshift("model")
    r.set_spin(A, force_kerr=force)
    r.set_redshift(mode)


def _mk(W=64, H=36, A=0.6, mode="model", force=False, **kw):
    from bhr_amd import HipRenderer
    sky, tex = _scene()
    r = HipRenderer(W, H, sky, tex, math="strict", **kw)
    _spin(r, A, mode, force)
    return r


def _cam(r, pos):
    c = r.camera_uniforms(list(pos), FOV, 0)
    return dict(pos=np.array(list(c.pos), dtype=np.float32), right=np.array(list(c.right), dtype=np.float32), up=np.array(list(c.up), dtype=np.float32),
                forward=np.array(list(c.forward), dtype=np.float32), pw=np.float32(c.pixel_width), ph=np.float32(c.pixel_height), width=r.width, height=r.height)


def _frame(r, t=0.0, row=0, **kw):
    """A frame from the map under the line `kw` with the sample planes kept -> (planes, bins, under, over, info)."""
    r.set_kerr_line(samples=True, **kw)
    r.set_kerr_line_row(row)
    r.render_from_kerr_ray_map_async(t_offset=t, skip_bloom=True)
    bins, under, over = r.kerr_line_counts(row, 1)
    return r.kerr_line_samples(), bins[0], int(under[0]), int(over[0]), r.kerr_line_info(row)


def _own_histogram(planes, s):
    """bins, under and over in NumPy from the device's own planes: f32 products, integer sums."""
    counted = planes["w"] != 0
    counted |= planes["g"] != 0
    return L.histogram(planes["g"], planes["w"], counted, s), counted


def _check_histogram(planes, bins, under, over, info, s):
    (b, u, o), counted = _own_histogram(planes, s)
    assert bins.dtype == np.uint64 and np.array_equal(bins, b), (s, np.flatnonzero(bins != b)[:8])
    assert under == int(u) and over == int(o), (s, under, int(u), over, int(o))
    assert info["samples"] == int(counted.sum())


def _near_edge(hits, A, r_disk):
    """Records whose radius is within f32 rounding of an edge of the annulus: the device's f32 test and the reference's binary64
    one may fall on different sides there."""
    a = A * 0.5
    h = hits.astype(np.float64)
    r = np.sqrt(np.maximum(h[..., 0] ** 2 + h[..., 1] ** 2 - a * a, 0.0))
    return (np.abs(r - r_disk[0]) < 4e-6 * r_disk[0]) | (np.abs(r - r_disk[1]) < 4e-6 * r_disk[1])


@pytest.mark.parametrize("view", VIEWS, ids=lambda v: "-".join(f"{c:g}" for c in v))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_samples_against_the_reference(size, view):
    W, H = size
    r = _mk(W, H)
    _, tex = _scene()
    worst_g = worst_w = 0.0
    try:
        for A, force in SPINS:
            for mode in ("model", "exact"):
                _spin(r, A, mode, force)
                r.build_kerr_ray_map(list(view), FOV)
                p = r.kerr_ray_map_passes()
                r_disk = (r.r_disk_inner, r.r_disk_outer)
                edge = _near_edge(p["hits"], A, r_disk)
                for em, orders, t in CONFIGS:
                    s = L.settings(emissivity=em, orders=orders)
                    planes, bins, under, over, info = _frame(r, t, emissivity=em, orders=orders)
                    assert np.isfinite(planes["g"]).all() and np.isfinite(planes["w"]).all()
                    _check_histogram(planes, bins, under, over, info, s)
                    if (W, H) == (1, 1):
                        assert not p["crossings"].any() and not planes["g"].any() and not planes["w"].any()
                        assert not bins.any() and under == 0 and over == 0 and info["samples"] == 0
                        continue
                    ref = L.frame(_cam(r, view), p["hits"], p["crossings"], A, mode, s, tex, t, r_disk)
                    cnt = ref["counted"]
                    # where the planes must be 0 they are 0 exactly; where a record counts, g is there
                    assert not planes["g"][~cnt & ~edge].any() and not planes["w"][~cnt & ~edge].any()
                    m = cnt & ~edge
                    assert (planes["g"][m] > 0).all() and m.sum() >= 0.99 * cnt.sum() and m.any()
                    dg = float((np.abs(planes["g"].astype(np.float64) - ref["g"])[m] / ref["g"][m]).max())
                    dw = float(np.abs(planes["w"].astype(np.float64) - ref["w"])[m].max() / ref["w"].max())
                    worst_g, worst_w = max(worst_g, dg), max(worst_w, dw)
                    print(f"{W}x{H} {view} A={A} {mode} {em}/{orders}: g {dg:.3e} w {dw:.3e}")
                    assert dg <= TOL_G, (A, mode, em, orders, dg)
                    assert dw <= TOL_W, (A, mode, em, orders, dw)
    finally:
        r.close()
    print(f"{W}x{H} {view}: largest g {worst_g:.3e} (bar {TOL_G:.3e}), w {worst_w:.3e} (bar {TOL_W:.3e})")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_histogram_is_exact(size):
    W, H = size
    r = _mk(W, H)
    try:
        for (A, force), mode, view in (((0.998, False), "exact", VIEWS[1]), ((-0.9, False), "model", VIEWS[0])):
            _spin(r, A, mode, force)
            r.build_kerr_ray_map(list(view), FOV)
            for kw in BINNINGS:
                s = L.settings(emissivity="texture", orders="all", **kw)
                planes, bins, under, over, info = _frame(r, 7.3, 0, emissivity="texture", orders="all", **kw)
                _check_histogram(planes, bins, under, over, info, s)
                total = int(bins.sum(dtype=np.uint64)) + under + over
                if (W, H) != (1, 1):
                    assert total > 0
                    if kw.get("g_range") == (0.0, 8.0):
                        assert int(bins[0]) == total
                    if kw.get("g_range") == (-1.0, 0.0):
                        assert over == total
                    if kw.get("g_range") == (0.8, 1.0) and (W, H) == (64, 36):
                        assert under > 0 and over > 0 and bins.any()
                # the same frame again on the other frame slot into another row, and once more into the first: identical rows
                r.set_kerr_line_row(1)
                r.render_from_kerr_ray_map_async(t_offset=7.3, skip_bloom=True)
                r.set_kerr_line_row(0)
                r.render_from_kerr_ray_map_async(t_offset=7.3, skip_bloom=True)
                b2, u2, o2 = r.kerr_line_counts(0, 2)
                for k in (0, 1):
                    assert np.array_equal(b2[k], bins) and int(u2[k]) == under and int(o2[k]) == over, (kw, k)
                assert r.kerr_line_info(1) == info
    finally:
        r.close()


def test_orders_and_emissivities():
    A, view, mode = TWO_CROSSINGS
    r = _mk(64, 36, A, mode)
    try:
        r.build_kerr_ray_map(list(view), FOV)
        cnt = r.kerr_ray_map_passes()["crossings"]
        assert (cnt >= 2).sum() >= 0.05 * (cnt >= 1).sum()          # a condition on the input
        rows = {}
        for em in ("powerlaw", "texture"):
            for orders in ("first", "all"):
                for t in (0.0, 7.3):
                    planes, bins, under, over, _ = _frame(r, t, emissivity=em, orders=orders)
                    rows[em, orders, t] = (planes["g"].copy(), planes["w"].copy(), bins.copy(), under, over)
        for em in ("powerlaw", "texture"):
            first, both = rows[em, "first", 0.0], rows[em, "all", 0.0]
            assert not np.array_equal(first[2], both[2])
            assert ((first[0] != 0).sum(0) <= 1).all() and ((both[0] != 0).sum(0) >= 2).any()
        assert (rows["powerlaw", "first", 0.0][2] <= rows["powerlaw", "all", 0.0][2]).all()
        for orders in ("first", "all"):
            a, b = rows["powerlaw", orders, 0.0], rows["powerlaw", orders, 7.3]
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]
            a, b = rows["texture", orders, 0.0], rows["texture", orders, 7.3]
            assert np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2])
    finally:
        r.close()


@pytest.mark.parametrize("mode", ("model", "exact"))
def test_nothing_existing_moves(mode):
    from bhr_amd import _lib
    r = _mk(64, 36, 0.6, mode)
    view = VIEWS[2]

    def frame(t):
        r.render_from_kerr_ray_map_async(t_offset=t)
        return [r.read_layer(k).copy() for k in (_lib.LAYER_FINAL, _lib.LAYER_BG, _lib.LAYER_DISK)] + [r.read_final_u8().copy()]

    try:
        r.set_kerr_polarization("toroidal", 0.7, 16)
        r.build_kerr_ray_map(list(view), FOV)
        before = r.kerr_ray_map_passes()
        plain = [frame(t) for t in (0.0, 7.3)]
        stokes = r.stokes().copy()
        r.set_kerr_line(emissivity="texture", orders="all", samples=True)
        r.build_kerr_ray_map(list(view), FOV)          # a build with a line set: the same map
        lined = [frame(t) for t in (0.0, 7.3)]
        assert r.kerr_line_info(0)["samples"] > 0
        for a, b in zip(plain, lined):
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and np.array_equal(x, y)
        assert np.array_equal(stokes, r.stokes())
        after = r.kerr_ray_map_passes()
        assert sorted(before) == sorted(after)
        for k in before:
            assert np.array_equal(before[k], after[k]), k
    finally:
        r.close()


def test_overflow_pixels_contribute_nothing():
    A, view, mode = TWO_CROSSINGS
    r = _mk(64, 36, A, mode, options={"raymap_slots": 1})
    try:
        r.build_kerr_ray_map(list(view), FOV)
        p = r.kerr_ray_map_passes()
        listed = p["crossings"] > 1
        assert listed.sum() >= 0.05 * (p["crossings"] >= 1).sum() and r.kerr_ray_map_info()["overflow_pixels"] == listed.sum()
        for em, orders, t in CONFIGS:
            planes, bins, under, over, info = _frame(r, t, emissivity=em, orders=orders)
            assert planes["g"].shape[0] == 1
            assert info["overflow_pixels"] == int(listed.sum())
            assert not planes["g"][0][listed].any() and not planes["w"][0][listed].any()
            assert (planes["g"][0][(p["crossings"] == 1)] > 0).all()
            _check_histogram(planes, bins, under, over, info, L.settings(emissivity=em, orders=orders))
    finally:
        r.close()


@pytest.mark.parametrize("emissivity", ("powerlaw", "texture"))
def test_video_rows_are_the_stills(emissivity, tmp_path):
    """render_video(spin_map=True, kerr_line=): row f of the .npz is the row of a still from the same map under the disk texture as
    the video's lifecycle had composed it at frame f (the driver's frames roll the texture itself and pass t_offset 0)."""
    from bhr_amd import drivers
    W, H, N = 64, 36, 5
    pov = [6.0, 0.0, 0.5]
    path = str(tmp_path / "line.npz")
    kw = dict(n_bins=64, emissivity=emissivity, orders="all")
    r, _, _, _ = drivers.make_renderer(W, H, pov, FOV, n_stars=200, tex_w=256, tex_h=128, spin=0.6)
    try:
        textures, frame_call = [], r.render_from_kerr_ray_map_async

        def spy(*a, **k):
            textures.append(r._read_disk_texture().copy())
            return frame_call(*a, **k)
        r.render_from_kerr_ray_map_async = spy
        drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=str(tmp_path / "v" / "v.mp4"), fov=FOV, static_cam_pos=pov, assemble=False,
                             video_stream="off", spin_map=True, kerr_line=dict(path=path, **kw))
        del r.render_from_kerr_ray_map_async
        z = np.load(path)
        assert len(textures) == N and z["counts"].shape == (N, 64) and z["flux"].shape == (N, 64) and z["under"].shape == (N,)
        assert z["counts"].dtype == np.uint64 and z["counts"].any(axis=1).all()
        with pytest.raises(AssertionError):
            r.kerr_line_counts(0, 1)                                        # the driver switched the line off again
        r.set_kerr_line(**kw)
        r.build_kerr_ray_map(pov, FOV)
        for f in range(N):
            r.update_disk_texture(textures[f])
            r.render_from_kerr_ray_map_async(frame=0, skip_bloom=True)
            bins, under, over = r.kerr_line_counts(0, 1)
            assert np.array_equal(bins[0], z["counts"][f]) and under[0] == z["under"][f] and over[0] == z["over"][f], f
        if emissivity == "powerlaw":
            assert (z["counts"] == z["counts"][0]).all()                    # independent of time
        elif any(not np.array_equal(textures[0][..., 3], t[..., 3]) for t in textures[1:]):
            assert not (z["counts"] == z["counts"][0]).all()                # the spectrum moves with the texture's opacity
    finally:
        r.close()


def test_refusals_leave_the_context_as_it_was():
    from bhr_amd import _lib
    r = _mk(64, 36, 0.6, "model")
    view = VIEWS[0]
    try:
        # without the Kerr march: BHR_ERR_STATE
        plain = _mk(16, 9, 0.0, "model")
        try:
            with pytest.raises(AssertionError, match="bhr_set_kerr_line"):
                plain.set_kerr_line()
        finally:
            plain.close()
        # a bad value names its field: BHR_ERR_INVALID
        par = dict(n_bins=256, g_min=0.0, g_max=2.0, power=4.0, index=3.0, emissivity=0, orders=0, r_inner=0.0, r_outer=0.0)
        for field, bad, word in (("n_bins", 0, "n_bins"), ("n_bins", 4097, "n_bins"), ("g_max", 0.0, "g_min"), ("g_max", float("nan"), "g_min"),
                                 ("power", -1.0, "power"), ("power", 9.0, "power"), ("index", -0.5, "index"), ("emissivity", 2, "emissivity"),
                                 ("orders", -1, "orders"), ("r_inner", 1.0, "r_inner"), ("r_outer", 16.0, "r_outer")):
            q = dict(par)
            q[field] = bad
            if field == "r_inner":
                q["r_outer"] = 10.0
            if field == "r_outer":
                q["r_inner"] = 3.0
            st = _lib.KerrLine(q["n_bins"], q["g_min"], q["g_max"], q["power"], q["index"], q["emissivity"], q["orders"], q["r_inner"], q["r_outer"])
            assert r._lib.bhr_set_kerr_line(r._ctx, C.byref(st)) == _lib.BHR_ERR_INVALID, (field, bad)
            assert word.encode() in r._lib.bhr_last_error(), (field, r._lib.bhr_last_error())
        r.build_kerr_ray_map(list(view), FOV)
        planes, bins, under, over, info = _frame(r, 0.0)
        # a row that is not reserved, a turned view, a shutter frame: BHR_ERR_STATE, and the row keeps what it held
        r.set_kerr_line_row(2)
        with pytest.raises(AssertionError, match="kerr_line_row"):
            r.render_from_kerr_ray_map_async(t_offset=1.0, skip_bloom=True)
        r.set_kerr_line_row(0)
        turned = [view[0] * np.cos(0.3) - view[1] * np.sin(0.3), view[0] * np.sin(0.3) + view[1] * np.cos(0.3), view[2]]     # the build camera turned about z
        with pytest.raises(AssertionError, match="bhr_set_kerr_line"):
            r.render_from_kerr_ray_map_async(t_offset=1.0, cam_pos=turned, skip_bloom=True)
        with pytest.raises(AssertionError, match="bhr_set_kerr_line"):
            r.render_shutter_from_kerr_ray_map_async([0.0, 0.1], skip_bloom=True)
        b2, u2, o2 = r.kerr_line_counts(0, 1)
        assert np.array_equal(b2[0], bins) and int(u2[0]) == under and int(o2[0]) == over
        # a supersampled build: BHR_ERR_INVALID, the map stays
        with pytest.raises(ValueError, match="bhr_set_kerr_line"):
            r.build_kerr_ray_map(list(view), FOV, supersample=2)
        r.set_option("kerr_raymap_supersample", 1)
        assert r.kerr_ray_map_info()["built"] == 1 and r.kerr_ray_map_info()["supersample"] == 1
        # a build under the Kerr anti-aliasing is refused as ever
        r.set_kerr_anti_alias(True, 1.0)
        with pytest.raises(ValueError, match="anti-aliasing"):
            r.build_kerr_ray_map(list(view), FOV)
        r.set_kerr_anti_alias(False)
    finally:
        r.close()
    # a map built supersampled, then a line: the render is refused with BHR_ERR_STATE
    r = _mk(16, 9, 0.6, "model")
    try:
        # ... and under a Kerr Disk V2 source (which a built map refuses in its turn: a context without one)
        from bhr_amd import drivers
        r.set_kerr_line()
        assert drivers.use_kerr_analytic_disk(r, "v2")
        with pytest.raises(ValueError, match="Disk V2"):
            r.build_kerr_ray_map(list(view), FOV)
        assert r.kerr_ray_map_info()["built"] == 0
        r.use_kerr_disk_v2(None)
        r.clear_kerr_line()
        r.build_kerr_ray_map(list(view), FOV, supersample=2)
        r.set_kerr_line()
        with pytest.raises(AssertionError, match="kerr_raymap_supersample"):
            r.render_from_kerr_ray_map_async(t_offset=0.0, skip_bloom=True)
        r.clear_kerr_line()
        r.render_from_kerr_ray_map_async(t_offset=0.0, skip_bloom=True)
        r.sync()
        with pytest.raises(AssertionError):
            r.kerr_line_counts(0, 1)
    finally:
        r.close()


def test_resources():
    r = _mk(8, 8)
    try:
        for mode in ("model", "exact"):
            for em in ("powerlaw", "texture"):
                res = r.kerr_line_resources(mode, em)
                print(mode, em, res)
                assert res["scratch_bytes"] == 0 and 0 < res["vgprs"] <= 128
    finally:
        r.close()
