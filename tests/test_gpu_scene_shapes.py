"""The march's texture and sky samplers (csrc/march_device.h: sample_disk_level, sample_skybox, the level pick in shade_hit) at
the shapes the rest of the suite never marches through: disk textures with fewer than the five stored mip levels, odd
sides, a single row, three texels across; skies that are neither a power of two nor 1:2, down to one texel.

Two kinds of shape.  Inside the reference's domain (every level it halves has even sides) the definition is the
reference's: generate_disk_mipmaps stops when a side drops below 2, and _sample_disk_mip clamps the level to the chain's
last (render.py:1113-1125, 2613) -- a 4 x 12 texture has the levels 4x12, 2x6, 1x3 and a crossing with lod 3 samples
level 2.  The fixtures few_levels / four_levels pin that against the reference's own statements
(test_gpu_reference_kernels.py, test_gpu_hybrid.py); here the oracle, which test_reference_kernels.py pins to the same
fixtures, stands in for it.  Outside that domain (the reference raises on an odd side) the library, textures.py and the
oracle floor-halve and go on: the oracle is the definition.

Bars are those of the tests named at each check; none is new.  Textures are seeded uniform noise (texel-scale contrast
of order 1: one wrong level or texel moves a pixel by far more than any bar) with alpha in [0.2, 1], a few texels at
exactly 1 (the 0.999 clamp of the compositing) and a few at 0."""
import numpy as np
import pytest

from adaptive_ref import refined_mask
from supersample_ref import box_resolve

pytestmark = pytest.mark.gpu

IN_DOMAIN = [(2, 6), (4, 12), (8, 24), (16, 48), (2, 64), (64, 4)]
FLOOR_HALVED = [(37, 101), (36, 100), (5, 7), (3, 3), (1, 8)]
DISK_SHAPES = IN_DOMAIN + FLOOR_HALVED
SKY_SHAPES = [(1, 1), (1, 3), (2, 2), (37, 101), (64, 64), (5, 512)]
FRAMES = [0, 3599, -40]          # the bench video's last frame; a negative offset: the phi < 0 wrap loop
VIEWS = {
    # compare_aa.py:43 view (the far_aa fixture's): far camera, strong minification
    "far_aa": dict(cam=[-20.0, 0.0, 2.0], fov=60.0, kw=dict(
        step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=20.0, anti_alias="lod_radius", aa_strength=1.5)),
    # camera inside the annulus, just above the plane: several crossings per ray, grazing footprints
    "inside_aa": dict(cam=[3.2, 0.5, 0.12], fov=100.0, kw=dict(
        step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=9.0, disk_tilt=3.0, anti_alias="lod_radius", aa_strength=2.0)),
}
W, H = 48, 27                    # ragged against the 8 x 8 tile in both directions
OTHER_COMPILATIONS = [(4, 12), (37, 101), (2, 64)]
T = 0.25                         # test_gpu_adaptive_supersample.py's threshold


def n_levels(n_r, n_phi):
    """Levels of the mip chain: halved while both sides are at least 2, five at the most (render.py:1113-1125)."""
    n = 1
    while n < 5 and n_r >= 2 and n_phi >= 2:
        n_r, n_phi, n = n_r // 2, n_phi // 2, n + 1
    return n


def random_disk(n_r, n_phi):
    rng = np.random.default_rng([11, n_r, n_phi])
    tex = rng.random((n_r, n_phi, 4), dtype=np.float32)
    tex[..., 3] = 0.2 + 0.8 * tex[..., 3]
    m = max(1, n_r * n_phi // 12)
    pick = rng.choice(n_r * n_phi, size=2 * m, replace=False)
    alpha = tex[..., 3].reshape(-1)
    alpha[pick[:m]] = 1.0
    alpha[pick[m:]] = 0.0
    return np.ascontiguousarray(tex)


def random_sky(h, w):
    return np.random.default_rng([13, h, w]).random((h, w, 3), dtype=np.float32)


def case(shape, view):
    """-> sky shape, frame, camera, fov, renderer arguments.  Skies cycle over the disk shapes, frames over shapes and views."""
    i, j = DISK_SHAPES.index(shape), sorted(VIEWS).index(view)
    v = VIEWS[view]
    return SKY_SHAPES[i % len(SKY_SHAPES)], FRAMES[(i + j) % len(FRAMES)], v["cam"], v["fov"], v["kw"]


_marched = {}


def oracle_march(oracle, shape, view, w=W, h=H, build=False):
    """(bg, disk) as (h, w, 3), the step total and the per-pixel largest asked lod (h, w) of the oracle's C march of a case:
    computed once, shared, read-only."""
    key = (shape, view, w, h, build)
    if key not in _marched:
        sky_shape, frame, cam, fov, kw = case(shape, view)
        o = oracle.OracleRenderer(w, h, random_sky(*sky_shape), random_disk(*shape), fast=build, **kw)
        assert o.num_mip_levels == n_levels(*shape)
        lods = np.ascontiguousarray(o.asked_lods(cam, fov, frame=frame).T)
        bg, disk = (np.ascontiguousarray(x.transpose(1, 0, 2)) for x in o.march(cam, fov, frame=frame, want_steps=False))
        for a in (bg, disk, lods):
            a.setflags(write=False)
        _marched[key] = (bg, disk, o.last_total_steps, lods)
    return _marched[key]


def hip_frame(shape, view, w=W, h=H, math="strict", final=False, **kw):
    """BG, DISK (and FINAL: the frame with its post-pass), ray-step total and mip_lds_level of one frame of a fresh context."""
    from bhr_amd import HipRenderer, _lib
    sky_shape, frame, cam, fov, rkw = case(shape, view)
    ctor = {k: kw.pop(k) for k in ("rows", "supersample", "supersample_threshold") if k in kw}
    r = HipRenderer(w, h, random_sky(*sky_shape), random_disk(*shape), math=math, **ctor, **rkw)
    try:
        assert r.num_mip_levels == n_levels(*shape)
        r.render_async(cam, fov, frame=frame, skip_bloom=not final, **kw)
        out = dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), steps=r.counters()["ray_steps"],
                   lds=r.mip_lds_level())
        if final:
            out["final"] = r.read_layer(_lib.LAYER_FINAL)
    finally:
        r.close()
    return out


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)))


def assert_matches_oracle(got, bg, disk, steps, tag):
    """The bars of test_gpu_fuzz.py::test_random_view_matches_oracle."""
    assert np.isfinite(got["bg"]).all() and np.isfinite(got["disk"]).all(), tag
    d_bg, d_disk = np.abs(got["bg"] - bg).max(), np.abs(got["disk"] - disk).max()
    print(f"\n[{tag}] bg max {d_bg:.3g} rmse {_rmse(got['bg'], bg):.3g}; disk max {d_disk:.3g} rmse {_rmse(got['disk'], disk):.3g}")
    if steps is not None:
        assert got["steps"] == steps, tag
    assert d_bg <= 2e-4 and d_disk <= 2e-4, (tag, d_bg, d_disk)
    assert _rmse(got["disk"], disk) <= 1e-5 and _rmse(got["bg"], bg) <= 1e-5, tag


def assert_lit(disk, tag):
    """An all-black frame cannot pass: the disk layer is really lit."""
    assert disk.max() > 0.05 and (disk.max(axis=2) > 0).mean() > 0.02, (tag, float(disk.max()), float((disk.max(axis=2) > 0).mean()))


_IDS = [f"{a}x{b}" for a, b in DISK_SHAPES]


# --------------------------------------------------------------------------- b. strict against the oracle, every shape
@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("shape", DISK_SHAPES, ids=_IDS)
def test_strict_march_matches_oracle(shape, view, oracle, hip_lib):
    bg, disk, steps, lods = oracle_march(oracle, shape, view)
    assert_lit(disk, (shape, view))
    if n_levels(*shape) < 4:
        # not vacuous: crossings of this frame ask for a level above the chain's last (the oracle's count of the lod that
        # shade_hit computes, render.py:2961-2989).  A sampler that clamps to the five stored levels reads the empty levels
        # there -- or, where n / 2^level is below 1, wraps its column index modulo zero
        beyond = int((lods.astype(np.int32) >= n_levels(*shape)).sum())
        print(f"\n[{shape} {view}] {beyond} of {W * H} pixels ask for a level beyond the last ({n_levels(*shape) - 1})")
        assert beyond > 0, (shape, view)
    assert_matches_oracle(hip_frame(shape, view), bg, disk, steps, f"{shape} {view} strict")


# --------------------------------------------------------------------------- c. the other compilations of the sampler
@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("shape", OTHER_COMPILATIONS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_persistent_march_matches_oracle(shape, view, oracle, hip_lib):
    """compaction=True: march_persistent_kernel, an object of its own."""
    bg, disk, steps, _ = oracle_march(oracle, shape, view)
    assert_matches_oracle(hip_frame(shape, view, compaction=True), bg, disk, steps, f"{shape} {view} persistent")


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("shape", OTHER_COMPILATIONS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_supersampled_and_adaptive_march(shape, view, oracle, hip_lib):
    """supersample=2 (the _ss twins of the tile kernels) and its adaptive form (the list kernels), strict.  As in
    test_gpu_supersample.py / test_gpu_adaptive_supersample.py: bit for bit the box filter of the k = 1 render at 2W x 2H,
    and the k = 1 frame with the pixels of the NumPy mask (computed from the GPU's own k = 1 frame) replaced by the SSAA
    frame's.  And, with the oracle feeding the same two references, within the bars of the strict test above."""
    k = 2
    one, fine, ss = hip_frame(shape, view), hip_frame(shape, view, k * W, k * H), hip_frame(shape, view, supersample=k)
    ada = hip_frame(shape, view, supersample=k, supersample_threshold=T)
    mask = refined_mask(one["bg"], one["disk"], T)
    assert 0.05 <= mask.mean() <= 0.95, float(mask.mean())
    for layer in ("bg", "disk"):
        np.testing.assert_array_equal(ss[layer], box_resolve(fine[layer], k), err_msg=f"{shape} {view} {layer}")
        np.testing.assert_array_equal(ada[layer], np.where(mask[..., None], ss[layer], one[layer]), err_msg=f"{shape} {view} {layer}")
    assert ss["steps"] == fine["steps"] and ada["steps"] > one["steps"]
    o_bg, o_disk, _, _ = oracle_march(oracle, shape, view)
    f_bg, f_disk, f_steps, _ = oracle_march(oracle, shape, view, k * W, k * H)
    r_bg, r_disk = box_resolve(f_bg, k), box_resolve(f_disk, k)
    assert_matches_oracle(ss, r_bg, r_disk, f_steps, f"{shape} {view} ss")
    assert_matches_oracle(ada, np.where(mask[..., None], r_bg, o_bg), np.where(mask[..., None], r_disk, o_disk), None,
                          f"{shape} {view} adaptive")


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("shape", OTHER_COMPILATIONS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_block_equals_rows_of_the_full_frame(shape, view, hip_lib):
    full, block = hip_frame(shape, view), hip_frame(shape, view, rows=(8, 19))
    assert block["bg"].shape == (11, W, 3)
    np.testing.assert_array_equal(block["bg"], full["bg"][8:19])
    np.testing.assert_array_equal(block["disk"], full["disk"][8:19])


# --------------------------------------------------------------------------- d. the fast object
@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("shape", OTHER_COMPILATIONS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fast_march_against_strict(shape, view, hip_lib):
    """The caps of test_gpu_parity.py::test_fast_march_in_the_rays_own_clock_radial_and_extreme_rays.  They are a condition:
    a wrong level moves the disk by up to 0.95 on the pixels that asked for it, far more than 1 % of this frame."""
    from bhr_amd import HipRenderer, _lib
    sky_shape, frame, cam, fov, kw = case(shape, view)
    r = HipRenderer(W, H, random_sky(*sky_shape), random_disk(*shape), math="fast", **kw)
    out = {}
    try:
        for math in ("strict", "fast"):
            r.render_async(cam, fov, frame=frame, math=math)
            out[math] = dict(final=r.read_layer(_lib.LAYER_FINAL), disk=r.read_layer(_lib.LAYER_DISK), steps=r.counters()["ray_steps"])
    finally:
        r.close()
    f, s = out["fast"], out["strict"]
    assert_lit(s["disk"], (shape, view))
    assert abs(f["steps"] - s["steps"]) <= 5e-3 * s["steps"], (f["steps"], s["steps"])
    for layer in ("final", "disk"):
        assert np.isfinite(f[layer]).all()
        d = np.abs(f[layer] - s[layer]).max(axis=2)
        print(f"\n[{shape} {view} fast/{layer}] beyond 0.05: {(d > 0.05).mean():.4f}, median {np.median(d):.3g}, max {d.max():.3g}")
        assert (d > 0.05).mean() <= 0.01, (layer, float((d > 0.05).mean()))
        assert np.median(d) <= 1e-5, (layer, float(np.median(d)))


def expected_lds_level(n_r, n_phi):
    """The launcher's rule (csrc/march_launch.hip): nothing where level 3 is empty; else as many of levels 3, 2, 1 as fit
    44 KB together with every level between them and 3 (16 bytes a texel)."""
    dims = [(n_r, n_phi)]
    for _ in range(3):
        h, w = dims[-1]
        dims.append((h // 2, w // 2) if h >= 2 and w >= 2 else (0, 0))
    if dims[3][0] * dims[3][1] == 0:
        return -1
    level = -1
    for first in (3, 2, 1):
        if 16 * sum(h * w for h, w in dims[first:4]) > 44 * 1024:
            break
        level = first
    return level


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("shape", OTHER_COMPILATIONS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_lds_staged_levels_give_the_same_bits(shape, view, hip_lib, monkeypatch):
    """BHR_MIP_LDS=1 (march_tile_mipstaged_kernel): the plain kernel's bits; no staging where the chain has no level 3."""
    frames = {}
    for on in ("0", "1"):
        monkeypatch.setenv("BHR_MIP_LDS", on)
        frames[on] = hip_frame(shape, view, math="fast")
    assert frames["0"]["lds"] == -1
    assert frames["1"]["lds"] == expected_lds_level(*shape), (shape, frames["1"]["lds"])
    assert_lit(frames["0"]["disk"], (shape, view))
    np.testing.assert_array_equal(frames["1"]["disk"], frames["0"]["disk"])
    np.testing.assert_array_equal(frames["1"]["bg"], frames["0"]["bg"])
    assert frames["1"]["steps"] == frames["0"]["steps"]


def test_expected_lds_level_is_the_rule_test_gpu_mip_lds_pins():
    assert [expected_lds_level(*s) for s in ((128, 256), (128, 512), (256, 1024))] == [2, 3, -1]
    assert [expected_lds_level(*s) for s in OTHER_COMPILATIONS] == [-1, 1, -1]


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("shape", OTHER_COMPILATIONS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hybrid_against_strict(shape, view, oracle, hip_lib):
    """math="hybrid", guards as the library picks them, at 192 x 128.  Step totals within 2e-4 and no pixel beyond 0.05, as in
    test_gpu_fuzz.py::test_random_view_hybrid_against_strict; per-channel RMSE within that test's 6e-5, or, where the f32
    noise of the march itself is larger, within the yardstick of
    test_gpu_fuzz.py::test_telephoto_views_hybrid_within_the_f32_noise_of_the_march: 1.5 x the distance of the strict march
    from the oracle's binary64 build on the same frame, for hybrid against strict and for hybrid against binary64.  (No
    pixels are set aside here as that test sets two aside.)  Texel-scale noise of contrast 1 turns an ulp of a grazing hit
    point into far more colour than scenes.noisy_disk does: 37 x 101 seen from inside the annulus has hybrid 9.0e-5 (disk) /
    5.9e-5 (bg) from strict, largest pixel 4.6e-3, with (b) passing on the same case; DESIGN section 2 has every figure."""
    from bhr_amd import HipRenderer, _lib
    w, h = 192, 128
    sky_shape, frame, cam, fov, kw = case(shape, view)
    r = HipRenderer(w, h, random_sky(*sky_shape), random_disk(*shape), math="hybrid", **kw)
    lay, steps = {}, {}
    try:
        for math in ("hybrid", "strict"):
            r.render_async(cam, fov, frame=frame, skip_bloom=True, math=math)
            lay[math] = dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK))
            steps[math] = r.counters()["ray_steps"]
    finally:
        r.close()
    o = oracle.OracleRenderer(w, h, random_sky(*sky_shape), random_disk(*shape), fast="f64", **kw)
    lay["f64"] = dict(zip(("bg", "disk"), (x.transpose(1, 0, 2) for x in o.march(cam, fov, frame=frame, want_steps=False))))

    def rm(a, b):
        return float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2, axis=(0, 1))).max())
    assert abs(steps["hybrid"] - steps["strict"]) <= max(2e-4 * steps["strict"], 64), steps
    failed = []
    for name in ("bg", "disk"):
        a, b, c = lay["hybrid"][name], lay["strict"][name], lay["f64"][name]
        assert np.isfinite(a).all()
        e_hs, e_s64, e_h64 = rm(a, b), rm(b, c), rm(a, c)
        flips = int((np.abs(a - b).max(axis=2) > 0.05).sum())
        print(f"\n[{shape} {view} hybrid/{name}] hybrid-strict {e_hs:.3g} (max {np.abs(a - b).max():.3g}, beyond 0.05: {flips}), "
              f"strict-binary64 {e_s64:.3g}, hybrid-binary64 {e_h64:.3g}")
        if flips or max(e_hs, e_h64) > max(6e-5, 1.5 * e_s64):
            failed.append((name, e_hs, e_h64, e_s64, flips))
    assert not failed, f"{shape} {view}: (layer, hybrid-strict, hybrid-binary64, strict-binary64, pixels beyond 0.05) {failed}"
