"""Adaptive supersampling on the device (bhr_set_adaptive_supersample; include/bhr.h states the function): a frame is the
k = 1 frame with the pixels whose neighbours differ by more than T replaced by their values in the SSAA-k frame -- bit for
bit under strict and fast, under hybrid by the arithmetic of the fine frame's tile.  The mask is always computed in NumPy
(tests/adaptive_ref.py) from the GPU's own k = 1 frame.  Degenerate thresholds, counters, Disk V2 sources, the post-pass,
setting changes on one context, frame slots, the video loop, the CLI and the refusals."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import hybrid_band as hb
from adaptive_ref import contrast, refined_mask
from supersample_ref import box_resolve
from test_gpu_supersample import KW, VIEWS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 0.25
VIEWS3 = dict(VIEWS, wide=dict(W=96, H=54, cam=[6.0, 0.0, 0.5], fov=90.0, tilt=0.0))
INF = float("inf")


def _scene():
    from bhr_amd import scenes
    return scenes.analytic_skybox(), scenes.noisy_disk()


def _frame(W, H, cam, fov, math, k=1, threshold=None, source=None, frozen_kw=()):
    """BG, DISK, counters (adaptive_info, hybrid_info) of one frame of a fresh context."""
    from bhr_amd import HipRenderer, _lib
    sky, tex = _scene()
    r = HipRenderer(W, H, sky, tex, math=math, supersample=k, supersample_threshold=threshold, **dict(frozen_kw))
    if source:
        from bhr_amd.disk_v2 import DiskV2Params
        r.use_disk_v2(DiskV2Params(), volume=source == "v2_volume")     # (params=None would switch BACK to the texture)
        assert r._dv2 is not None
    r.render_async(cam, fov, skip_bloom=True)
    out = dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), c=r.counters())
    if threshold is not None and k > 1:
        out["ada"] = r.adaptive_info()
    if math == "hybrid":
        out["info"] = r.hybrid_info()
        out["uniforms"] = hb.cam_from_uniforms(r.camera_uniforms(cam, fov))
    r.close()
    return out


@functools.lru_cache(maxsize=None)
def _cached(W, H, cam, fov, math, k, frozen_kw, source=None):
    """The k = 1 and SSAA-k frames of a view are shared by the thresholds and factors tested against them."""
    return _frame(W, H, list(cam), fov, math, k, None, source, frozen_kw)


def _fk(kw):
    return tuple(sorted(kw.items()))


def _where(mask, ss, one):
    return {layer: np.where(mask[..., None], ss[layer], one[layer]) for layer in ("bg", "disk")}


def _assert_layers(got, want, tag):
    for layer in ("bg", "disk"):
        bad = int((got[layer] != want[layer]).any(axis=2).sum())
        assert bad == 0, f"{tag} {layer}: {bad} pixels differ"


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("aa", ["disabled", "lod_radius"])
@pytest.mark.parametrize("math", ["strict", "fast"])
@pytest.mark.parametrize("view", sorted(VIEWS3))
def test_the_definition_strict_and_fast(view, math, aa, k, hip_lib):
    v = VIEWS3[view]
    kw = _fk(dict(KW, disk_tilt=v["tilt"], anti_alias=aa))
    one = _cached(v["W"], v["H"], tuple(v["cam"]), v["fov"], math, 1, kw)
    ss = _cached(v["W"], v["H"], tuple(v["cam"]), v["fov"], math, k, kw)
    mask = refined_mask(one["bg"], one["disk"], T)
    print(f"\n[{view} {math} {aa} k={k}] refined share {mask.mean():.3f}")
    assert 0.05 <= mask.mean() <= 0.95, mask.mean()
    got = _frame(v["W"], v["H"], v["cam"], v["fov"], math, k, T, frozen_kw=kw)
    _assert_layers(got, _where(mask, ss, one), f"{view} {math} {aa} k={k}")
    n = int(mask.sum())
    assert got["ada"] == dict(refined=n, strict=n if math == "strict" else 0, pixels=v["W"] * v["H"])
    assert got["c"]["rays"] == v["W"] * v["H"] + k * k * n


@pytest.mark.parametrize("math", ["strict", "fast", "hybrid"])
def test_degenerate_thresholds(math, hip_lib):
    v, k = VIEWS3["wide"], 4                                          # tilt 0, no AA: a hybrid frame without guards
    W, H = v["W"], v["H"]
    kw = _fk(dict(KW, disk_tilt=0.0, anti_alias="disabled"))
    one = _cached(W, H, tuple(v["cam"]), v["fov"], math, 1, kw)
    ss = _cached(W, H, tuple(v["cam"]), v["fov"], math, k, kw)
    if math == "hybrid":
        assert one["info"]["repaired_pixels"] == 0 and ss["info"]["repaired_pixels"] == 0
    none = _frame(W, H, v["cam"], v["fov"], math, k, INF, frozen_kw=kw)
    _assert_layers(none, one, f"{math} T=+inf")
    assert none["ada"]["refined"] == 0 and none["c"]["rays"] == W * H
    assert none["c"]["ray_steps"] == one["c"]["ray_steps"] > 0
    every = _frame(W, H, v["cam"], v["fov"], math, k, -1.0, frozen_kw=kw)
    _assert_layers(every, ss, f"{math} T=-1")
    assert every["ada"]["refined"] == W * H and every["c"]["rays"] == W * H * (1 + k * k)
    assert every["c"]["ray_steps"] == one["c"]["ray_steps"] + ss["c"]["ray_steps"]
    # T = 0 with the shadow in frame: pixels whose neighbours equal them exist, and keep their k = 1 bits
    c = contrast(one["bg"], one["disk"])
    assert (c == 0).any() and (c > 0).any()
    zero = _frame(W, H, v["cam"], v["fov"], math, k, 0.0, frozen_kw=kw)
    _assert_layers(zero, _where(c > 0, ss, one), f"{math} T=0")
    assert zero["ada"]["refined"] == int((c > 0).sum())


def _fine_tile_flags(one, W, H, k, tilt, step):
    """strict flag and decision margin per OUTPUT pixel: those of the 8 x 8 tile of the fine frame that holds its group."""
    cam = one["uniforms"]
    fine_cam = hb.Cam(cam.pos, cam.right, cam.up, cam.forward, float(np.float32(cam.pw) / np.float32(k)),
                      float(np.float32(cam.ph) / np.float32(k)))
    lo, hi = hb.effective_band(step)
    flags, margin, _ = hb.tile_flags(fine_cam, k * W, k * H, 0, k * H, tilt, lo, hi)
    ty, tx = (np.arange(H) * k) // 8, (np.arange(W) * k) // 8
    return flags[np.ix_(ty, tx)], margin[np.ix_(ty, tx)]


@pytest.mark.parametrize("k", [2, 4])
def test_hybrid_without_guards(k, hip_lib):
    W, H, cam, fov = 96, 54, (6.0, 0.0, 0.5), 90.0
    kw = _fk(dict(KW, disk_tilt=0.0, anti_alias="disabled"))
    one = _cached(W, H, cam, fov, "hybrid", 1, kw)
    ss = _cached(W, H, cam, fov, "hybrid", k, kw)
    assert one["info"]["repaired_pixels"] == 0 and ss["info"]["repaired_pixels"] == 0
    mask = refined_mask(one["bg"], one["disk"], T)
    assert 0.05 <= mask.mean() <= 0.95
    got = _frame(W, H, list(cam), fov, "hybrid", k, T, frozen_kw=kw)
    _assert_layers(got, _where(mask, ss, one), f"hybrid k={k}")
    assert got["ada"]["refined"] == int(mask.sum()) and got["ada"]["pixels"] == W * H
    assert 0 < got["ada"]["strict"] < got["ada"]["refined"], got["ada"]
    flags, margin = _fine_tile_flags(one, W, H, k, 0.0, KW["step_size"])
    sure = margin >= 1e-6
    lo_n, hi_n = int((mask & flags & sure).sum()), int((mask & (flags | ~sure)).sum())
    assert lo_n <= got["ada"]["strict"] <= hi_n, (got["ada"], lo_n, hi_n)


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("guard", ["aa", "tilt"])
def test_hybrid_with_guards_in_the_base_frame(guard, k, hip_lib):
    W, H, cam, fov = 160, 90, (6.0, 0.0, 0.5), 90.0
    tilt = 20.0 if guard == "tilt" else 0.0
    kw = _fk(dict(KW, disk_tilt=tilt, anti_alias="lod_radius" if guard == "aa" else "disabled", aa_strength=1.5))
    one = _cached(W, H, cam, fov, "hybrid", 1, kw)
    fine_fast = _cached(k * W, k * H, cam, fov, "fast", 1, kw)
    fine_strict = _cached(k * W, k * H, cam, fov, "strict", 1, kw)
    mask = refined_mask(one["bg"], one["disk"], T)
    got = _frame(W, H, list(cam), fov, "hybrid", k, T, frozen_kw=kw)
    assert got["ada"]["refined"] == int(mask.sum())

    def match(ref):
        return ~((got["bg"] != ref["bg"]).any(axis=2) | (got["disk"] != ref["disk"]).any(axis=2))
    keep = match(one)
    assert keep[~mask].all(), f"{int((~keep[~mask]).sum())} unrefined pixels differ from the hybrid k = 1 frame"
    mf = match({layer: box_resolve(fine_fast[layer], k) for layer in ("bg", "disk")})
    ms = match({layer: box_resolve(fine_strict[layer], k) for layer in ("bg", "disk")})
    assert (mf | ms)[mask].all(), f"{int((~(mf | ms))[mask].sum())} refined pixels are the filter of neither render"
    flags, margin = _fine_tile_flags(one, W, H, k, tilt, KW["step_size"])
    sure = margin >= 1e-6
    strict_px, fast_px = mask & flags & sure, mask & ~flags & sure
    print(f"\n[hybrid {guard} k={k}] refined {int(mask.sum())}: strict {int(strict_px.sum())}, fast {int(fast_px.sum())}, "
          f"tie tiles' pixels {int((mask & ~sure).sum())}")
    assert strict_px.any() and fast_px.any()
    assert ms[strict_px].all(), f"{int((~ms[strict_px]).sum())} groups of strict tiles are not the strict filter"
    assert mf[fast_px].all(), f"{int((~mf[fast_px]).sum())} groups of fast tiles are not the fast filter"
    assert int(strict_px.sum()) <= got["ada"]["strict"] <= int((mask & (flags | ~sure)).sum()), got["ada"]


@pytest.mark.parametrize("source", ["v2", "v2_volume"])
def test_disk_v2_sources(source, hip_lib):
    W, H, cam, fov, k = 20, 12, (9.0, 0.0, 1.2), 60.0, 2
    kw = _fk(dict(KW, r_disk_outer=10.0, disk_tilt=0.0, anti_alias="disabled"))
    one = _cached(W, H, cam, fov, "strict", 1, kw, source)
    ss = _cached(W, H, cam, fov, "strict", k, kw, source)
    assert ss["disk"].max() > 0
    thr = float(np.median(contrast(one["bg"], one["disk"])))          # from the k = 1 frame's own contrast
    mask = refined_mask(one["bg"], one["disk"], thr)
    assert 0.05 <= mask.mean() <= 0.95, mask.mean()
    got = _frame(W, H, list(cam), fov, "strict", k, thr, source, frozen_kw=kw)
    _assert_layers(got, _where(mask, ss, one), source)
    assert got["ada"] == dict(refined=int(mask.sum()), strict=int(mask.sum()), pixels=W * H)


@pytest.mark.parametrize("math", ["strict", "hybrid"])
def test_post_pass_runs_on_the_adaptive_layers(math, hip_lib):
    from bhr_amd import HipRenderer, _lib
    sky, tex = _scene()
    W, H, cam, fov = 160, 90, [6.0, 0.0, 0.5], 90.0
    r = HipRenderer(W, H, sky, tex, math=math, supersample=2, supersample_threshold=T, **KW)
    final = r.render(cam, fov)
    bg, disk = r.read_layer(_lib.LAYER_BG), r.read_layer(_lib.LAYER_DISK)
    u8 = r.read_final_u8()
    n = r.adaptive_info()["refined"]
    r.close()
    assert 0 < n < W * H
    p = HipRenderer(W, H, sky, tex, math=math, **KW)
    p.write_layer(_lib.LAYER_BG, bg)
    p.write_layer(_lib.LAYER_DISK, disk)
    p.bloom_only()
    want = p.read_layer(_lib.LAYER_FINAL)
    p.close()
    assert np.array_equal(final, want)
    assert np.array_equal(u8, (np.clip(final, 0, 1) * np.float32(255)).astype(np.uint8))


def test_setting_changes_on_one_context(hip_lib):
    from bhr_amd import HipRenderer, _lib
    sky, tex = _scene()
    W, H, cam, fov = 40, 24, [6.0, 0.0, 0.5], 90.0
    kw = dict(KW, disk_tilt=20.0, anti_alias="lod_radius")        # hybrid with guards: tile order, lists and fix lists all in play
    settings = [(1, None), (2, T), (4, None), (4, 0.05), (1, None)]
    fresh = {s: _frame(W, H, cam, fov, "hybrid", s[0], s[1], frozen_kw=_fk(kw)) for s in set(settings)}
    r = HipRenderer(W, H, sky, tex, math="hybrid", **kw)
    for k, thr in settings:
        r.set_supersample(k, thr)
        assert r.supersample == k and r.supersample_threshold == (None if thr is None else float(np.float32(thr)))
        for _ in range(2):                                          # both frame slots
            r.render_async(cam, fov, skip_bloom=True)
        got = dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK))
        _assert_layers(got, fresh[(k, thr)], f"setting {(k, thr)}")
        if thr is not None:
            assert r.adaptive_info() == fresh[(k, thr)]["ada"]
        else:
            with pytest.raises(AssertionError):                     # BHR_ERR_STATE: not adaptive
                r.adaptive_info()
    r.close()


def test_frame_slots_and_repeats(hip_lib):
    from bhr_amd import HipRenderer, _lib
    from bhr_amd.camera import orbit_position
    sky, tex = _scene()
    W, H, fov, pov, k = 64, 36, 90.0, [6.0, 0.0, 0.5], 2
    kw = dict(KW, disk_tilt=0.0, anti_alias="disabled")
    frames = {}
    for slots in (1, 2):
        r = HipRenderer(W, H, sky, tex, math="hybrid", frame_slots=slots, supersample=k, supersample_threshold=T, **kw)
        with pytest.raises(AssertionError):                         # BHR_ERR_STATE before the first adaptive frame
            r.adaptive_info()
        out = []
        for f in list(range(6)) + [5]:                              # a changing camera, then the last frame once more
            r.render_async(orbit_position(pov, f, 12, 360.0), fov, skip_bloom=True)
            out.append((r.read_layer(_lib.LAYER_BG), r.read_layer(_lib.LAYER_DISK), r.adaptive_info()))
        r.close()
        frames[slots] = out
        assert np.array_equal(out[5][0], out[6][0]) and np.array_equal(out[5][1], out[6][1]) and out[5][2] == out[6][2]
    for a, b in zip(frames[1], frames[2]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert len({f[2]["refined"] for f in frames[1]}) > 1             # the camera did change what is refined


def test_video_frames_are_the_still_frames(tmp_path, hip_lib):
    from PIL import Image
    from bhr_amd import drivers
    from bhr_amd.camera import orbit_position
    W, H, n, k, fov, pov = 64, 36, 4, 2, 90.0, [6.0, 0.0, 0.5]
    r, _, _, _ = drivers.make_renderer(W, H, pov, fov, n_stars=600, tex_w=512, tex_h=256, frame_slots=2, math="hybrid")
    out = os.path.join(str(tmp_path), "v.mp4")
    drivers.render_video(r, W, H, n_frames=n, fps=30, output_path=out, fov=fov, static_cam_pos=pov, orbit=True,
                         assemble=False, video_stream="off", supersample=k, supersample_threshold=T)
    assert r.supersample == k and r.supersample_threshold == T
    assert 0 < r.adaptive_info()["refined"] < W * H
    r.close()
    s, _, n_r, n_phi = drivers.make_renderer(W, H, pov, fov, n_stars=600, tex_w=512, tex_h=256, frame_slots=1, math="hybrid",
                                             supersample=k, supersample_threshold=T)
    factories = drivers.init_lifecycle_system(s, n_r, n_phi, seed=42)
    dt = 0.1
    for f in range(n):
        drivers.advance_lifecycle_frame(s, factories, f * dt, dt, recompute_stats=(f % 60 == 0), compose=True)
        s.render_async(orbit_position(pov, f, n, 360.0), fov, frame=0)
        want = s.read_final_u8()
        got = np.asarray(Image.open(os.path.join(drivers._frames_dir(out), f"frame_{f:04d}.png")).convert("RGB"))
        assert np.array_equal(got, want), f
    s.close()


def test_refusals(hip_lib):
    from bhr_amd import HipRenderer, _lib
    sky, tex = _scene()
    cam, fov = [6.0, 0.0, 0.5], 90.0
    r = HipRenderer(64, 36, sky, tex, math="strict", supersample=2, supersample_threshold=T, **KW)
    with pytest.raises(ValueError):
        r.render_async(cam, fov, compaction=True)                  # BHR_PERSISTENT
    with pytest.raises(ValueError):
        r.row_costs(cam, fov)                                       # BHR_ROW_COSTS
    uni = r.camera_uniforms(cam, fov)
    ctxs = (C.c_void_p * 1)(r._ctx)
    assert hip_lib.bhr_group_render(ctxs, 1, C.byref(uni), 0, None) == _lib.BHR_ERR_INVALID
    handles = _lib.TileHandles()
    assert hip_lib.bhr_tile_export(r._ctx, 0, C.byref(handles)) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_tile_render(r._ctx, C.byref(uni), 0) == _lib.BHR_ERR_INVALID
    for k in (0, 3, 16):
        assert hip_lib.bhr_set_adaptive_supersample(r._ctx, k, T) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_set_adaptive_supersample(r._ctx, 2, float("nan")) == _lib.BHR_ERR_INVALID
    assert r.supersample == 2 and r.supersample_threshold == T
    r.render(cam, fov)                                              # and the context still renders, adaptively
    assert 0 < r.adaptive_info()["refined"] < 64 * 36
    r.set_supersample(1, T)                                         # k = 1 turns supersampling off
    assert r.supersample_threshold is None
    r.render(cam, fov)
    with pytest.raises(AssertionError):
        r.adaptive_info()
    r.close()
    with pytest.raises(ValueError):
        HipRenderer(64, 36, sky, tex, rows=(0, 16), supersample=2, supersample_threshold=T, **KW)
    big = HipRenderer(8192, 4096, sky, tex, frame_slots=1, **KW)   # 64 x 2^25 rays = 2^31
    with pytest.raises(ValueError):
        big.set_supersample(8, T)
    big.set_supersample(4, T)
    big.close()


def test_cli_matches_render_image(tmp_path, hip_lib):
    from PIL import Image
    from bhr_amd import drivers
    out = os.path.join(str(tmp_path), "cli.png")
    subprocess.run([sys.executable, os.path.join(ROOT, "render.py"), "-r", "sd", "--supersample", "2", "--supersample_threshold",
                    "0.03", "--math", "strict", "--n_stars", "600", "-o", out], check=True, cwd=ROOT, timeout=600)
    img = drivers.render_image(640, 360, [6, 0, 0.5], 90, 0.1, n_stars=600, supersample=2, supersample_threshold=0.03,
                               math="strict")
    ref = os.path.join(str(tmp_path), "api.png")
    drivers.save_image(img, ref)
    a = np.asarray(Image.open(out).convert("RGB"))
    b = np.asarray(Image.open(ref).convert("RGB"))
    assert a.shape == (360, 640, 3) and np.array_equal(a, b)
    plain = drivers.render_image(640, 360, [6, 0, 0.5], 90, 0.1, n_stars=600, math="strict")
    assert not np.array_equal(img, plain)                           # the threshold did refine something
