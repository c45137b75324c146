"""Supersampling on the device (bhr_set_supersample): a W x H frame with factor k has the BG and DISK layers of the k x k
box filter (tests/supersample_ref.py) of the k = 1 render of the same view at kW x kH -- bit for bit under the strict and
the fast arithmetic, and under hybrid without guards; with guards a pixel is the filter of the hybrid or of the strict
render, the latter only for the pixels bhr_hybrid_repairs counts.  The post-pass, the counters, factor changes on one
context, the video loop, the CLI and the refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from supersample_ref import box_resolve

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0)
VIEWS = {   # small frames: odd sizes (not multiples of the 8x8 tile), a tilted disk seen from off axis
    "odd": dict(W=21, H=13, cam=[6.0, 0.0, 0.5], fov=90.0, tilt=0.0),
    "tilt": dict(W=24, H=15, cam=[5.0, 2.0, 1.0], fov=70.0, tilt=20.0),
}


def _scene():
    from bhr_amd import scenes
    return scenes.analytic_skybox(), scenes.noisy_disk()


def _render(W, H, k, cam, fov, math, source=None, set_k=True, **kw):
    """BG, DISK, counters (and hybrid_info) of one frame; set_k=False: a context on which the factor was never set."""
    from bhr_amd import HipRenderer, _lib
    sky, tex = _scene()
    r = HipRenderer(W, H, sky, tex, math=math, **({"supersample": k} if set_k else {}), **kw)
    if source:
        from bhr_amd.disk_v2 import DiskV2Params
        r.use_disk_v2(DiskV2Params(), volume=source == "v2_volume")     # (params=None would switch BACK to the texture)
        assert r._dv2 is not None
    r.render_async(cam, fov, skip_bloom=True)
    out = dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), c=r.counters())
    if math == "hybrid":
        out["info"] = r.hybrid_info()
    r.close()
    return out


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _check_exact(ss, fine, k, tag):
    for layer in ("bg", "disk"):
        want = box_resolve(fine[layer], k)
        bad = int((ss[layer] != want).any(axis=2).sum())
        assert bad == 0, f"{tag} {layer}: {bad} pixels differ from the box filter of the k = 1 render"


@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("aa", ["disabled", "lod_radius"])
@pytest.mark.parametrize("math", ["strict", "fast"])
@pytest.mark.parametrize("view", sorted(VIEWS))
def test_strict_and_fast_are_the_box_filter_of_the_fine_render(view, math, aa, k, hip_lib):
    v = VIEWS[view]
    kw = dict(KW, disk_tilt=v["tilt"], anti_alias=aa)
    ss = _render(v["W"], v["H"], k, v["cam"], v["fov"], math, **kw)
    fine = _render(k * v["W"], k * v["H"], 1, v["cam"], v["fov"], math, **kw)
    _check_exact(ss, fine, k, f"{view} {math} {aa} k={k}")


@pytest.mark.parametrize("k", [2, 4])
def test_hybrid_without_guards_is_the_box_filter_of_the_fine_hybrid_render(k, hip_lib):
    W, H, cam, fov = 96, 54, [6.0, 0.0, 0.5], 90.0
    kw = dict(KW, disk_tilt=0.0, anti_alias="disabled")
    ss = _render(W, H, k, cam, fov, "hybrid", **kw)
    fine = _render(k * W, k * H, 1, cam, fov, "hybrid", **kw)
    assert ss["info"]["strict_tiles"] > 0 and ss["info"]["repaired_pixels"] == 0
    assert ss["info"]["strict_tiles"] == fine["info"]["strict_tiles"] and ss["info"]["tiles"] == fine["info"]["tiles"]
    _check_exact(ss, fine, k, f"hybrid k={k}")


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("guard", ["aa", "tilt"])
def test_hybrid_with_guards_repairs_whole_groups(guard, k, hip_lib):
    W, H, cam, fov = 160, 90, [6.0, 0.0, 0.5], 90.0
    kw = dict(KW, disk_tilt=20.0 if guard == "tilt" else 0.0, anti_alias="lod_radius" if guard == "aa" else "disabled",
              aa_strength=1.5)
    ss = _render(W, H, k, cam, fov, "hybrid", **kw)
    hyb = _render(k * W, k * H, 1, cam, fov, "hybrid", **kw)
    st = _render(k * W, k * H, 1, cam, fov, "strict", **kw)

    def match(ref):
        return ~((ss["bg"] != box_resolve(ref["bg"], k)).any(axis=2) | (ss["disk"] != box_resolve(ref["disk"], k)).any(axis=2))
    mh, ms = match(hyb), match(st)
    assert (mh | ms).all(), f"{int((~(mh | ms)).sum())} pixels are the filter of neither render"
    only_strict = int((ms & ~mh).sum())
    rep = ss["info"]["repaired_pixels"]
    assert only_strict <= rep, (only_strict, ss["info"])
    assert ss["info"]["repair_capacity"] == hyb["info"]["repair_capacity"] // (k * k)


@pytest.mark.parametrize("source", ["v2", "v2_volume"])
def test_disk_v2_sources(source, hip_lib):
    W, H, cam, fov, k = 20, 12, [9.0, 0.0, 1.2], 60.0, 2
    kw = dict(KW, r_disk_outer=10.0, disk_tilt=0.0, anti_alias="disabled")
    ss = _render(W, H, k, cam, fov, "strict", source=source, **kw)
    fine = _render(k * W, k * H, 1, cam, fov, "strict", source=source, **kw)
    assert ss["disk"].max() > 0
    _check_exact(ss, fine, k, source)


def test_post_pass_runs_on_the_resolved_layers(hip_lib):
    from bhr_amd import HipRenderer, _lib
    sky, tex = _scene()
    W, H, cam, fov = 160, 90, [6.0, 0.0, 0.5], 90.0
    r = HipRenderer(W, H, sky, tex, math="strict", supersample=2, **KW)
    final = r.render(cam, fov)
    bg, disk = r.read_layer(_lib.LAYER_BG), r.read_layer(_lib.LAYER_DISK)
    r.close()
    p = HipRenderer(W, H, sky, tex, math="strict", **KW)
    p.write_layer(_lib.LAYER_BG, bg)
    p.write_layer(_lib.LAYER_DISK, disk)
    p.bloom_only()
    want = p.read_layer(_lib.LAYER_FINAL)
    p.close()
    assert np.array_equal(final, want)


def test_factor_changes_on_one_context(hip_lib):
    from bhr_amd import HipRenderer, _lib
    sky, tex = _scene()
    W, H, cam, fov = 40, 24, [6.0, 0.0, 0.5], 90.0
    kw = dict(KW, disk_tilt=20.0, anti_alias="lod_radius")        # hybrid with guards: tile order, lists and fix lists all in play
    never = _render(W, H, 1, cam, fov, "hybrid", set_k=False, **kw)
    one = _render(W, H, 1, cam, fov, "hybrid", **kw)
    assert _same(never["bg"], one["bg"]) and _same(never["disk"], one["disk"])
    fresh = {k: _render(W, H, k, cam, fov, "hybrid", **kw) for k in (1, 2, 4)}
    r = HipRenderer(W, H, sky, tex, math="hybrid", **kw)
    for k in (2, 1, 4, 2):
        r.set_supersample(k)
        assert r.supersample == k
        for _ in range(2):                                          # both frame slots
            r.render_async(cam, fov, skip_bloom=True)
        bg, disk = r.read_layer(_lib.LAYER_BG), r.read_layer(_lib.LAYER_DISK)
        assert _same(bg, fresh[k]["bg"]) and _same(disk, fresh[k]["disk"]), k
    r.close()


@pytest.mark.parametrize("math", ["strict", "fast", "hybrid"])
def test_counters(math, hip_lib):
    W, H, cam, fov, k = 48, 27, [6.0, 0.0, 0.5], 90.0, 4
    kw = dict(KW, disk_tilt=0.0, anti_alias="disabled")
    ss = _render(W, H, k, cam, fov, math, **kw)
    fine = _render(k * W, k * H, 1, cam, fov, math, **kw)
    assert ss["c"]["rays"] == k * k * W * H == fine["c"]["rays"]
    assert ss["c"]["ray_steps"] == fine["c"]["ray_steps"] > 0


def test_video_frames_are_the_still_frames(tmp_path, hip_lib):
    from PIL import Image
    from bhr_amd import drivers
    from bhr_amd.camera import orbit_position
    W, H, n, k, fov, pov = 64, 36, 4, 2, 90.0, [6.0, 0.0, 0.5]
    r, _, _, _ = drivers.make_renderer(W, H, pov, fov, n_stars=600, tex_w=512, tex_h=256, frame_slots=2, math="hybrid")
    out = os.path.join(str(tmp_path), "v.mp4")
    drivers.render_video(r, W, H, n_frames=n, fps=30, output_path=out, fov=fov, static_cam_pos=pov, orbit=True,
                         assemble=False, video_stream="off", supersample=k)
    assert r.supersample == k
    r.close()
    # the same frames one at a time: the video loop's lifecycle steps, still renders, read_final_u8
    s, _, n_r, n_phi = drivers.make_renderer(W, H, pov, fov, n_stars=600, tex_w=512, tex_h=256, frame_slots=1, math="hybrid",
                                             supersample=k)
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
    r = HipRenderer(64, 36, sky, tex, math="strict", supersample=2, **KW)
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
    for k in (3, 16):
        assert hip_lib.bhr_set_supersample(r._ctx, k) == _lib.BHR_ERR_INVALID
    r.render(cam, fov)                                              # and the context still renders
    r.close()
    with pytest.raises(ValueError):
        HipRenderer(64, 36, sky, tex, rows=(0, 16), supersample=2, **KW)
    big = HipRenderer(8192, 4096, sky, tex, frame_slots=1, **KW)   # 64 x 2^25 rays = 2^31
    with pytest.raises(ValueError):
        big.set_supersample(8)
    big.set_supersample(4)
    big.close()


def test_cli_matches_render_image(tmp_path, hip_lib):
    from PIL import Image
    from bhr_amd import drivers
    out = os.path.join(str(tmp_path), "cli.png")
    subprocess.run([sys.executable, os.path.join(ROOT, "render.py"), "-r", "sd", "--supersample", "2", "--math", "strict",
                    "--n_stars", "600", "-o", out], check=True, cwd=ROOT, timeout=600)
    img = drivers.render_image(640, 360, [6, 0, 0.5], 90, 0.1, n_stars=600, supersample=2, math="strict")
    ref = os.path.join(str(tmp_path), "api.png")
    drivers.save_image(img, ref)
    a = np.asarray(Image.open(out).convert("RGB"))
    b = np.asarray(Image.open(ref).convert("RGB"))
    assert a.shape == (360, 640, 3) and np.array_equal(a, b)
