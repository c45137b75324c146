"""Motion blur from the ray map (bhr_raymap_render_shutter; include/bhr.h states the frame): the BG and DISK layers are the
sequential f32 mean (tests/shutter_ref.py) of the layers its samples' single map frames store -- bhr_raymap_render_view of a turned
camera, bhr_raymap_render of the build pose -- and the post-pass is bhr_bloom's on the resolved layers.  Two routes give those
bits: one fused launch (a map without overflow pixels, option "raymap_shutter_fused" not 0) and, sample by sample, the existing
shade, fix and accumulation launches.  Every comparison here is for zero differing pixels.

Views and scenes are those of test_gpu_orbit_map.py -- "ring" 96 x 54 (the hole's image, rays with two crossings), "odd" 21 x 13
(partial tiles on both sides), "aa" 24 x 15 anti-aliased (records with differentials) -- plus the still view "tilt", 24 x 15,
anti-aliased over a disk tilted by 25 degrees."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from shutter_ref import resolve

pytestmark = pytest.mark.gpu

POV, FOV, N_ORBIT, S, SPEED = (6.0, 0.0, 0.5), 90.0, 512, 0.5, 0.1
VIEWS = {
    "ring": dict(W=96, H=54, pov=POV, fov=FOV, kw=()),
    "odd": dict(W=21, H=13, pov=POV, fov=FOV, kw=()),
    "aa": dict(W=24, H=15, pov=POV, fov=FOV, kw=(("anti_alias", "lod_radius"), ("disk_tilt", 0.0))),
    "tilt": dict(W=24, H=15, pov=(5.0, 2.0, 1.0), fov=80.0, kw=(("anti_alias", "lod_radius"), ("disk_tilt", 25.0))),
}
LAYERS = ("final", "bg", "disk", "blur")


def _cam(k, pov=POV):
    from bhr_amd.camera import orbit_position
    return [float(v) for v in orbit_position(list(pov), k, N_ORBIT)]


def _mk(view, math="strict", **kw):
    from bhr_amd import HipRenderer, scenes
    v = VIEWS[view]
    return HipRenderer(v["W"], v["H"], scenes.analytic_skybox(), scenes.noisy_disk(), math=math, **dict(v["kw"]), **kw)


def _read(r, names=LAYERS, u8=True):
    from bhr_amd import _lib
    ids = dict(final=_lib.LAYER_FINAL, bg=_lib.LAYER_BG, disk=_lib.LAYER_DISK, blur=_lib.LAYER_BLUR, hdr=_lib.LAYER_HDR)
    out = {k: r.read_layer(ids[k]) for k in names}
    if u8:
        out["u8"] = r.read_final_u8()
    return out


def _assert_equal(got, want, tag, names=LAYERS + ("u8",)):
    for k in names:
        bad = int((got[k] != want[k]).any(axis=-1).sum())
        assert bad == 0, f"{tag} {k}: {bad} pixels differ (max |d| {np.abs(got[k].astype(np.float64) - want[k]).max():.3g})"


def _orbit_samples(f, n):
    """What render_video's shutter loop hands a frame f of the 512-frame orbit: positions and t_offsets of its n samples."""
    from bhr_amd import drivers
    u = drivers.shutter_times(f, S, n)
    return [_cam(t) for t in u], [(t - f) * SPEED for t in u]


def _bloom_of(r, layers, lens_flare=False):
    """bhr_bloom of the given BG and DISK in context r: FINAL, BLUR, u8 (and the layers back)."""
    from bhr_amd import _lib
    r.write_layer(_lib.LAYER_BG, layers["bg"])
    r.write_layer(_lib.LAYER_DISK, layers["disk"])
    r.bloom_only()
    if lens_flare:
        r.apply_lens_flare()
    return _read(r)


@functools.lru_cache(maxsize=None)
def _orbit_reference(view, f, n, slots=None):
    """The n single map frames of an orbit exposure, rendered one by one on ONE context, resolved on the host; and the sum of
    their overflow re-marches' steps."""
    r = _mk(view, **({} if slots is None else {"options": {"raymap_slots": slots}}))
    r.build_ray_map(_cam(0), FOV)
    pos, toff = _orbit_samples(f, n)
    singles, steps = [], 0
    for p, t in zip(pos, toff):
        r.render_from_ray_map_async(t_offset=t, cam_pos=p, fov=FOV, skip_bloom=True)
        singles.append(_read(r, ("bg", "disk"), u8=False))
        steps += r.counters()["ray_steps"]
    r.close()
    out = {k: resolve([s[k] for s in singles]) for k in ("bg", "disk")}
    for a in out.values():
        a.setflags(write=False)
    out["steps"] = steps
    out["differ"] = n > 1 and bool((singles[0]["bg"] != singles[-1]["bg"]).any() and (singles[0]["disk"] != singles[-1]["disk"]).any())
    return out


def _composition(view, n, fused, frames=(0, 5), slots=None):
    v = VIEWS[view]
    opts = {"raymap_shutter_fused": fused}
    if slots is not None:
        opts["raymap_slots"] = slots
    r = _mk(view, options=opts)
    r.build_ray_map(_cam(0), FOV)
    info = r.ray_map_info()
    for f in frames:
        tag = f"{view} n={n} f={f} fused={fused}"
        want = _orbit_reference(view, f, n, slots)
        pos, toff = _orbit_samples(f, n)
        if f == 0 and n == 3:
            assert pos[1] == _cam(0) and toff[1] == 0.0            # a sample exactly at the build camera, inside a ROT launch
        timed = r.counters()["frames_timed"]
        r.render_shutter_from_ray_map_async(toff, pos, FOV, skip_bloom=True)
        got = _read(r, ("bg", "disk"), u8=False)
        c = r.counters()
        _assert_equal(got, want, tag, ("bg", "disk"))
        assert want["differ"] == (n > 1)                          # the samples really differ: the test can fail
        assert c["rays"] == n * v["W"] * v["H"] and c["frames_timed"] == timed + 1        # one entry in the timing ring
        assert c["ray_steps"] == want["steps"], tag
        assert (c["ray_steps"] > 0) == (info["overflow_pixels"] > 0)
        assert c["march_ms"] > 0 and c["frame_ms"] >= c["march_ms"]
        # with bloom: the post-pass is bhr_bloom of the resolved layers
        r.render_shutter_from_ray_map_async(toff, pos, FOV)
        full = _read(r)
        _assert_equal(full, want, tag + " bloom", ("bg", "disk"))
        _assert_equal(full, _bloom_of(r, want), tag + " bloom")
        assert full["blur"].max() > 0.0 and (full["disk"] > 0).any() and (full["bg"] > 0).any()
    r.close()
    return info


# ---- 1. composition, orbit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("view", ["ring", "odd", "aa"])
def test_orbit_exposure_is_the_mean_of_its_map_frames(view, n, fused, hip_lib):
    info = _composition(view, n, fused)
    assert info["overflow_pixels"] == 0 and info["diff"] == (1 if view == "aa" else 0)


@pytest.mark.parametrize("fused", [1, 0])
def test_sixty_four_samples(fused, hip_lib):
    _composition("odd", 64, fused, frames=(5,))


# ---- 2. overflow ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("n", [1, 3])
def test_map_with_overflow_pixels_takes_the_unfused_route(n, fused, hip_lib):
    info = _composition("ring", n, fused, slots=1)
    assert info["overflow_pixels"] > 0 and info["slots"] == 1


def test_overflow_steps_of_a_still_exposure_are_n_times_one_map_frames(hip_lib):
    n = 4
    r = _mk("ring", options={"raymap_slots": 1})
    r.build_ray_map(_cam(0), FOV)
    assert r.ray_map_info()["overflow_pixels"] > 0
    r.render_from_ray_map_async(t_offset=0.3, skip_bloom=True)
    one = r.counters()["ray_steps"]
    r.render_shutter_from_ray_map_async([0.3 + 0.1 * j for j in range(n)], skip_bloom=True)
    c = r.counters()
    r.close()
    assert one > 0 and c["ray_steps"] == n * one and c["rays"] == n * 96 * 54


@pytest.mark.parametrize("slots,fused,launches", [(None, 1, 0), (None, 0, 3), (1, 1, 3), (1, 0, 3)])
def test_which_route_ran(slots, fused, launches, hip_lib):
    """The two routes give the same bits, so the frames cannot tell which one ran.  The accumulation launches can: under option
    "shutter_timing" every one of them is bracketed and counted, the sample-by-sample route has n of them and the fused launch
    none.  A map without overflow pixels takes the fused launch unless the option says 0; a map with overflow pixels never."""
    n = 3
    opts = {"raymap_shutter_fused": fused, "shutter_timing": 1}
    if slots is not None:
        opts["raymap_slots"] = slots
    r = _mk("ring", options=opts)
    r.build_ray_map(_cam(0), FOV)
    assert (r.ray_map_info()["overflow_pixels"] > 0) == (slots == 1)
    pos, toff = _orbit_samples(5, n)
    r.render_shutter_async(pos, FOV, toff, math="strict")       # a marched shutter frame first: its count must not linger
    assert r.shutter_timing()["launches"] == n
    r.render_shutter_from_ray_map_async(toff, pos, FOV)
    assert r.shutter_timing()["launches"] == launches
    r.render_shutter_from_ray_map_async(toff[:1], pos[:1], FOV)    # one sample: the one map frame, nothing to accumulate
    assert r.shutter_timing()["launches"] == 0
    r.close()


def test_fused_route_is_the_default(hip_lib):
    n = 3
    r = _mk("ring", options={"shutter_timing": 1})
    r.build_ray_map(_cam(0), FOV)
    pos, toff = _orbit_samples(5, n)
    r.set_option("raymap_shutter_fused", 0)
    r.render_shutter_from_ray_map_async(toff, pos, FOV)
    assert r.shutter_timing()["launches"] == n
    r.close()
    r = _mk("ring", options={"shutter_timing": 1})            # a fresh context: the option as bhr_create leaves it
    r.build_ray_map(_cam(0), FOV)
    r.render_shutter_async(pos, FOV, toff, math="strict")
    assert r.shutter_timing()["launches"] == n
    r.render_shutter_from_ray_map_async(toff, pos, FOV)
    assert r.shutter_timing()["launches"] == 0
    r.close()


# ---- 3. still camera against the march ----------------------------------------------------------------------------------------
def _still_offsets(n):
    """t_j spread over a frame time, around a frame 5 steps in."""
    return [5 * SPEED + SPEED * ((j + 0.5) / n - 0.5) for j in range(n)]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("n", [2, 5])
@pytest.mark.parametrize("view", ["ring", "tilt"])
def test_still_exposure_is_the_marched_strict_shutter_frame(view, n, fused, hip_lib):
    v = VIEWS[view]
    toff = _still_offsets(n)
    r = _mk(view, options={"raymap_shutter_fused": fused})
    r.build_ray_map(v["pov"], v["fov"])
    assert r.ray_map_info()["overflow_pixels"] == 0
    r.render_shutter_from_ray_map_async(toff)
    got = _read(r)
    r.render_shutter_async([list(v["pov"])] * n, v["fov"], toff, math="strict")
    want = _read(r)
    r.close()
    _assert_equal(got, want, f"{view} n={n} fused={fused}")
    assert (want["disk"] > 0).any() and (want["bg"] > 0).any() and want["blur"].max() > 0.0


@pytest.mark.parametrize("fused", [1, 0])
def test_still_exposure_with_lens_flare_and_under_a_grade(fused, hip_lib):
    view, n = "tilt", 5
    v = VIEWS[view]
    toff = _still_offsets(n)
    r = _mk(view, options={"raymap_shutter_fused": fused})
    r.build_ray_map(v["pov"], v["fov"])
    r.render_shutter_from_ray_map_async(toff, lens_flare=True)
    got = _read(r)
    r.render_shutter_async([list(v["pov"])] * n, v["fov"], toff, math="strict", lens_flare=True)
    want = _read(r)
    r.render_shutter_async([list(v["pov"])] * n, v["fov"], toff, math="strict", lens_flare=False)
    plain = _read(r)
    _assert_equal(got, want, f"flare fused={fused}")
    assert (want["final"] != plain["final"]).any()                # the flare is there
    r.set_grade("aces", exposure=1.0, transfer="srgb", keep_hdr=True)
    names = LAYERS + ("hdr",)
    r.render_shutter_from_ray_map_async(toff)
    got = _read(r, names)
    r.render_shutter_async([list(v["pov"])] * n, v["fov"], toff, math="strict")
    want = _read(r, names)
    r.close()
    _assert_equal(got, want, f"graded fused={fused}", names + ("u8",))
    assert (want["final"] != plain["final"]).any()                # ... and so is the grade


# ---- 4. not ignoring its arguments --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_samples_times_and_cameras_reach_the_frame(fused, hip_lib):
    n = 4
    r = _mk("ring", options={"raymap_shutter_fused": fused})
    r.build_ray_map(_cam(0), FOV)
    pos, toff = _orbit_samples(40, n)
    r.render_shutter_from_ray_map_async([toff[0]] * n, skip_bloom=True)
    same_t = _read(r, ("bg", "disk"), u8=False)
    r.render_shutter_from_ray_map_async([10 * t for t in toff], skip_bloom=True)
    spread_t = _read(r, ("bg", "disk"), u8=False)
    r.render_shutter_from_ray_map_async([toff[0]] * n, pos, FOV, skip_bloom=True)
    turned = _read(r, ("bg", "disk"), u8=False)
    r.close()
    assert (same_t["disk"] != spread_t["disk"]).any()            # the t_offsets are not ignored
    assert (turned["disk"] != same_t["disk"]).any() and (turned["bg"] != same_t["bg"]).any()      # nor are the cameras


# ---- 5. a hybrid context --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_hybrid_context_gets_the_strict_layers_and_its_own_post_pass(fused, hip_lib):
    view, n, f = "ring", 3, 5
    want = _orbit_reference(view, f, n)
    pos, toff = _orbit_samples(f, n)
    r = _mk(view, math="hybrid", options={"raymap_shutter_fused": fused})
    r.build_ray_map(_cam(0), FOV)
    r.render_shutter_from_ray_map_async(toff, pos, FOV)
    got = _read(r)
    buf = np.empty(16, dtype=np.uint8)                           # the frame went through the split-f16 post-pass: its operands exist
    assert hip_lib.bhr_debug_read(r._ctx, 0, buf.ctypes.data, buf.nbytes, None) == 0, hip_lib.bhr_last_error()
    _assert_equal(got, want, f"hybrid fused={fused}", ("bg", "disk"))
    _assert_equal(got, _bloom_of(r, want), f"hybrid fused={fused} post-pass")
    r.close()
    assert got["blur"].max() > 0.0


# ---- 6. two frame slots ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_frames_on_two_slots_equal_one_slot(fused, hip_lib):
    """Four shutter-map frames in a row, alternating with plain map frames: every frame of the two-slot context equals the same
    frame of a fresh one-slot context -- no shared or stale sums."""
    view = "ring"

    def sequence(slots):
        r = _mk(view, math="hybrid", frame_slots=slots, options={"raymap_shutter_fused": fused})
        assert r.frame_slots == slots
        r.build_ray_map(_cam(0), FOV)
        frames = []
        for k, n in enumerate((5, 2, 8, 3)):
            pos, toff = _orbit_samples(10 * k + 3, n)
            r.render_shutter_from_ray_map_async(toff, pos, FOV)
            frames.append(_read(r))
            r.render_from_ray_map_async(frame=k, cam_pos=_cam(7 * k), fov=FOV)
            frames.append(_read(r))
        r.close()
        return frames

    one, two = sequence(1), sequence(2)
    for k, (g, w) in enumerate(zip(two, one)):
        _assert_equal(g, w, f"frame {k} fused={fused}")
    assert (two[0]["final"] != two[2]["final"]).any() and (two[0]["final"] != two[1]["final"]).any()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_context_usable(hip_lib):
    from bhr_amd import HipRenderer, _lib, scenes
    lib = hip_lib
    view, n = "odd", 5
    r = _mk(view)
    pos, toff = _orbit_samples(5, n)

    def cams_of(renderer, positions, offsets, fov=FOV, count=None):
        cams = (_lib.Camera * (count or len(positions)))()
        for j, (p, t) in enumerate(zip(positions, offsets)):
            cams[j] = renderer.camera_uniforms(p, fov, t_offset=t)
        return cams

    good = cams_of(r, pos, toff)

    def refused(ctx, cams, count, flags, code, word=None):
        rc = lib.bhr_raymap_render_shutter(ctx, cams, count, flags)
        assert rc == code, (rc, lib.bhr_last_error())
        assert b"bhr_raymap_render_shutter" in lib.bhr_last_error()
        if word is not None:
            assert word in lib.bhr_last_error(), lib.bhr_last_error()

    refused(r._ctx, good, n, 0, _lib.BHR_ERR_STATE, b"no ray map")       # before a build
    r.build_ray_map(_cam(0), FOV)
    r.render_from_ray_map_async(frame=5)
    want = _read(r)

    def still_renders(ctx_r=r, ref=want):
        before = ctx_r.counters()["frames_timed"]
        ctx_r.render_from_ray_map_async(frame=5)
        _assert_equal(_read(ctx_r), ref, "after a refusal")
        return before

    frames = still_renders()
    big = cams_of(r, [pos[j % n] for j in range(65)], [0.01 * j for j in range(65)])
    refused(r._ctx, big, 0, 0, _lib.BHR_ERR_INVALID, b"samples")
    refused(r._ctx, big, 65, 0, _lib.BHR_ERR_INVALID, b"samples")
    refused(r._ctx, big, -1, 0, _lib.BHR_ERR_INVALID, b"samples")
    for flags in (_lib.SKIP_DIFFERENTIALS, _lib.PERSISTENT, _lib.FORCE_FAST, _lib.ROW_COSTS):
        refused(r._ctx, good, n, flags, _lib.BHR_ERR_INVALID, b"flags")
    refused(r._ctx, None, n, 0, _lib.BHR_ERR_INVALID)
    refused(None, good, n, 0, _lib.BHR_ERR_INVALID)
    nan = cams_of(r, pos, toff)
    nan[3].t_offset = float("nan")
    refused(r._ctx, nan, n, 0, _lib.BHR_ERR_INVALID, b"sample 3: t_offset")
    high = cams_of(r, pos[:2] + [_cam(5, pov=(6.0, 0.0, 0.6))] + pos[3:], toff)            # sample 2 at another height
    refused(r._ctx, high, n, 0, _lib.BHR_ERR_INVALID, b"sample 2")
    assert b"height" in lib.bhr_last_error()
    assert r.counters()["frames_timed"] == frames + 1          # nothing but still_renders' frame was launched
    still_renders()
    with pytest.raises(ValueError):                            # the Python surface maps the codes as everywhere else
        r.render_shutter_from_ray_map_async(toff, pos[:2] + [_cam(5, pov=(6.0, 0.0, 0.6))] + pos[3:], FOV)
    with pytest.raises(ValueError):
        r.render_shutter_from_ray_map_async(toff, pos[:2], FOV)               # mismatched lengths
    with pytest.raises(ValueError):
        r.render_shutter_from_ray_map_async(toff, pos)                         # positions without fov
    with pytest.raises(ValueError):
        r.render_shutter_from_ray_map_async([])                                # no sample
    # supersampling and adaptive supersampling: the map stays and renders again once the setting is back
    for sampling in ((2, None), (2, 0.1)):
        r.set_supersample(*sampling)
        refused(r._ctx, good, n, 0, _lib.BHR_ERR_STATE, b"supersampling")
        r.set_supersample(1)
        still_renders()
    r.free_ray_map()
    refused(r._ctx, good, n, 0, _lib.BHR_ERR_STATE, b"no ray map")
    r.build_ray_map(_cam(0), FOV)
    still_renders()
    r.close()
    # a tilted disk: the still camera is served, a turned one refused
    v = VIEWS["tilt"]
    t = _mk("tilt")
    t.build_ray_map(v["pov"], v["fov"])
    t.render_from_ray_map_async(frame=5)
    tilted = _read(t)
    before = t.counters()["frames_timed"]
    turned = cams_of(t, [list(v["pov"]), _cam(3, pov=v["pov"])], [0.1, 0.2], fov=v["fov"])
    refused(t._ctx, turned, 2, 0, _lib.BHR_ERR_INVALID, b"sample 1")
    assert b"tilted" in lib.bhr_last_error()
    assert t.counters()["frames_timed"] == before
    still_renders(t, tilted)
    t.render_shutter_from_ray_map_async([0.1, 0.2])             # ... and the still exposure on the same context works
    assert np.isfinite(_read(t)["final"]).all()
    t.close()
    # a row-block context
    block = HipRenderer(21, 13, scenes.analytic_skybox(), scenes.noisy_disk(), rows=(8, 13))
    refused(block._ctx, good, n, 0, _lib.BHR_ERR_INVALID, b"whole-frame")
    block.close()


# ---- 8. driver ------------------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_still_video_is_the_marched_shutter_video(tmp_path, capsys, hip_lib):
    from bhr_amd import drivers
    W, H, N, NS = 48, 27, 3, 4
    cam0, fov = [6, 0, 0.5], 90

    def video(out, **kw):
        r, _, _, _ = drivers.make_renderer(W, H, cam0, fov, n_stars=50, tex_w=256, tex_h=128, math="strict")
        try:
            drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=out, fov=fov, static_cam_pos=cam0, orbit=False,
                                 disk_rotation_speed=SPEED, video_stream="off", assemble=False, shutter=S, shutter_samples=NS, **kw)
            assert r.ray_map_info()["built"] == 0            # the map, if any, is freed at the end
        finally:
            r.close()
        return drivers._frames_dir(out)

    d0 = video(str(tmp_path / "march" / "v.mp4"))
    d1 = video(str(tmp_path / "map" / "v.mp4"), shutter_map=True)
    names = [f"frame_{f:04d}.png" for f in range(N)]
    assert sorted(os.listdir(d0)) == sorted(os.listdir(d1)) == names + ["progress.json"]
    p0, p1 = (json.load(open(os.path.join(d, "progress.json")))["params"] for d in (d0, d1))
    assert "shutter_map" not in p0 and p1 == dict(p0, shutter_map=True)
    for name in names:
        assert open(os.path.join(d0, name), "rb").read() == open(os.path.join(d1, name), "rb").read(), name
    assert (_png(os.path.join(d1, names[0])) != _png(os.path.join(d1, names[-1]))).any()
    # a resume under the other setting starts over
    capsys.readouterr()
    assert video(str(tmp_path / "map" / "v.mp4"), resume=True) == d1
    assert "starting over" in capsys.readouterr().out
    assert "shutter_map" not in json.load(open(os.path.join(d1, "progress.json")))["params"]
    with pytest.raises(ValueError, match="shutter_map"):
        video(str(tmp_path / "both" / "v.mp4"), shutter_map=True, ray_map=True)
    assert not os.path.exists(drivers._frames_dir(str(tmp_path / "both" / "v.mp4")))


def test_orbit_video_is_the_composition_of_map_frames(tmp_path, hip_lib):
    """render_video(orbit=True, shutter_map=True): every frame file is the u8 frame of the composition of test 1 -- the single
    map frames of shutter_times' cameras, resolved on the host, bhr_bloom of the result -- on a context driven through the same
    lifecycle steps."""
    from bhr_amd import _lib, drivers
    from bhr_amd.camera import orbit_position
    W, H, N, NS = 48, 27, 3, 4
    cam0, fov, deg = [6, 0, 0.5], 90, 90.0
    out = str(tmp_path / "orbit" / "v.mp4")
    r, _, _, _ = drivers.make_renderer(W, H, cam0, fov, n_stars=50, tex_w=256, tex_h=128, math="strict")
    drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=out, fov=fov, static_cam_pos=cam0, orbit=True, orbit_degrees=deg,
                         disk_rotation_speed=SPEED, video_stream="off", assemble=False, shutter=S, shutter_samples=NS, shutter_map=True)
    r.close()
    d = drivers._frames_dir(out)

    r, _, _, _ = drivers.make_renderer(W, H, cam0, fov, n_stars=50, tex_w=256, tex_h=128, math="strict")
    r.set_outputs("u8")
    factories = drivers.init_lifecycle_system(r, r.dtex_h, r.dtex_w, seed=42)
    r.build_ray_map(orbit_position(cam0, 0, N, deg), fov)
    frames = []
    for f in range(N):
        drivers.advance_lifecycle_frame(r, factories, f * SPEED, SPEED, recompute_stats=(f % 60 == 0), compose=True)
        singles = []
        for u in drivers.shutter_times(f, S, NS):
            r.render_from_ray_map_async(t_offset=(u - f) * SPEED, cam_pos=orbit_position(cam0, u, N, deg), fov=fov, skip_bloom=True)
            singles.append(_read(r, ("bg", "disk"), u8=False))
        r.write_layer(_lib.LAYER_BG, resolve([s["bg"] for s in singles]))
        r.write_layer(_lib.LAYER_DISK, resolve([s["disk"] for s in singles]))
        r.bloom_only()
        frames.append(r.read_final_u8())
    r.close()
    for f in range(N):
        np.testing.assert_array_equal(_png(os.path.join(d, f"frame_{f:04d}.png")), frames[f], err_msg=f"frame {f}")
    assert (frames[0] != frames[N - 1]).any()
