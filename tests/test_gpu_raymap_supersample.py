"""Supersampled ray maps on the device (option "raymap_supersample", HipRenderer.build_ray_map(supersample=k); include/bhr.h
states the contract): the map of the fine frame, k x k records per pixel, resolved in the shade.  Every comparison is exact.

The yardsticks are never the code under test:
  (A) the marched strict frame of a fresh context with set_supersample(k) -- the marched supersampled kernels;
  (B) tests/supersample_ref.box_resolve of the skip-bloom BG / DISK of a k = 1 map frame from a context of k W x k H pixels
      -- the k = 1 map kernels and the NumPy statement of the filter.
Maps are built under scene "a" and rendered under scene "b", and the tests assert that the swap changed the picture.

Frames: 21 x 13 (fine 42 x 26 and 84 x 52: partial fine tiles on both sides), 5 x 3 at k = 8 (one output pixel per tile, the whole
butterfly), 24 x 15 tilted and anti-aliased (records with differentials), 24 x 15 untilted and anti-aliased (turned), 96 x 54
(the hole's image; rays with several crossings: overflow groups)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from shutter_ref import resolve
from supersample_ref import box_resolve

pytestmark = pytest.mark.gpu

CAM, FOV = (6.0, 0.0, 0.5), 90.0
VIEWS = {
    "odd": dict(W=21, H=13, cam=CAM, fov=FOV, kw=()),
    "tiny": dict(W=5, H=3, cam=CAM, fov=FOV, kw=()),
    "tilt": dict(W=24, H=15, cam=(5.0, 2.0, 1.0), fov=80.0, kw=(("anti_alias", "lod_radius"), ("disk_tilt", 20.0))),
    "aa": dict(W=24, H=15, cam=CAM, fov=FOV, kw=(("anti_alias", "lod_radius"), ("disk_tilt", 0.0))),
    "ring": dict(W=96, H=54, cam=CAM, fov=FOV, kw=()),
}
LAYERS = ("final", "bg", "disk", "blur")
TS = (0.0, 0.3, 7.5)
N_ORBIT = 24


@functools.lru_cache(maxsize=None)
def _scene(which):
    from bhr_amd import scenes
    return (scenes.analytic_skybox(), scenes.noisy_disk(seed=7)) if which == "a" else (scenes.star_skybox(), scenes.noisy_disk(seed=11))


def _mk(view, scene="a", scale=1, math_mode="strict", **kw):
    """A context of the view's frame (scale = k: of its fine frame, k W x k H pixels)."""
    from bhr_amd import HipRenderer
    v = VIEWS[view]
    sky, tex = _scene(scene)
    return HipRenderer(v["W"] * scale, v["H"] * scale, sky, tex, math=math_mode, **dict(v["kw"]), **kw)


def _set_scene(r, which):
    from bhr_amd import _lib
    sky, tex = _scene(which)
    _lib.check(r._lib.bhr_set_skybox(r._ctx, _lib.fptr(sky), sky.shape[0], sky.shape[1]))
    r.update_disk_texture(tex)


def _orbit_cam(view, f):
    from bhr_amd.camera import orbit_position
    return tuple(float(x) for x in orbit_position(list(VIEWS[view]["cam"]), f, N_ORBIT))


def _read(r, names=LAYERS, u8=True):
    from bhr_amd import _lib
    ids = dict(final=_lib.LAYER_FINAL, bg=_lib.LAYER_BG, disk=_lib.LAYER_DISK, blur=_lib.LAYER_BLUR)
    out = {k: r.read_layer(ids[k]) for k in names}
    if u8:
        out["u8"] = r.read_final_u8()
    return out


def _frozen(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _assert_equal(got, want, tag, names=LAYERS + ("u8",)):
    for k in names:
        bad = int((got[k] != want[k]).any(axis=-1).sum())
        assert bad == 0, f"{tag} {k}: {bad} pixels differ (max |d| {np.abs(got[k].astype(np.float64) - want[k]).max():.3g})"


@functools.lru_cache(maxsize=None)
def _marched(view, k, scene, t, flags=0, cam=None, math_mode="strict", force_strict=True):
    """(A): bhr_render of the view on a fresh context with set_supersample(k).  Computed once, shared, never modified."""
    from bhr_amd import _lib
    v = VIEWS[view]
    r = _mk(view, scene, math_mode=math_mode)
    r.set_supersample(k)
    uniforms = r.camera_uniforms(list(cam or v["cam"]), v["fov"], t_offset=t)
    _lib.check(r._lib.bhr_render(r._ctx, C.byref(uniforms), flags | (_lib.FORCE_STRICT if force_strict else 0)))
    out = _read(r)
    out["c"] = r.counters()
    r.close()
    return _frozen(out)


@functools.lru_cache(maxsize=None)
def _fine_map_frame(view, k, scene, t, skip_differentials=False, cam=None, build_cam=None):
    """(B): the k = 1 map of a context of k W x k H pixels (its pixel pitch is the fine camera's bit for bit), built at the
    view's camera (or `build_cam`), rendered skip-bloom -- turned to `cam` if given -- and box-filtered on the host."""
    v = VIEWS[view]
    r = _mk(view, scene, scale=k)
    r.build_ray_map(list(build_cam or v["cam"]), v["fov"], skip_differentials=skip_differentials)
    assert r.ray_map_info()["supersample"] == 1
    if cam is None:
        r.render_from_ray_map_async(t_offset=t, skip_bloom=True)
    else:
        r.render_from_ray_map_async(t_offset=t, skip_bloom=True, cam_pos=list(cam), fov=v["fov"])
    fine = _read(r, ("bg", "disk"), u8=False)
    r.close()
    return _frozen({name: box_resolve(fine[name], k) for name in ("bg", "disk")})


# ---- 1. a still camera -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view,k,skip", [("odd", 2, False), ("odd", 4, False), ("tiny", 8, False), ("tilt", 2, False), ("tilt", 2, True)])
def test_map_frame_is_the_marched_supersampled_strict_frame(view, k, skip, hip_lib):
    from bhr_amd import _lib
    v = VIEWS[view]
    flags = _lib.SKIP_DIFFERENTIALS if skip else 0
    r = _mk(view, "a")
    r.build_ray_map(list(v["cam"]), v["fov"], skip_differentials=skip, supersample=k)
    info = r.ray_map_info()
    assert (info["supersample"], info["width"], info["rows"], info["diff"]) == (k, v["W"], v["H"], 1 if view == "tilt" and not skip else 0)
    assert info["ray_steps"] == _marched(view, k, "a", 0.0, flags)["c"]["ray_steps"]      # the build is the strict supersampled march
    _set_scene(r, "b")                                   # between build and render: the map does not hold the scene
    for t in TS:
        tag = f"{view} k={k} t={t}"
        r.render_from_ray_map_async(t_offset=t)
        got = _read(r)
        assert r.counters()["rays"] == k * k * v["W"] * v["H"]
        _assert_equal(got, _marched(view, k, "b", t, flags), tag + " (A)")
        _assert_equal(got, _fine_map_frame(view, k, "b", t, skip), tag + " (B)", ("bg", "disk"))
        one = _marched(view, 1, "b", t, flags)
        assert (got["bg"] != one["bg"]).any() and (got["disk"] != one["disk"]).any(), "the k = 1 frame: the test cannot fail"
        old = _marched(view, k, "a", t, flags)
        assert (got["bg"] != old["bg"]).any() and (got["disk"] != old["disk"]).any(), "the scene swap changed nothing"
    if view == "tilt" and skip:                          # anti-aliased: the differentials change the picture
        assert (_marched(view, k, "b", 0.3, flags)["disk"] != _marched(view, k, "b", 0.3)["disk"]).any()
    r.close()


# ---- 2. overflow groups ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ring_map(slots, k=2):
    v = VIEWS["ring"]
    r = _mk("ring", "a", options={"raymap_slots": slots})
    r.build_ray_map(list(v["cam"]), v["fov"], supersample=k)
    out = dict(info=r.ray_map_info(), passes=r.ray_map_passes())
    _set_scene(r, "b")
    r.render_from_ray_map_async(t_offset=0.3)
    out["frame"] = _read(r)
    out["c"] = r.counters()
    r.close()
    return out


def _groups(plane, k):
    """(k H, k W) -> (H, W, k k): the sub-samples of every output pixel."""
    h, w = plane.shape[0] // k, plane.shape[1] // k
    return plane.reshape(h, k, w, k).transpose(0, 2, 1, 3).reshape(h, w, k * k)


@pytest.mark.parametrize("slots", [1, 4, 8])
def test_overflow_groups_are_remarched_whole(slots, hip_lib):
    k, W, H = 2, 96, 54
    m = _ring_map(slots)
    _assert_equal(m["frame"], _marched("ring", k, "b", 0.3), f"K={slots}")
    p, info = m["passes"], m["info"]
    assert p["crossings"].shape == (k * H, k * W) and p["hits"].shape == (slots, k * H, k * W, 5)
    over = _groups(p["crossings"], k) > slots                         # (H, W, k k): the rays over the slots
    listed = over.any(axis=-1)                                        # ... and the groups that hold one: listed whole
    assert info["overflow_pixels"] == int(listed.sum()) * k * k
    assert info["crossings_stored"] == int(np.minimum(p["crossings"], slots).sum())
    # the frame's counters: the steps of the re-march of every ray of every listed group
    assert m["c"]["ray_steps"] == int(_groups(p["steps"], k)[listed].sum())
    assert m["c"]["rays"] == k * k * W * H and m["c"]["frames_timed"] == 1
    if slots == 1:
        assert info["overflow_pixels"] > 0 and info["overflow_pixels"] % (k * k) == 0
        mixed = listed & ~over.all(axis=-1)                           # a ray with CROSSINGS <= K beside one with CROSSINGS > K
        print(f"K=1: {int(listed.sum())} listed groups, {int(mixed.sum())} of them mixed")
        assert mixed.any(), "no mixed group: the group-wise OR is not exercised"
    if slots == 8:
        assert info["overflow_pixels"] < _ring_map(1)["info"]["overflow_pixels"]
    _assert_equal(m["frame"], _ring_map(1)["frame"], f"K={slots} against K=1")


# ---- 3. turned about z ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view,k", [("odd", 2), ("aa", 4)])
def test_turned_map_frames(view, k, hip_lib):
    v = VIEWS[view]
    t = 0.5
    r = _mk(view, "a")
    cam0 = _orbit_cam(view, 0)                           # the orbit's radius is |pov|: frame 0 is not the pov itself
    r.build_ray_map(list(cam0), v["fov"], supersample=k)
    assert r.ray_map_info()["diff"] == (1 if view == "aa" else 0)
    _set_scene(r, "b")
    frames = {}
    for f in (0, 1, 17):
        cam = _orbit_cam(view, f)
        r.render_from_ray_map_async(t_offset=t, cam_pos=list(cam), fov=v["fov"], skip_bloom=True)
        frames[f] = _read(r, ("bg", "disk"), u8=False)
        assert r.counters()["rays"] == k * k * v["W"] * v["H"]
        _assert_equal(frames[f], _fine_map_frame(view, k, "b", t, cam=cam, build_cam=cam0), f"{view} k={k} orbit frame {f} (B)", ("bg", "disk"))
    for f in (1, 17):
        assert (frames[f]["bg"] != frames[0]["bg"]).any() and (frames[f]["disk"] != frames[0]["disk"]).any(), "the turn changed nothing"
    # at the build camera: the still map frame, which is the marched supersampled frame, in every layer
    r.render_from_ray_map_async(t_offset=t, cam_pos=list(cam0), fov=v["fov"])
    got = _read(r)
    r.render_from_ray_map_async(t_offset=t)
    still = _read(r)
    r.close()
    _assert_equal(got, still, f"{view} k={k} angle 0 against the still frame")
    _assert_equal(got, _marched(view, k, "b", t, cam=cam0), f"{view} k={k} angle 0 (A)")


# ---- 4. shutter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("view,orbit", [("tilt", False), ("odd", True)])
def test_shutter_frames_resolve_each_sample_then_take_the_mean(view, orbit, n, fused, hip_lib):
    v, k = VIEWS[view], 2
    r = _mk(view, "a", options={"raymap_shutter_fused": fused})
    cam0 = _orbit_cam(view, 0) if orbit else v["cam"]
    r.build_ray_map(list(cam0), v["fov"], supersample=k)
    _set_scene(r, "b")
    offsets = [0.3 + 0.07 * j for j in range(n)]
    positions = [list(_orbit_cam(view, 0.25 * j)) for j in range(n)] if orbit else None
    singles = []
    for j in range(n):
        if orbit:
            r.render_from_ray_map_async(t_offset=offsets[j], cam_pos=positions[j], fov=v["fov"], skip_bloom=True)
        else:
            r.render_from_ray_map_async(t_offset=offsets[j], skip_bloom=True)
        singles.append(_read(r, ("bg", "disk"), u8=False))
    # the first sample is the build's view: the marched supersampled frame (tests 1 and 3 hold the others)
    _assert_equal(singles[0], _marched(view, k, "b", offsets[0], cam=cam0), f"{view} sample 0 (A)", ("bg", "disk"))
    want = {name: resolve([s[name] for s in singles]) for name in ("bg", "disk")}
    r.render_shutter_from_ray_map_async(offsets, positions, v["fov"], skip_bloom=True)
    got = _read(r, ("bg", "disk"), u8=False)
    c = r.counters()
    r.close()
    _assert_equal(got, want, f"{view} n={n} fused={fused}", ("bg", "disk"))
    assert c["rays"] == n * k * k * v["W"] * v["H"]
    if n > 1:
        assert (singles[0]["disk"] != singles[-1]["disk"]).any() and (got["disk"] != singles[0]["disk"]).any()


# ---- 5. the context is left as it was --------------------------------------------------------------------------------------------
def test_a_supersampled_build_leaves_the_contexts_own_frames_alone(hip_lib):
    view, k = "ring", 2
    v = VIEWS[view]
    cam, fov = list(v["cam"]), v["fov"]
    other = [3.2, 0.5, 0.12]

    def hybrid_frame(r, pos, f):
        r.render_async(pos, f)
        return _read(r)

    fresh = _mk(view, "a", math_mode="hybrid", frame_slots=2)
    want_own, want_other = hybrid_frame(fresh, cam, fov), hybrid_frame(fresh, other, 100.0)
    fresh.close()
    r = _mk(view, "a", math_mode="hybrid", frame_slots=2)
    assert r.frame_slots == 2
    first = hybrid_frame(r, cam, fov)                    # builds the tile order, the hybrid lists and the fix lists of the k = 1 frame
    r.build_ray_map(cam, fov, supersample=k)
    again = hybrid_frame(r, cam, fov)
    _assert_equal(again, first, "the same bhr_render frame behind a k = 2 build")
    _assert_equal(again, want_own, "... against a fresh context")
    assert (want_own["final"] != want_other["final"]).any()
    # map frames and marched frames over both slots
    for step, (what, arg) in enumerate([("map", 0.0), ("march", cam), ("map", 7.5), ("march", other), ("march", cam), ("map", 0.0), ("map", 0.3)]):
        if what == "map":
            r.render_from_ray_map_async(t_offset=arg)
            _assert_equal(_read(r), _marched(view, k, "a", arg), f"step {step}: map frame t={arg}")
        else:
            got = hybrid_frame(r, arg, fov if arg is cam else 100.0)
            _assert_equal(got, want_own if arg is cam else want_other, f"step {step}: marched frame")
    assert (_marched(view, k, "a", 0.0)["final"] != _marched(view, k, "a", 7.5)["final"]).any()
    # back to one ray per pixel: the k = 1 map's contract holds again
    r.build_ray_map(cam, fov, supersample=1)
    assert r.ray_map_info()["supersample"] == 1 and r.ray_map_passes()["steps"].shape == (v["H"], v["W"])
    r.render_from_ray_map_async(t_offset=0.3)
    _assert_equal(_read(r), _marched(view, 1, "a", 0.3), "k = 1 again")
    _assert_equal(hybrid_frame(r, cam, fov), want_own, "the context's own frame at the end")
    r.close()


# ---- 6. refusals and bookkeeping ---------------------------------------------------------------------------------------------------
def test_refusals_and_bookkeeping(hip_lib):
    from bhr_amd import HipRenderer, _lib
    lib = hip_lib
    view, v, k = "odd", VIEWS["odd"], 2
    W, H = v["W"], v["H"]
    r = _mk(view, "a")
    cam = r.camera_uniforms(list(v["cam"]), v["fov"])
    frames0 = r.counters()["frames_timed"]
    # the option
    for bad in (3, 0, 16, -2, 2.5, 6):
        assert lib.bhr_set_option(r._ctx, b"raymap_supersample", float(bad)) == _lib.BHR_ERR_INVALID
        assert b"raymap_supersample" in lib.bhr_last_error()
    for bad in (3, 0, 16):
        with pytest.raises(ValueError):
            r.build_ray_map(list(v["cam"]), v["fov"], supersample=bad)
    assert r.ray_map_info()["built"] == 0 and r.ray_map_info()["device_bytes"] == 0
    # ... and from the environment of bhr_create: the build refuses
    saved = os.environ.get("BHR_RAYMAP_SUPERSAMPLE")
    os.environ["BHR_RAYMAP_SUPERSAMPLE"] = "3"
    try:
        env = _mk(view, "a")
    finally:
        if saved is None:
            os.environ.pop("BHR_RAYMAP_SUPERSAMPLE", None)
        else:
            os.environ["BHR_RAYMAP_SUPERSAMPLE"] = saved
    assert lib.bhr_raymap_build(env._ctx, C.byref(cam), 0) == _lib.BHR_ERR_INVALID and b"raymap_supersample" in lib.bhr_last_error()
    assert env.ray_map_info()["built"] == 0 and env.ray_map_info()["device_bytes"] == 0
    env.close()
    # the build, its planes and its bytes
    for slots, skip in ((4, False), (2, True)):
        r.set_option("raymap_slots", slots)
        r.build_ray_map(list(v["cam"]), v["fov"], skip_differentials=skip, supersample=k)
        info, p = r.ray_map_info(), r.ray_map_passes()
        assert (info["built"], info["supersample"], info["slots"], info["width"], info["rows"]) == (1, k, slots, W, H)
        assert p["steps"].shape == p["status"].shape == p["crossings"].shape == p["hit_r"].shape == (k * H, k * W)
        assert p["escape_dir"].shape == (k * H, k * W, 3) and p["hits"].shape == (slots, k * H, k * W, 5)
        assert int(p["steps"].sum()) == info["ray_steps"]
        # k^2 (24 + K 20 + 4) bytes per output pixel; beyond it only the list's round-up to 256 entries and the map's counters
        # (16 u32 of list count, 8 + 128 * 32 u64 of totals and step cells)
        planes = k * k * W * H * (24 + slots * 20 + 4)
        assert 0 <= info["device_bytes"] - planes <= 255 * 4 + 16 * 4 + (8 + 128 * 32) * 8
        buf = np.zeros((H, W), dtype=np.int32)                # the planes are fine-sized: the output frame's size is refused
        assert lib.bhr_raymap_read(r._ctx, _lib.RAYMAP_STEPS, buf.ctypes.data, buf.nbytes) == _lib.BHR_ERR_INVALID
    want = _marched(view, k, "a", 0.3, _lib.SKIP_DIFFERENTIALS)

    def still_renders():
        r.render_from_ray_map_async(t_offset=0.3)
        _assert_equal(_read(r), want, "after a refusal")

    still_renders()
    frames = r.counters()["frames_timed"]
    assert frames == frames0 + 1
    # the context's own supersampling stays refused, as for every map
    for sampling in ((2, None), (2, 0.1)):
        r.set_supersample(*sampling)
        assert lib.bhr_raymap_build(r._ctx, C.byref(cam), 0) == _lib.BHR_ERR_INVALID and b"one ray per pixel" in lib.bhr_last_error()
        assert lib.bhr_raymap_render(r._ctx, 0.0, 0) == _lib.BHR_ERR_STATE and b"one ray per pixel" in lib.bhr_last_error()
        assert lib.bhr_raymap_render_view(r._ctx, C.byref(cam), 0) == _lib.BHR_ERR_STATE
        assert lib.bhr_raymap_render_shutter(r._ctx, C.byref(cam), 1, 0) == _lib.BHR_ERR_STATE
        r.set_supersample(1)
    assert r.counters()["frames_timed"] == frames            # nothing was launched
    still_renders()
    # free, render
    r.free_ray_map()
    assert r.ray_map_info()["built"] == 0 and r.ray_map_info()["device_bytes"] == 0
    assert lib.bhr_raymap_render(r._ctx, 0.3, 0) == _lib.BHR_ERR_STATE
    with pytest.raises(AssertionError):
        r.ray_map_passes()
    r.close()
    # k^2 W H >= 2^31: refused by arithmetic, nothing allocated.  32768 x 1024 pixels: 8^2 of them are 2^31 rays, 4^2 are not
    # (that build is not attempted: it would be a 2 GB march)
    sky, tex = _scene("a")
    wide = HipRenderer(32768, 1024, sky, tex, math="strict")
    wcam = wide.camera_uniforms(list(v["cam"]), v["fov"])
    wide.set_option("raymap_supersample", 8)
    assert lib.bhr_raymap_build(wide._ctx, C.byref(wcam), 0) == _lib.BHR_ERR_INVALID and b"2^31" in lib.bhr_last_error()
    assert wide.ray_map_info()["built"] == 0 and wide.ray_map_info()["device_bytes"] == 0
    assert wide.counters()["frames_timed"] == 0
    wide.close()


# ---- 7. the video loop -------------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


@pytest.mark.parametrize("mode", ["ray_map", "orbit_map", "shutter_map"])
def test_video_loop_with_a_supersampled_map(mode, tmp_path, hip_lib):
    from bhr_amd import drivers
    from bhr_amd.camera import orbit_position
    W, H, N, NS, K = 48, 27, 6, 3, 2
    cam0, fov, speed, deg, S = [6, 0, 0.5], 90, 0.1, 90.0, 0.5
    orbit = mode == "orbit_map"
    shutter = S if mode == "shutter_map" else 0.0
    out = str(tmp_path / mode / "v.mp4")
    r, _, _, _ = drivers.make_renderer(W, H, cam0, fov, n_stars=50, tex_w=256, tex_h=128, math="strict")
    drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=out, fov=fov, static_cam_pos=cam0, orbit=orbit, orbit_degrees=deg,
                         disk_rotation_speed=speed, video_stream="off", assemble=False, shutter=shutter, shutter_samples=NS,
                         map_supersample=K, **{mode: True})
    assert r.ray_map_info()["built"] == 0                # freed at the end
    r.close()
    d = drivers._frames_dir(out)
    names = [f"frame_{f:04d}.png" for f in range(N)]
    assert sorted(os.listdir(d)) == names + ["progress.json"]
    params = json.load(open(os.path.join(d, "progress.json")))["params"]
    assert params["map_supersample"] == K and params[mode] is True

    # the same loop by hand
    frames = {}
    for k in (K, 1):
        r, _, _, _ = drivers.make_renderer(W, H, cam0, fov, n_stars=50, tex_w=256, tex_h=128, math="strict")
        r.set_outputs("u8")
        factories = drivers.init_lifecycle_system(r, r.dtex_h, r.dtex_w, seed=42)
        r.build_ray_map(orbit_position(cam0, 0, N, deg) if orbit else cam0, fov, supersample=k)
        assert r.ray_map_info()["supersample"] == k
        frames[k] = []
        for f in range(N if k == K else 1):
            drivers.advance_lifecycle_frame(r, factories, f * speed, speed, recompute_stats=(f % 60 == 0), compose=True)
            if mode == "shutter_map":
                r.render_shutter_from_ray_map_async([(u - f) * speed for u in drivers.shutter_times(f, S, NS)], None, fov)
            elif orbit:
                r.render_from_ray_map_async(frame=0, cam_pos=orbit_position(cam0, f, N, deg), fov=fov)
            else:
                r.render_from_ray_map_async(frame=0)
            frames[k].append(r.read_final_u8())
        r.close()
    for f in range(N):
        np.testing.assert_array_equal(_png(os.path.join(d, names[f])), frames[K][f], err_msg=f"frame {f}")
    assert (frames[K][0] != frames[K][N - 1]).any()          # the video moves
    assert (frames[K][0] != frames[1][0]).any()              # ... and the factor reached the frames
