"""Supersampled Kerr ray maps on the device (option "kerr_raymap_supersample", HipRenderer.build_kerr_ray_map(supersample=k);
include/bhr.h states the contract, csrc/march_kerr_raymap.hip has the kernels): the map of the fine frame, k x k Kerr record
lists per pixel, resolved in the shade.  Every comparison is exact.

The yardsticks are never the code under test:
  (A) the marched Kerr frame of a fresh strict context with set_supersample(k), same spin and redshift -- the marched
      supersampled Kerr kernels;
  (B) tests/supersample_ref.box_resolve of the skip-bloom BG / DISK of a k = 1 Kerr map frame from a context of k W x k H
      pixels (its pixel pitch is the fine camera's bit for bit) -- the k = 1 map kernels and the NumPy statement of the filter;
      turned to the same camera for turned views.

Scene and constants: tests/kerr_cases.py.  Frames: 21 x 13 (fine 42 x 26 and 84 x 52: partial fine tiles on both sides), 5 x 3 at
k = 8 (one output pixel per tile, the whole butterfly), 12 x 8 (fine tiles that are whole at k = 2), 24 x 16 (turned), 48 x 32
(the hole's image at fov 40: rays with two crossings, overflow groups), 64 x 40 (video)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import kerr_cases as KC
from supersample_ref import box_resolve

pytestmark = pytest.mark.gpu

KW = dict(step_size=KC.STEP, r_max=KC.R_MAX, r_disk_inner=KC.R_INNER, r_disk_outer=KC.R_OUTER, disk_tilt=0.0, anti_alias="disabled",
          disk_rotation_speed=0.1)
# ROLLS of tests/test_gpu_kerr_raymap.py: (t_offset of the map frame, frame number of the marched one; float32(frame * 0.1) is the same float)
ROLLS = ((0.0, 0), (7.3, 73), (float(np.float32(400 * 0.1)), 400))
VIEW, FOV = KC.VIEWS[0], KC.FOV
N_ORBIT = 24
LAYERS = ("final", "bg", "disk")


def _scene(roll=0):
    sky, tex = KC.scene()
    if roll == 0:
        return sky, tex
    return np.ascontiguousarray(np.roll(sky, -roll, axis=1)), np.ascontiguousarray(np.roll(tex, -roll, axis=1))


def _mk(A, redshift="model", force=False, width=21, height=13, roll=0, **kw):
    from bhr_amd import HipRenderer
    sky, tex = _scene(roll)
    r = HipRenderer(width, height, sky, tex, math="strict", **{**KW, **kw})
    if A != 0.0 or force:
        r.set_spin(A, force_kerr=force)
    if redshift == "exact":
        r.set_redshift("exact")
    return r


def _set_scene(r, roll):
    from bhr_amd import _lib
    sky, tex = _scene(roll)
    _lib.check(r._lib.bhr_set_skybox(r._ctx, _lib.fptr(sky), sky.shape[0], sky.shape[1]))
    r.update_disk_texture(tex)


def _read(r, names=LAYERS, u8=True):
    from bhr_amd import _lib
    ids = dict(final=_lib.LAYER_FINAL, bg=_lib.LAYER_BG, disk=_lib.LAYER_DISK)
    out = {k: r.read_layer(ids[k]) for k in names}
    if u8:
        out["u8"] = r.read_final_u8()
    return out


def _assert_equal(got, want, tag, names=None):
    for k in names or [n for n in want if n in got]:
        bad = int((got[k] != want[k]).any(axis=-1).sum())
        assert bad == 0, f"{tag} {k}: {bad} pixels differ (max |d| {np.abs(got[k].astype(np.float64) - want[k]).max():.3g})"


def _orbit_cam(f, pov=VIEW):
    from bhr_amd.camera import orbit_position
    return [float(v) for v in orbit_position(list(pov), f, N_ORBIT)]


def _groups(plane, k):
    """(k H, k W) -> (H, W, k k): the sub-samples of every output pixel."""
    h, w = plane.shape[0] // k, plane.shape[1] // k
    return plane.reshape(h, k, w, k).transpose(0, 2, 1, 3).reshape(h, w, k * k)


# ---- 1. a still camera ------------------------------------------------------------------------------------------------------------------
STILL = [(21, 13, 2, A, m, False) for A in (0.6, -0.9, 0.998) for m in ("model", "exact")] + \
        [(21, 13, 2, 0.0, "model", True), (21, 13, 4, 0.6, "model", False), (21, 13, 4, -0.9, "exact", False),
         (5, 3, 8, 0.6, "model", False), (5, 3, 8, 0.998, "exact", False), (12, 8, 2, 0.6, "model", False), (12, 8, 2, -0.9, "exact", False)]


@pytest.mark.parametrize("W, H, k, A, redshift, force", STILL, ids=lambda v: str(v))
def test_map_frame_is_the_marched_supersampled_kerr_frame(W, H, k, A, redshift, force, hip_lib):
    tag0 = f"{W}x{H} k={k} A={A} {redshift}"
    r = _mk(A, redshift, force, W, H)
    r.build_kerr_ray_map(list(VIEW), FOV, supersample=k)
    info = r.kerr_ray_map_info()
    assert (info["built"], info["supersample"], info["width"], info["rows"], info["redshift"]) == (1, k, W, H, redshift)
    marched = _mk(A, redshift, force, W, H)                   # (A): a fresh context that marches k x k Kerr rays per pixel
    marched.set_supersample(k)
    fine = _mk(A, redshift, force, k * W, k * H)              # (B): the k = 1 Kerr map of the fine frame
    fine.build_kerr_ray_map(list(VIEW), FOV)
    assert fine.kerr_ray_map_info()["supersample"] == 1
    frames = []
    for n, (t, frame) in enumerate(ROLLS + (ROLLS[1],)):
        swapped = n == len(ROLLS)
        if swapped:                                           # the map outlives a scene swap: it holds no scene
            for ctx in (r, marched, fine):
                _set_scene(ctx, 37)
        tag = f"{tag0} t={t:g}" + (" swapped" if swapped else "")
        r.render_from_kerr_ray_map_async(t_offset=t)
        got = _read(r)
        marched.render_async(list(VIEW), FOV, frame=frame)
        want = _read(marched)
        _assert_equal(got, want, tag + " (A)", LAYERS + ("u8",))
        assert info["ray_steps"] == marched.counters()["ray_steps"], (tag, info["ray_steps"], marched.counters()["ray_steps"])
        fine.render_from_kerr_ray_map_async(t_offset=t, skip_bloom=True)
        f = _read(fine, ("bg", "disk"), u8=False)
        _assert_equal(got, {name: box_resolve(f[name], k) for name in ("bg", "disk")}, tag + " (B)", ("bg", "disk"))
        assert (want["disk"] > 0).any() and (want["bg"] > 0).any(), f"{tag}: a blank frame"
        frames.append(got)
    assert (frames[0]["disk"] != frames[1]["disk"]).any(), "the roll changed nothing"
    assert (frames[1]["final"] != frames[3]["final"]).any(), "the scene swap changed nothing"
    # the k = 1 frame of the view is another picture: the test can fail
    marched.set_supersample(1)
    marched.render_async(list(VIEW), FOV, frame=ROLLS[1][1])
    one = _read(marched, ("bg", "disk"), u8=False)
    assert (one["bg"] != frames[3]["bg"]).any() and (one["disk"] != frames[3]["disk"]).any(), "the k = 1 frame: the test cannot fail"
    for ctx in (r, marched, fine):
        ctx.close()


# ---- 2. overflow groups -----------------------------------------------------------------------------------------------------------------
OVER_W, OVER_H = 48, 32


@pytest.mark.parametrize("redshift", ["model", "exact"])
def test_overflow_groups_are_remarched_whole(redshift, hip_lib):
    """KC.CROSSINGS[0] (A 0.998, fov 40, r_inner 0.7: rays that cross the annulus twice) at k = 2 with 1, 4 and 8 slots, against (A).
    With one slot some groups hold a ray with two crossings beside rays with one or none: the group-wise OR of the build and of the
    shade, and the fix kernel's resolve of whole groups, all run.
    Frame size 48 x 32, the first one tried.  Seen on the device (MI355X) with one slot, under either redshift: 315 listed
    groups, 62 of them mixed."""
    e, k, W, H = KC.CROSSINGS[0], 2, OVER_W, OVER_H
    marched = _mk(e.A, redshift, width=W, height=H, r_disk_inner=e.r_inner)
    marched.set_supersample(k)
    want = []
    for t, frame in ROLLS[:2]:
        marched.render_async(list(e.view), e.fov, frame=frame)
        want.append((_read(marched), marched.counters()["ray_steps"]))
    marched.close()
    assert (want[0][0]["disk"] > 0).any() and (want[0][0]["bg"] > 0).any()
    r = _mk(e.A, redshift, width=W, height=H, r_disk_inner=e.r_inner)
    overflow = {}
    for slots in (1, 4, 8):
        r.set_option("raymap_slots", slots)
        r.build_kerr_ray_map(list(e.view), e.fov, supersample=k)
        info, p = r.kerr_ray_map_info(), r.kerr_ray_map_passes()
        assert info["slots"] == slots and info["supersample"] == k and p["crossings"].shape == (k * H, k * W)
        assert info["ray_steps"] == want[0][1] == int(p["steps"].astype(np.int64).sum())
        over = _groups(p["crossings"], k) > slots                     # (H, W, k k): the rays over the slots
        listed = over.any(axis=-1)                                    # ... and the groups that hold one: listed whole
        mixed = listed & ~over.all(axis=-1)                           # a ray with crossings <= K beside a ray over K
        overflow[slots] = info["overflow_pixels"]
        assert info["overflow_pixels"] == k * k * int(listed.sum()) and info["overflow_pixels"] % (k * k) == 0
        assert info["crossings_stored"] == int(np.minimum(p["crossings"], slots).sum())
        if slots == 1:
            print(f"\n[kerr map supersample] {redshift} {W}x{H} k={k} K=1: {int(listed.sum())} listed groups, {int(mixed.sum())} of them mixed")
            assert int(listed.sum()) > 0, "no listed group: the fix kernel did not run"
            assert int(mixed.sum()) > 0, "no mixed group: the group-wise OR is not exercised"
        for (t, frame), (frame_want, _) in zip(ROLLS[:2], want):
            r.render_from_kerr_ray_map_async(t_offset=t)
            _assert_equal(_read(r), frame_want, f"K={slots} {redshift} t={t:g} (A)", LAYERS + ("u8",))
            # the frame's counter: the steps of the re-march of every ray of every listed group
            assert r.counters()["ray_steps"] == int(_groups(p["steps"], k)[listed].astype(np.int64).sum())
    assert overflow[8] <= overflow[4] < overflow[1]
    r.close()


# ---- 3. turned about z, the spin axis ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, A, redshift", [(2, 0.6, "model"), (4, 0.6, "exact"), (2, -0.9, "exact"), (4, -0.9, "model")])
def test_turned_map_frames(k, A, redshift, hip_lib):
    """Orbit positions 0, 1 and 17 of 24 against (B) turned to the same camera: the same fine rays, the same turn, the NumPy filter.
    Eight slots, so that no ray of either map is on an overflow list (a listed GROUP is re-marched whole from the turned camera,
    a listed ray of the k = 1 map alone: the two would differ by two Kerr marches of symmetric views)."""
    W, H, t = 24, 16, 0.5
    cam0 = _orbit_cam(0)                                     # the orbit's radius is |pov|: frame 0 is not the pov itself
    r = _mk(A, redshift, width=W, height=H, options={"raymap_slots": 8})
    r.build_kerr_ray_map(cam0, FOV, supersample=k)
    fine = _mk(A, redshift, width=k * W, height=k * H, options={"raymap_slots": 8})
    fine.build_kerr_ray_map(cam0, FOV)
    assert r.kerr_ray_map_info()["overflow_pixels"] == 0 and fine.kerr_ray_map_info()["overflow_pixels"] == 0, "a ray over eight crossings"
    frames = {}
    for f in (0, 1, 17):
        cam = _orbit_cam(f)
        r.render_from_kerr_ray_map_async(t_offset=t, cam_pos=cam, skip_bloom=True)
        frames[f] = _read(r, ("bg", "disk"), u8=False)
        fine.render_from_kerr_ray_map_async(t_offset=t, cam_pos=cam, skip_bloom=True)
        ff = _read(fine, ("bg", "disk"), u8=False)
        _assert_equal(frames[f], {name: box_resolve(ff[name], k) for name in ("bg", "disk")}, f"k={k} A={A} {redshift} orbit frame {f} (B)")
        assert (frames[f]["disk"] > 0).any() and (frames[f]["bg"] > 0).any()
    for f in (1, 17):
        assert (frames[f]["bg"] != frames[0]["bg"]).any() and (frames[f]["disk"] != frames[0]["disk"]).any(), "the turn changed nothing"
    fine.close()
    # at the build camera: the still map frame, which is the marched supersampled frame, in every layer
    r.render_from_kerr_ray_map_async(t_offset=t, cam_pos=cam0)
    got = _read(r)
    r.render_from_kerr_ray_map_async(t_offset=t)
    still = _read(r)
    r.close()
    _assert_equal(got, still, "angle 0 against the still frame", LAYERS + ("u8",))
    marched = _mk(A, redshift, width=W, height=H)
    marched.set_supersample(k)
    marched.render_async(cam0, FOV, frame=5)                 # float32(5 * 0.1) == 0.5
    _assert_equal(got, _read(marched), "angle 0 (A)", LAYERS + ("u8",))
    marched.close()


# ---- 4. one context, many maps ----------------------------------------------------------------------------------------------------------
def test_one_context_many_maps(hip_lib):
    W, H, k, A = 21, 13, 2, 0.6
    view, other = list(VIEW), list(KC.VIEWS[1])
    # (A) for the map frames
    marched = _mk(A, width=W, height=H)
    marched.set_supersample(k)
    want_ss = {}
    for t, frame in ROLLS:
        marched.render_async(view, FOV, frame=frame)
        want_ss[t] = _read(marched)
    marched.close()

    r = _mk(0.0, width=W, height=H, frame_slots=2)
    assert r.frame_slots == 2
    # a Schwarzschild map, built at spin 0, held by the same context throughout
    r.build_ray_map(view, FOV, skip_differentials=True)
    r.render_from_ray_map_async(frame=3)
    S, schw = _read(r), r.ray_map_info()
    r.set_spin(A)

    def own(pos, frame=0):
        r.render_async(pos, FOV, frame=frame)
        return _read(r)

    first, first_other = own(view), own(other, 73)           # the context's own marched Kerr frames, one ray per pixel
    assert r.kerr_ray_map_info() == {**r.kerr_ray_map_info(), "built": 0, "supersample": 1}
    r.build_kerr_ray_map(view, FOV, supersample=k)
    two = r.kerr_ray_map_info()
    _assert_equal(own(view), first, "the context's marched frame behind a k = 2 build", LAYERS + ("u8",))
    assert (first["final"] != want_ss[0.0]["final"]).any()
    # map frames and marched frames over both slots
    for step, (what, arg) in enumerate([("map", 0.0), ("march", view), ("map", 7.3), ("march", other), ("march", view), ("map", 0.0), ("map", ROLLS[2][0])]):
        if what == "map":
            r.render_from_kerr_ray_map_async(t_offset=arg)
            _assert_equal(_read(r), want_ss[arg], f"step {step}: map frame t={arg:g}", LAYERS + ("u8",))
        else:
            got = own(arg, 0 if arg is view else 73)
            _assert_equal(got, first if arg is view else first_other, f"step {step}: marched frame", LAYERS + ("u8",))
    assert r.ray_map_info() == schw
    # back to one ray per pixel: the k = 1 map's contract holds again
    r.build_kerr_ray_map(view, FOV, supersample=1)
    one = r.kerr_ray_map_info()
    assert one["supersample"] == 1 and r.kerr_ray_map_passes()["steps"].shape == (H, W)
    r.render_from_kerr_ray_map_async(t_offset=0.0)
    _assert_equal(_read(r), first, "the k = 1 map frame again", LAYERS + ("u8",))
    # device memory: k^2 x (24 + K x 20) bytes per output pixel and 4 per entry of the overflow list, whose capacity is the fine
    # plane rounded up to 256; the counters do not scale
    K = one["slots"]
    per_ray = 24 + K * 20
    cap = lambda n: (n + 255) // 256 * 256
    assert two["device_bytes"] - one["device_bytes"] == (k * k - 1) * W * H * per_ray + 4 * (cap(k * k * W * H) - cap(W * H))
    assert (two["supersample"], two["width"], two["rows"], two["slots"]) == (k, W, H, K)
    r.free_kerr_ray_map()
    assert r.kerr_ray_map_info()["built"] == 0 and r.kerr_ray_map_info()["supersample"] == 1 and r.kerr_ray_map_info()["device_bytes"] == 0
    # the Schwarzschild map is as it was, and gives its frame once the spin is off
    assert r.ray_map_info() == schw
    r.set_spin(0.0)
    r.render_from_ray_map_async(frame=3)
    _assert_equal(_read(r), S, "the Schwarzschild map's frame behind the Kerr maps' lives", LAYERS + ("u8",))
    r.close()


# ---- 5. bookkeeping and refusals --------------------------------------------------------------------------------------------------------
def _refused(r, words, call, exc=ValueError):
    """`call` raises exc (ValueError: BHR_ERR_INVALID; AssertionError: BHR_ERR_STATE) with every word in the message and launches nothing."""
    before = r.counters()["frames_timed"]
    with pytest.raises(exc) as e:
        call()
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert r.counters()["frames_timed"] == before


def test_bookkeeping_and_refusals(hip_lib):
    from bhr_amd import _lib
    lib = hip_lib
    W, H, k, A = 21, 13, 2, 0.6
    view = list(VIEW)
    r = _mk(A, width=W, height=H)
    cam = r.camera_uniforms(view, FOV)
    got = C.c_int32(-1)
    assert lib.bhr_kerr_raymap_get_supersample(r._ctx, C.byref(got)) == 0 and got.value == 1       # no map: 1, and no failure
    assert r.kerr_ray_map_info()["supersample"] == 1 and r.kerr_ray_map_info()["built"] == 0
    # the option
    for bad in (3, 0, 16, -2, 2.5, 6):
        assert lib.bhr_set_option(r._ctx, b"kerr_raymap_supersample", float(bad)) == _lib.BHR_ERR_INVALID
        assert b"kerr_raymap_supersample" in lib.bhr_last_error()
    for bad in (3, 0):
        with pytest.raises(ValueError):
            r.set_option("kerr_raymap_supersample", bad)
        with pytest.raises(ValueError):
            r.build_kerr_ray_map(view, FOV, supersample=bad)
    assert r.kerr_ray_map_info()["built"] == 0 and r.kerr_ray_map_info()["device_bytes"] == 0
    # ... and from the environment of bhr_create: the build refuses
    saved = os.environ.get("BHR_KERR_RAYMAP_SUPERSAMPLE")
    os.environ["BHR_KERR_RAYMAP_SUPERSAMPLE"] = "3"
    try:
        env = _mk(A, width=W, height=H)
    finally:
        if saved is None:
            os.environ.pop("BHR_KERR_RAYMAP_SUPERSAMPLE", None)
        else:
            os.environ["BHR_KERR_RAYMAP_SUPERSAMPLE"] = saved
    assert lib.bhr_kerr_raymap_build(env._ctx, C.byref(cam), 0) == _lib.BHR_ERR_INVALID and b"kerr_raymap_supersample" in lib.bhr_last_error()
    assert env.kerr_ray_map_info()["built"] == 0 and env.kerr_ray_map_info()["device_bytes"] == 0
    env.close()
    # the build, its planes and its counts
    for slots in (4, 2):
        r.set_option("raymap_slots", slots)
        r.build_kerr_ray_map(view, FOV, supersample=k)
        info, p = r.kerr_ray_map_info(), r.kerr_ray_map_passes()
        assert (info["built"], info["supersample"], info["slots"], info["width"], info["rows"]) == (1, k, slots, W, H)
        assert lib.bhr_kerr_raymap_get_supersample(r._ctx, C.byref(got)) == 0 and got.value == k
        assert p["steps"].shape == p["status"].shape == p["crossings"].shape == (k * H, k * W)
        assert p["escape_dir"].shape == (k * H, k * W, 3) and p["hits"].shape == (slots, k * H, k * W, 5)
        assert int(p["steps"].astype(np.int64).sum()) == info["ray_steps"]
        assert info["crossings_stored"] == int(np.minimum(p["crossings"], slots).sum()) > 0
        assert info["overflow_pixels"] == k * k * int((_groups(p["crossings"], k) > slots).any(axis=-1).sum())
        for c in range(slots):                                   # no record beyond a ray's crossings
            assert not p["hits"][c][p["crossings"] <= c].any()
        # k^2 (24 + K 20) bytes per output pixel and the list's 4; beyond them only the list's round-up and the map's counters
        planes = k * k * W * H * (24 + slots * 20 + 4)
        assert 0 <= info["device_bytes"] - planes <= 255 * 4 + 16 * 4 + (8 + 128 * 32) * 8
        buf = np.zeros((H, W), dtype=np.int32)                   # the planes are fine-sized: the output frame's size is refused
        assert lib.bhr_kerr_raymap_read(r._ctx, _lib.RAYMAP_STEPS, buf.ctypes.data, buf.nbytes) == _lib.BHR_ERR_INVALID
    n0 = r.counters()["frames_timed"]
    r.render_from_kerr_ray_map_async(t_offset=0.3)
    want = _read(r)
    assert r.counters()["frames_timed"] == n0 + 1                # one timing-ring entry, like any frame
    assert r.counters()["rays"] == k * k * W * H
    r.render_async(view, FOV)
    own = _read(r)

    def renders_as_before():
        r.render_from_kerr_ray_map_async(t_offset=0.3)
        _assert_equal(_read(r), want, "the map frame after a refusal", LAYERS + ("u8",))
        r.render_async(view, FOV)
        _assert_equal(_read(r), own, "the marched frame after a refusal", LAYERS + ("u8",))

    # the context's own supersampling stays refused: the message names both factors
    r.set_supersample(2)
    _refused(r, ("bhr_kerr_raymap_build", "supersampling is on (factor 2)", "one ray per pixel", "kerr_raymap_supersample", "bhr_set_supersample"),
             lambda: r.build_kerr_ray_map(view, FOV, supersample=k))
    _refused(r, ("bhr_kerr_raymap_render", "supersampling is on (factor 2)"), lambda: r.render_from_kerr_ray_map_async())
    r.set_supersample(1)
    renders_as_before()
    # a Kerr polarisation: the momentum build and the Kerr Stokes kernel have no supersampled twin
    r.set_kerr_polarization("toroidal")
    _refused(r, ("bhr_kerr_raymap_build", "kerr_raymap_supersample", "polarisation", "bhr_set_kerr_polarization"),
             lambda: r.build_kerr_ray_map(view, FOV, supersample=k))
    _refused(r, ("bhr_kerr_raymap_render", "bhr_set_kerr_polarization"), lambda: r.render_from_kerr_ray_map_async(t_offset=0.3), AssertionError)
    r.set_kerr_polarization(None)
    assert r.kerr_ray_map_info()["built"] == 1 and r.kerr_ray_map_info()["supersample"] == k      # the map stayed
    renders_as_before()
    # "raymap_supersample" stays the Schwarzschild map's: refused with the words it always had
    r.set_option("raymap_supersample", 2)
    _refused(r, ("bhr_kerr_raymap_build: raymap_supersample 2; a Kerr ray map has no supersampled form (1 only)",),
             lambda: r.build_kerr_ray_map(view, FOV, supersample=k))
    r.set_option("raymap_supersample", 1)
    renders_as_before()
    # a turned view of the k = 2 map takes render_view's checks as ever
    _refused(r, ("bhr_kerr_raymap_render_view",), lambda: r.render_from_kerr_ray_map_async(cam_pos=[6.0, 0.0, 0.7]))
    r.free_kerr_ray_map()
    assert lib.bhr_kerr_raymap_get_supersample(r._ctx, C.byref(got)) == 0 and got.value == 1
    with pytest.raises(AssertionError):
        r.kerr_ray_map_passes()
    r.close()


# ---- 6. video ---------------------------------------------------------------------------------------------------------------------------
def _video(tmp_path, name, orbit, renderer, resume=False, **kw):
    from bhr_amd import drivers
    out = str(tmp_path / name / "v.mp4")
    drivers.render_video(renderer, 64, 40, n_frames=6, fps=24, output_path=out, fov=FOV, static_cam_pos=list(VIEW), orbit=orbit, resume=resume,
                         video_stream="off", assemble=False, **kw)
    d = drivers._frames_dir(out)
    frames = [open(os.path.join(d, f"frame_{f:04d}.png"), "rb").read() for f in range(6)]
    with open(os.path.join(d, "progress.json")) as fh:
        rec = json.load(fh)
    return frames, rec


def _decode(png):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGB"), dtype=np.float64) / 255.0


@pytest.mark.parametrize("orbit", [False, True], ids=["still", "orbit"])
def test_video(orbit, tmp_path, hip_lib, capsys):
    k = 2
    m = _mk(0.6, width=64, height=40)
    m.set_supersample(k)
    marched, rec0 = _video(tmp_path, "marched", orbit, m)
    m.close()
    assert "spin_map" not in rec0["params"] and "spin_map_supersample" not in rec0["params"]
    r = _mk(0.6, width=64, height=40)
    mapped, rec1 = _video(tmp_path, "mapped", orbit, r, spin_map=True, spin_map_supersample=k)
    assert rec1["params"]["spin_map"] is True and rec1["params"]["spin_map_supersample"] == k and rec1["completed"] == list(range(6))
    assert r.kerr_ray_map_info()["built"] == 0               # freed at the end
    assert mapped[0] == marched[0]
    if not orbit:
        assert mapped == marched                             # byte-identical frame files
        assert mapped[0] != mapped[5]                        # the video moves
    else:
        for f in range(1, 6):
            e = KC.rmse(_decode(mapped[f]), _decode(marched[f]))
            print(f"\n[kerr map supersample video] orbit frame {f}: RMSE to the marched frame {e:.3g}")
            assert e <= 1.0 / 255.0 and mapped[f] != mapped[0]
    # a resume with the same factor takes the frames up; with another it starts over
    capsys.readouterr()
    _video(tmp_path, "mapped", orbit, r, resume=True, spin_map=True, spin_map_supersample=k)
    assert "Resuming: 6/6" in capsys.readouterr().out
    again, rec2 = _video(tmp_path, "mapped", orbit, r, resume=True, spin_map=True, spin_map_supersample=1)
    assert "starting over" in capsys.readouterr().out and "spin_map_supersample" not in rec2["params"] and rec2["params"]["spin_map"] is True
    assert again[0] != mapped[0]                             # the factor reached the frames
    r.close()
