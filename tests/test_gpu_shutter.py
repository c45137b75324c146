"""Motion blur on the device (bhr_render_shutter; include/bhr.h states the frame): the BG and DISK layers of a shutter frame
are the sequential f32 mean (tests/shutter_ref.py) of its samples' layers, each bit for bit the layer a skip-bloom bhr_render
of that sample's camera stores; the post-pass is bhr_bloom's on the resolved layers.  Frame slots, supersampling, counters,
refusals and the video loop.

The frames are small on purpose: 21 x 13 has 819 floats per layer (no multiple of 4: the accumulation kernel's scalar tail),
24 x 15 is tilted and anti-aliased (guards and fix list under hybrid), 50 x 27 has more than one accumulation block; the hybrid
cases use 96 x 54, the smallest of the suite's frames with strict and fast tiles."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest

from shutter_ref import resolve

pytestmark = pytest.mark.gpu

VIEWS = {
    "odd": dict(W=21, H=13, cam=(6.0, 0.0, 0.5), fov=90.0, kw=()),
    "tilt": dict(W=24, H=15, cam=(5.0, 2.0, 1.0), fov=80.0, kw=(("anti_alias", "lod_radius"), ("disk_tilt", 20.0))),
    "blocks": dict(W=50, H=27, cam=(6.0, 0.0, 0.5), fov=90.0, kw=()),
    "wide": dict(W=96, H=54, cam=(6.0, 0.0, 0.5), fov=90.0, kw=()),
    "wide_aa": dict(W=96, H=54, cam=(5.0, 2.0, 1.0), fov=80.0, kw=(("anti_alias", "lod_radius"), ("disk_tilt", 20.0))),
}
SMALL = ("odd", "tilt", "blocks")
NS = (1, 2, 3, 5, 8)
LAYERS = ("final", "bg", "disk", "blur")


def _view_of(math_mode, n):
    """The views take turns over n, so that every arithmetic meets every shape; hybrid needs a frame with strict tiles."""
    i = NS.index(n)
    return ("wide", "wide_aa")[i % 2] if math_mode == "hybrid" else SMALL[i % 3]


def _samples(view, n):
    """Sample j of a view: the camera turned by j / 7 of a 10 degree orbit arc, and a t_offset of its own -- the same for
    every n, so that the single frames are shared by the cases."""
    x, y, z = VIEWS[view]["cam"]
    pos, toff = [], []
    for j in range(n):
        a = math.radians(10.0) * j / 7
        pos.append([x * math.cos(a) - y * math.sin(a), x * math.sin(a) + y * math.cos(a), z])
        toff.append(0.3 + 0.17 * j)
    return pos, toff


def _mk(view, math_mode, **kw):
    from bhr_amd import HipRenderer, scenes
    v = VIEWS[view]
    return HipRenderer(v["W"], v["H"], scenes.analytic_skybox(), scenes.noisy_disk(), math=math_mode, **dict(v["kw"]), **kw)


def _render_one(r, pos, fov, t_offset, skip_bloom=False):
    """bhr_render of one sample's camera (render_async takes a frame number, not a t_offset)."""
    from bhr_amd import _lib
    cam = r.camera_uniforms(pos, fov, t_offset=t_offset)
    _lib.check(r._lib.bhr_render(r._ctx, C.byref(cam), _lib.SKIP_BLOOM if skip_bloom else 0))


def _read(r, names=LAYERS):
    from bhr_amd import _lib
    ids = dict(final=_lib.LAYER_FINAL, bg=_lib.LAYER_BG, disk=_lib.LAYER_DISK, blur=_lib.LAYER_BLUR)
    return {k: r.read_layer(ids[k]) for k in names}


@functools.lru_cache(maxsize=None)
def _singles(view, math_mode, sampling=(1, None)):
    """The eight samples of a view rendered one by one with skip_bloom on ONE fresh context: BG, DISK, ray_steps of each."""
    r = _mk(view, math_mode, supersample=sampling[0], supersample_threshold=sampling[1])
    pos, toff = _samples(view, 8)
    out = []
    for p, t in zip(pos, toff):
        _render_one(r, p, VIEWS[view]["fov"], t, skip_bloom=True)
        got = _read(r, ("bg", "disk"))
        got["ray_steps"] = r.counters()["ray_steps"]
        out.append(got)
    r.close()
    return out


@functools.lru_cache(maxsize=None)
def _shutter(view, math_mode, n, sampling=(1, None)):
    r = _mk(view, math_mode, supersample=sampling[0], supersample_threshold=sampling[1])
    pos, toff = _samples(view, n)
    r.render_shutter_async(pos, VIEWS[view]["fov"], toff, skip_bloom=True)
    out = _read(r, ("bg", "disk"))
    out["c"] = r.counters()
    r.close()
    return out


def _assert_equal(got, want, tag, names):
    for k in names:
        bad = int((got[k] != want[k]).any(axis=-1).sum())
        assert bad == 0, f"{tag} {k}: {bad} pixels differ (max |d| {np.abs(got[k].astype(np.float64) - want[k]).max():.3g})"


@pytest.mark.parametrize("math_mode", ["strict", "fast", "hybrid"])
@pytest.mark.parametrize("n", NS)
def test_layers_are_the_f32_mean_of_the_samples(n, math_mode, hip_lib):
    view = _view_of(math_mode, n)
    single = _singles(view, math_mode)[:n]
    got = _shutter(view, math_mode, n)
    want = {k: resolve([s[k] for s in single]) for k in ("bg", "disk")}
    _assert_equal(got, want, f"{view} {math_mode} n={n}", ("bg", "disk"))
    if n > 1:                                                   # the samples really differ: the test can fail
        assert (single[0]["bg"] != single[n - 1]["bg"]).any() and (single[0]["disk"] != single[n - 1]["disk"]).any()
    assert got["disk"].min() >= 0.0 and got["disk"].max() <= 1.0


@pytest.mark.parametrize("math_mode", ["strict", "fast", "hybrid"])
@pytest.mark.parametrize("n", [1, 3, 8])
def test_counters_are_the_sums_over_the_samples(n, math_mode, hip_lib):
    view = _view_of(math_mode, n)
    v = VIEWS[view]
    c = _shutter(view, math_mode, n)["c"]
    assert c["rays"] == n * v["W"] * v["H"]
    assert c["ray_steps"] == sum(s["ray_steps"] for s in _singles(view, math_mode)[:n]) > 0
    assert c["frames_timed"] == 1 and c["ray_steps_sum"] == c["ray_steps"]        # one entry in the timing ring
    assert c["march_ms"] > 0 and c["frame_ms"] >= c["march_ms"]


@pytest.mark.parametrize("lens_flare", [False, True])
@pytest.mark.parametrize("math_mode", ["strict", "fast"])
def test_post_pass_is_bloom_of_the_resolved_layers(math_mode, lens_flare, hip_lib):
    """strict: the exact f32 post-pass; fast: the split-f16 one (pack, H, V)."""
    from bhr_amd import _lib
    view, n = "blocks", 3
    pos, toff = _samples(view, n)
    r = _mk(view, math_mode)
    r.render_shutter_async(pos, VIEWS[view]["fov"], toff, lens_flare=lens_flare)
    got = _read(r)
    u8 = r.read_final_u8()
    r.close()
    single = _singles(view, math_mode)[:n]
    want_layers = {k: resolve([s[k] for s in single]) for k in ("bg", "disk")}
    _assert_equal(got, want_layers, f"{math_mode} flare={lens_flare}", ("bg", "disk"))
    ref = _mk(view, math_mode)
    ref.write_layer(_lib.LAYER_BG, want_layers["bg"])
    ref.write_layer(_lib.LAYER_DISK, want_layers["disk"])
    ref.bloom_only()
    if lens_flare:
        ref.apply_lens_flare()
    want = _read(ref)
    ref.close()
    _assert_equal(got, want, f"{math_mode} flare={lens_flare}", LAYERS)
    assert got["blur"].max() > 0.0
    np.testing.assert_array_equal(u8, (np.clip(got["final"], 0.0, 1.0) * np.float32(255.0)).astype(np.uint8))


@pytest.mark.parametrize("math_mode,view", [("strict", "odd"), ("fast", "blocks"), ("hybrid", "wide_aa")])
def test_one_sample_is_the_plain_frame(math_mode, view, hip_lib):
    pos, toff = _samples(view, 2)
    a, b = _mk(view, math_mode), _mk(view, math_mode)
    a.render_shutter_async(pos[1:], VIEWS[view]["fov"], toff[1:])
    _render_one(b, pos[1], VIEWS[view]["fov"], toff[1])
    got, want = _read(a), _read(b)
    np.testing.assert_array_equal(a.read_final_u8(), b.read_final_u8())
    a.close()
    b.close()
    _assert_equal(got, want, f"{math_mode} {view}", LAYERS)


def test_shutter_frames_on_two_slots_equal_one_slot(hip_lib):
    """Shutter frame A, a plain frame, shutter frame B of another view with fewer samples, A again: every frame of the
    two-slot context equals the one-slot context's, and the second A the first -- no shared or stale accumulator."""
    view, fov = "wide", VIEWS["wide"]["fov"]
    pos_a, toff_a = _samples(view, 5)
    pos_b = [[-p[0], p[1] + 1.0, 0.3] for p in pos_a[:2]]
    toff_b = [0.9, 1.4]

    def sequence(slots):
        r = _mk(view, "hybrid", frame_slots=slots)
        assert r.frame_slots == slots
        frames = []
        for step in ("A", "plain", "B", "A"):
            if step == "A":
                r.render_shutter_async(pos_a, fov, toff_a)
            elif step == "B":
                r.render_shutter_async(pos_b, fov, toff_b)
            else:
                r.render_async([3.2, 0.5, 0.12], 100.0)
            frames.append(_read(r))
        r.close()
        return frames

    one, two = sequence(1), sequence(2)
    for k, (g, w) in enumerate(zip(two, one)):
        _assert_equal(g, w, f"frame {k}", LAYERS)
    _assert_equal(two[3], two[0], "A again", LAYERS)
    assert (two[0]["final"] != two[2]["final"]).any() and (two[0]["final"] != two[1]["final"]).any()
    single = _singles(view, "hybrid")[:5]
    _assert_equal(two[0], {k: resolve([s[k] for s in single]) for k in ("bg", "disk")}, "A", ("bg", "disk"))


@pytest.mark.parametrize("math_mode,view,sampling", [("fast", "odd", (2, None)), ("strict", "tilt", (2, None)),
                                                      ("hybrid", "wide", (2, 0.25))])
def test_supersampled_shutter_frames(math_mode, view, sampling, hip_lib):
    """set_supersample(2), and one adaptive case: the samples are the supersampled frames."""
    single = _singles(view, math_mode, sampling)[:2]
    got = _shutter(view, math_mode, 2, sampling)
    _assert_equal(got, {k: resolve([s[k] for s in single]) for k in ("bg", "disk")}, f"{math_mode} {view} {sampling}", ("bg", "disk"))
    plain = _singles(view, math_mode)[:2]
    assert any((s[k] != p[k]).any() for s, p in zip(single, plain) for k in ("bg", "disk"))      # supersampling changed the samples
    if sampling[1] is None:
        assert got["c"]["rays"] == 2 * 4 * VIEWS[view]["W"] * VIEWS[view]["H"]


def test_refusals_leave_the_context_usable(hip_lib):
    from bhr_amd import HipRenderer, _lib, scenes
    view, fov = "blocks", VIEWS["blocks"]["fov"]
    pos, toff = _samples(view, 2)
    r = _mk(view, "fast")
    r.render_shutter_async(pos, fov, toff)                      # a frame in flight on a slot
    cams = (_lib.Camera * 65)()
    for j in range(65):
        cams[j] = r.camera_uniforms(pos[j % 2], fov, t_offset=0.1 * j)
    before = r.counters()["frames_timed"]
    for args in ((None, cams, 2, 0), (r._ctx, None, 2, 0), (r._ctx, cams, 0, 0), (r._ctx, cams, -3, 0), (r._ctx, cams, 65, 0),
                 (r._ctx, cams, 2, _lib.PERSISTENT), (r._ctx, cams, 2, _lib.ROW_COSTS)):
        assert hip_lib.bhr_render_shutter(*args) == _lib.BHR_ERR_INVALID, args[2:]
        assert b"bhr_render_shutter" in hip_lib.bhr_last_error()
    for bad in (dict(cam_positions=[], t_offsets=[]), dict(cam_positions=pos, t_offsets=toff[:1])):
        with pytest.raises(ValueError):
            r.render_shutter_async(fov=fov, **bad)
    assert r.counters()["frames_timed"] == before               # nothing was launched
    block = HipRenderer(VIEWS[view]["W"], VIEWS[view]["H"], scenes.analytic_skybox(), scenes.noisy_disk(), math="fast", rows=(8, 16))
    assert hip_lib.bhr_render_shutter(block._ctx, cams, 2, 0) == _lib.BHR_ERR_INVALID
    assert b"whole-frame" in hip_lib.bhr_last_error()
    block.close()
    fresh = _mk(view, "fast")
    want = fresh.render(pos[0], fov)
    fresh.close()
    np.testing.assert_array_equal(r.render(pos[0], fov), want)
    r.close()


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_video_with_a_shutter(tmp_path, hip_lib):
    """render_video(shutter=0.5, shutter_samples=4): every frame file is the u8 frame of render_shutter with shutter_times'
    cameras on a context driven through the same lifecycle steps; shutter=0 leaves the files and the record as they were."""
    from bhr_amd import drivers
    from bhr_amd.camera import orbit_position
    W, H, N, S, NS_ = 64, 36, 3, 0.5, 4
    cam0, fov, speed, deg = [6, 0, 0.5], 90, 0.1, 90.0

    def video(out, **kw):
        r, _, _, _ = drivers.make_renderer(W, H, cam0, fov, n_stars=50, tex_w=256, tex_h=128)
        drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=out, fov=fov, static_cam_pos=cam0, orbit=True,
                             disk_rotation_speed=speed, orbit_degrees=deg, video_stream="off", assemble=False, **kw)
        r.close()
        return drivers._frames_dir(out)

    d = video(str(tmp_path / "blur" / "v.mp4"), shutter=S, shutter_samples=NS_)
    prog = json.load(open(os.path.join(d, "progress.json")))
    assert prog["params"] == {"n_frames": N, "fov": fov, "orbit": True, "disk_rotation_speed": speed, "orbit_degrees": deg,
                              "shutter": S, "shutter_samples": NS_}
    assert sorted(prog["completed"]) == list(range(N))

    r, _, _, _ = drivers.make_renderer(W, H, cam0, fov, n_stars=50, tex_w=256, tex_h=128)
    r.set_outputs("u8")
    factories = drivers.init_lifecycle_system(r, r.dtex_h, r.dtex_w, seed=42)
    frames = []
    for f in range(N):
        drivers.advance_lifecycle_frame(r, factories, f * speed, speed, recompute_stats=(f % 60 == 0), compose=True)
        u = drivers.shutter_times(f, S, NS_)
        r.render_shutter_async([orbit_position(cam0, t, N, deg) for t in u], fov, [(t - f) * speed for t in u])
        frames.append(r.read_final_u8())
    r.close()
    for f in range(N):
        np.testing.assert_array_equal(_png(os.path.join(d, f"frame_{f:04d}.png")), frames[f], err_msg=f"frame {f}")
    assert (frames[0] != frames[N - 1]).any()

    d0 = video(str(tmp_path / "plain" / "v.mp4"))
    d1 = video(str(tmp_path / "closed" / "v.mp4"), shutter=0, shutter_samples=8)
    names = sorted(os.listdir(d0))
    assert names == sorted(os.listdir(d1)) == [f"frame_{f:04d}.png" for f in range(N)] + ["progress.json"]
    for name in names:
        assert open(os.path.join(d0, name), "rb").read() == open(os.path.join(d1, name), "rb").read(), name
    assert (_png(os.path.join(d0, "frame_0001.png")) != frames[1]).any()                  # the shutter changed the frame
