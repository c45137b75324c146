"""Light delay on the device (bhr_render_delayed; csrc/ray_delay.h) against the context's own strict frame at scale 0, against its
CPU reference tests/delay_ref.py in binary64, under supersampling, with frames in flight, through the stages downstream of the
march, in a video, and its refusals and resources.

Bars.  The device evaluates the reference's float32 operations in their order, so per layer and channel it is allowed twice the
distance the float32 run of delay_ref keeps from its binary64 run on the same case, and never less than the project's 1e-4
(DESIGN.md 2); at most 0.5 % of the pixels may be off by more than 1e-3 in any channel (tests/test_delay_ref.py shows the float32
reference itself under that cap on every case), and the step total stays within 2e-4 of the float32 reference's."""
import os

import numpy as np
import pytest

import delay_cases as DC
from supersample_ref import box_resolve

pytestmark = pytest.mark.gpu

KW = dict(step_size=DC.STEP, r_max=DC.R_MAX, r_disk_inner=DC.R_INNER, r_disk_outer=DC.R_OUTER, anti_alias="disabled",
          disk_rotation_speed=DC.ROTATION_SPEED)
BAR_FLOOR = 1e-4
OFF_SHARE = 0.005
STEPS_RTOL = 2e-4
VIEWS2 = DC.VIEWS[:2]


def _mk(width=DC.W, height=DC.H, tilt=0.0, math="strict", texture="smooth", **kw):
    from bhr_amd import HipRenderer
    sky, tex = DC.scene(texture)
    return HipRenderer(width, height, sky, tex, math=math, disk_tilt=tilt, **{**KW, **kw})


def _read(r):
    from bhr_amd import _lib
    return dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), final=r.read_layer(_lib.LAYER_FINAL),
                steps=r.counters()["ray_steps"])


def _delayed(r, view, scale, frame=0, **kw):
    r.render_async(list(view), DC.FOV, frame=frame, light_delay=scale, **kw)
    return _read(r)


# ---- 1. scale 0 is the strict frame ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("supersample", (1, 2))
@pytest.mark.parametrize("tilt", DC.TILTS)
@pytest.mark.parametrize("size", ((96, 64), (61, 43), (5, 3)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_scale_zero_is_the_strict_frame(size, tilt, supersample, hip_lib):
    r = _mk(*size, tilt=tilt, supersample=supersample, texture="noisy")
    try:
        for view in VIEWS2:
            for frame in (0, 73):
                r.render_async(list(view), DC.FOV, frame=frame, math="strict")
                want = _read(r)
                got = _delayed(r, view, 0.0, frame)
                for layer in ("bg", "disk", "final"):
                    assert np.array_equal(got[layer], want[layer]), f"{layer} at {view}, frame {frame}: {int((got[layer] != want[layer]).any(axis=2).sum())} pixels differ"
                assert got["steps"] == want["steps"] > 0
            assert r.counters()["rays"] == supersample * supersample * size[0] * size[1]
    finally:
        r.close()


# ---- 2. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", DC.CASES, ids=lambda c: c.name)
def test_device_against_delay_ref_float64(case, hip_lib):
    r64, r32 = DC.reference(case, np.float64), DC.reference(case, np.float32)
    r = _mk(tilt=case.tilt, texture=case.texture)
    try:
        got = _delayed(r, case.view, case.scale, case.frame, skip_bloom=True)
    finally:
        r.close()
    for layer in ("bg", "disk"):
        d32, d = DC.rmse(r32[layer], r64[layer]), DC.rmse(got[layer], r64[layer])
        bar = np.maximum(2.0 * d32, BAR_FLOOR)
        print(f"[delay] {case.name} {layer}: device {d} from binary64, the float32 reference {d32}, bar {bar}")
        assert (d <= bar).all(), (case.name, layer, d, bar)
    share = DC.off_share((got["bg"], got["disk"]), (r64["bg"], r64["disk"]))
    steps32 = int(r32["steps"].sum())
    print(f"[delay] {case.name}: {share:.5f} of the pixels off by more than 1e-3; ray_steps {got['steps']} (float32 reference {steps32}, "
          f"binary64 {int(r64['steps'].sum())}); device equals the float32 reference in {float((got['disk'] == r32['disk']).all(axis=2).mean()):.4f} of DISK")
    assert share <= OFF_SHARE
    assert abs(got["steps"] - steps32) <= STEPS_RTOL * steps32
    assert np.isfinite(got["bg"]).all() and np.isfinite(got["disk"]).all()


# ---- 3. the delay shows and touches nothing else ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tilt", DC.TILTS)
def test_the_delay_shows_in_the_disk_alone(tilt, hip_lib):
    """Scale 1 against scale 0: the same steps, another DISK.  BG is the sky through 1 - alpha of the ray's crossings, and the
    texture's alpha is sampled under the delayed roll like its colour: BG is the same bits wherever the ray crosses no disk, and with
    the smooth texture, whose alpha does not depend on phi, within the bilinear sampler's rounding elsewhere (delay_cases.BG_ROUNDING
    derives the bound; bit-for-bit equality there is not the sampler's to give: its four weights do not sum to 1 exactly).  With
    the noisy texture BG moves where the disk is crossed, and nowhere else."""
    r, noisy = _mk(tilt=tilt), _mk(tilt=tilt, texture="noisy")
    try:
        for view in VIEWS2:
            off, on, more = (_delayed(r, view, s, 73, skip_bloom=True) for s in (0.0, 1.0, 2.5))
            assert off["steps"] == on["steps"] == more["steps"] > 0
            clear = (off["disk"] == 0).all(axis=2)
            assert clear.any() and not clear.all()
            for f in (on, more):
                assert np.array_equal(f["bg"][clear], off["bg"][clear]) and np.array_equal(f["disk"][clear], off["disk"][clear])
                d_bg = float(np.abs(f["bg"].astype(np.float64) - off["bg"]).max())
                print(f"[delay] tilt {tilt} view {view}: BG moves by {d_bg:.3e} at most (bound {DC.BG_ROUNDING}), DISK by {float(np.abs(f['disk'] - off['disk']).max()):.3f}")
                assert d_bg <= DC.BG_ROUNDING
                assert np.array_equal(f["bg"] == 0, off["bg"] == 0)
            assert (on["disk"] != off["disk"]).any(axis=2).mean() > 0.05 and np.abs(on["disk"] - off["disk"]).max() > 0.02
            assert (more["disk"] != on["disk"]).any(axis=2).mean() > 0.05
            n_off, n_on = _delayed(noisy, view, 0.0, 73, skip_bloom=True), _delayed(noisy, view, 1.0, 73, skip_bloom=True)
            crossed = (n_off["disk"] != 0).any(axis=2) | (n_on["disk"] != 0).any(axis=2)
            assert n_off["steps"] == n_on["steps"] and np.array_equal(n_on["bg"][~crossed], n_off["bg"][~crossed])
            assert (n_on["disk"] != n_off["disk"]).any()
    finally:
        r.close()
        noisy.close()


# ---- 4. supersampling -------------------------------------------------------------------------------------------------------------
def test_supersampled_frame_is_the_box_filter_of_the_fine_frame(hip_lib):
    """bhr_set_supersample's contract: the k = 2 frame of 48 x 32 is, bit for bit, the pairwise-tree box filter of the 96 x 64
    frame of the same view and scale (a context has one frame size, so the fine frame comes from a second context)."""
    ss, fine = _mk(DC.W // 2, DC.H // 2, tilt=25.0, supersample=2), _mk(DC.W, DC.H, tilt=25.0)
    try:
        a, b = _delayed(ss, DC.VIEWS[1], 1.0, 73, skip_bloom=True), _delayed(fine, DC.VIEWS[1], 1.0, 73, skip_bloom=True)
        for layer in ("bg", "disk"):
            want = box_resolve(b[layer], 2)
            assert np.array_equal(a[layer], want), f"{layer}: {int((a[layer] != want).any(axis=2).sum())} pixels are not the box filter of the fine frame"
        assert a["steps"] == b["steps"] and ss.counters()["rays"] == DC.W * DC.H
        assert a["disk"].max() > 0 and a["bg"].max() > 0
    finally:
        ss.close()
        fine.close()


# ---- 5. frames in flight ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ("strict", "hybrid"))
def test_frames_in_flight_keep_their_own_scale(math, hip_lib):
    """The scale travels with the call: four frames queued without a sync alternate two (scale, t_offset) pairs, and each is the
    frame of the same call made alone (the post-pass follows the context's arithmetic, so the whole frame is compared)."""
    pairs = ((1.0, 0), (2.5, 73), (1.0, 0), (2.5, 73))
    one, two = _mk(math=math, frame_slots=1), _mk(math=math, frame_slots=2)
    try:
        assert two.frame_slots == 2
        want = [_delayed(one, DC.VIEWS[0], s, f) for s, f in pairs[:2]]
        assert not np.array_equal(want[0]["disk"], want[1]["disk"])
        for last in range(len(pairs)):
            for k in range(last + 1):
                two.render_async(list(DC.VIEWS[0]), DC.FOV, frame=pairs[k][1], light_delay=pairs[k][0])
            got = _read(two)
            for layer in ("bg", "disk", "final"):
                assert np.array_equal(got[layer], want[last % 2][layer]), f"frame {last} {layer}"
            assert got["steps"] == want[last % 2]["steps"]
    finally:
        one.close()
        two.close()


# ---- 6. downstream of the march -----------------------------------------------------------------------------------------------------
def test_post_pass_flare_grade_and_rows_run_on_the_delayed_layers(hip_lib):
    from bhr_amd import _lib
    r, plain = _mk(), _mk()
    try:
        got = _delayed(r, DC.VIEWS[0], 1.0, 73)
        plain.write_layer(_lib.LAYER_BG, got["bg"])
        plain.write_layer(_lib.LAYER_DISK, got["disk"])
        plain.bloom_only()
        assert np.array_equal(plain.read_layer(_lib.LAYER_FINAL), got["final"])
        assert not np.array_equal(got["final"], _delayed(r, DC.VIEWS[0], 0.0, 73)["final"])
        r.set_grade(tonemap="aces", exposure=-0.5, transfer="srgb", keep_hdr=True)
        flared = _delayed(r, DC.VIEWS[0], 1.0, 73, lens_flare=True)
        u8, hdr = r.read_final_u8(), r.read_hdr()
        assert np.isfinite(flared["final"]).all() and np.isfinite(hdr).all() and flared["final"].max() > 0
        assert u8.shape == (DC.H, DC.W, 3) and u8.dtype == np.uint8 and u8.max() > 0
        assert not np.array_equal(flared["final"], got["final"])
    finally:
        r.close()
        plain.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(r, hip_lib, word, scale=1.0, reserved=0, flags=0):
    import ctypes as C
    from bhr_amd import _lib
    cam = r.camera_uniforms(list(DC.VIEWS[0]), DC.FOV)
    d = _lib.LightDelay(scale, reserved)
    before = r.counters()
    assert hip_lib.bhr_render_delayed(r._ctx, C.byref(cam), C.byref(d), flags) == _lib.BHR_ERR_INVALID
    msg = hip_lib.bhr_last_error().decode()
    assert "bhr_render_delayed" in msg and word in msg, msg
    after = r.counters()
    assert all(after[k] == before[k] for k in ("rays", "ray_steps", "frames_timed"))       # nothing was launched


def _renders_as_ever(r, want=None):
    r.render_async(list(DC.VIEWS[0]), DC.FOV, skip_bloom=True)
    got = _read(r)
    assert got["steps"] > 0 and got["final"].shape == (r.rows, r.width, 3)
    if want is not None:
        for layer in ("bg", "disk", "final"):
            assert np.array_equal(got[layer], want[layer]), layer
    return got


def test_refusals_name_the_combination_and_leave_the_context_alone(hip_lib):
    import ctypes as C
    from bhr_amd import _lib
    w, h = 32, 16
    r = _mk(w, h)
    try:
        want = _renders_as_ever(r)
        cam, d = r.camera_uniforms(list(DC.VIEWS[0]), DC.FOV), _lib.LightDelay(1.0, 0)
        for args in ((None, C.byref(cam), C.byref(d)), (r._ctx, None, C.byref(d)), (r._ctx, C.byref(cam), None)):
            assert hip_lib.bhr_render_delayed(*args, 0) == _lib.BHR_ERR_INVALID
            assert "null" in hip_lib.bhr_last_error().decode()
        _renders_as_ever(r, want)
        for scale in (float("nan"), -0.25, -0.0 - 1e-6, 16.5, float("inf")):
            _refused(r, hip_lib, "scale", scale=scale)
        _renders_as_ever(r, want)
        _refused(r, hip_lib, "reserved", reserved=1)
        _refused(r, hip_lib, "reserved", reserved=-7)
        _renders_as_ever(r, want)
        for flag in (_lib.SKIP_DIFFERENTIALS, _lib.PERSISTENT, _lib.FORCE_FAST, _lib.FORCE_STRICT, _lib.FORCE_HYBRID, 1 << 20):
            _refused(r, hip_lib, "flags", flags=flag)
        _renders_as_ever(r, want)
        with pytest.raises(ValueError, match="light_delay"):         # the Python layer checks the scale and the keywords itself
            r.render_async(list(DC.VIEWS[0]), DC.FOV, light_delay=17.0)
        with pytest.raises(ValueError, match="light_delay"):
            r.render_async(list(DC.VIEWS[0]), DC.FOV, light_delay=1.0, math="fast")
        with pytest.raises(ValueError, match="light_delay"):
            r.render_async(list(DC.VIEWS[0]), DC.FOV, light_delay=1.0, observer=(0.1, 0.0, 0.0))
        with pytest.raises(ValueError, match="light_delay"):
            r.render_async(list(DC.VIEWS[0]), DC.FOV, light_delay=1.0, projection="fisheye")
        r.set_supersample(2, 0.05)
        _refused(r, hip_lib, "adaptive supersampling")
        r.set_supersample(1)
        _renders_as_ever(r, want)
        r.set_spin(0.5)
        _refused(r, hip_lib, "spin")
        r.set_spin(0.0, force_kerr=True)
        _refused(r, hip_lib, "Kerr march forced")
        r.set_redshift("exact")
        _refused(r, hip_lib, "exact redshift")
        r.set_redshift("model")
        r.set_spin(0.0)
        _renders_as_ever(r, want)
        delayed = _delayed(r, DC.VIEWS[0], 1.0, skip_bloom=True)     # and the delayed frame itself still renders
        assert delayed["steps"] == want["steps"] and not np.array_equal(delayed["disk"], want["disk"])
        from bhr_amd.disk_v2 import DiskV2Params
        r.use_disk_v2(DiskV2Params())                            # (params=None would switch back to the texture)
        _refused(r, hip_lib, "Disk V2")
    finally:
        r.close()
    r = _mk(w, h)
    try:
        _renders_as_ever(r, want)                                # a context like the one the refusals met renders the frame it rendered before them
    finally:
        r.close()
    aa = _mk(w, h, anti_alias="lod_radius")
    try:
        before = _renders_as_ever(aa)
        _refused(aa, hip_lib, "anti_alias")
        _renders_as_ever(aa, before)
    finally:
        aa.close()
    block = _mk(w, h, rows=(0, 8))
    try:
        before = _renders_as_ever(block)
        _refused(block, hip_lib, "row-block")
        _renders_as_ever(block, before)
    finally:
        block.close()


# ---- 8. resources ---------------------------------------------------------------------------------------------------------------------
def test_resources(hip_lib):
    import ctypes as C
    from bhr_amd import _lib
    r = _mk(16, 8)
    try:
        for ss in (0, 1):
            out = (C.c_int32 * 3)()
            assert hip_lib.bhr_delayed_resources(ss, out) == _lib.BHR_OK
            vgprs, lds, scratch = (int(v) for v in out)
            print(f"[delay] march kernel (supersampled {ss}): {vgprs} VGPRs, {lds} bytes of LDS, {scratch} bytes of scratch")
            assert scratch == 0 and 0 < vgprs <= 128 and lds > 0
            assert r.delayed_resources(supersampled=bool(ss)) == dict(vgprs=vgprs, lds_bytes=lds, scratch_bytes=scratch)
    finally:
        r.close()
    assert hip_lib.bhr_delayed_resources(0, None) == _lib.BHR_ERR_INVALID


# ---- 9. video ---------------------------------------------------------------------------------------------------------------------------
def test_video_frames_are_the_frames_rendered_alone(tmp_path, hip_lib):
    """A 4-frame 48 x 32 render_video with light_delay = 1 and an orbit: the PNG files decode to read_final_u8 of the same frames
    rendered one by one; without the delay the loop writes other frames."""
    from PIL import Image
    from bhr_amd import drivers
    from bhr_amd.camera import orbit_position
    w, h, n, fov, pov = 48, 32, 4, 90, [6, 0, 0.5]
    mk = lambda slots: drivers.make_renderer(w, h, pov, fov, n_stars=600, tex_w=512, tex_h=256, frame_slots=slots, math="strict")[0]

    def alone(scale):
        r = mk(1)
        try:
            factories = drivers.init_lifecycle_system(r, r.dtex_h, r.dtex_w, seed=42)
            frames = []
            for f in range(n):
                drivers.advance_lifecycle_frame(r, factories, f * 0.1, 0.1, recompute_stats=(f % 60 == 0), compose=True)
                r.render(orbit_position(pov, f, n, 360.0), fov, frame=0, **({} if scale is None else {"light_delay": scale}))
                frames.append(r.read_final_u8())
            return frames
        finally:
            r.close()

    out = os.path.join(str(tmp_path), "delayed", "v.mp4")
    r = mk(2)
    try:
        drivers.render_video(r, w, h, n_frames=n, fps=12, output_path=out, fov=fov, static_cam_pos=pov, orbit=True, assemble=False,
                             video_stream="off", light_delay=1.0)
    finally:
        r.close()
    want = alone(1.0)
    frames = [np.asarray(Image.open(os.path.join(drivers._frames_dir(out), f"frame_{f:04d}.png")).convert("RGB")) for f in range(n)]
    for f in range(n):
        assert frames[f].shape == (h, w, 3)
        assert np.array_equal(frames[f], want[f]), f"frame {f}: {int((frames[f] != want[f]).any(axis=2).sum())} pixels differ"
    assert frames[0].max() > 100 and (frames[0] != frames[-1]).mean() > 0.01       # the frames are real and the camera moves
    undelayed = alone(None)
    assert (undelayed[-1] != want[-1]).any()                               # the delay is in the files
    import json
    with open(os.path.join(drivers._frames_dir(out), "progress.json")) as fh:
        assert json.load(fh)["params"]["light_delay"] == 1.0
