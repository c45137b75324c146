"""The moving observer on the device (bhr_render_observer; csrc/ray_observer.h) against the context's own strict frame at rest,
against its CPU reference tests/observer_ref.py in binary64, under supersampling, with frames in flight, through the stages
downstream of the march, and its refusals and resources.

Bars.  The device evaluates the reference's float32 operations in their order, so per layer and channel it is allowed twice the
distance the float32 run of observer_ref keeps from its binary64 run on the same case, and never less than the project's 1e-4
(DESIGN.md 2); at most 0.5 % of the pixels may be off by more than 1e-3 in any channel (tests/test_observer_ref.py shows the
float32 reference itself under that cap on every case), and the step total stays within 2e-4 of the float32 reference's."""
import numpy as np
import pytest

import observer_cases as OC
from supersample_ref import box_resolve

pytestmark = pytest.mark.gpu

KW = dict(step_size=OC.STEP, r_max=OC.R_MAX, r_disk_inner=OC.R_INNER, r_disk_outer=OC.R_OUTER, anti_alias="disabled")
BAR_FLOOR = 1e-4
OFF_SHARE = 0.005
STEPS_RTOL = 2e-4
MOVING = (0.3, -0.4, 0.5)


def _mk(width=OC.W, height=OC.H, tilt=0.0, math="strict", sky_gain=1.0, **kw):
    from bhr_amd import HipRenderer
    sky, tex = OC.scene()
    return HipRenderer(width, height, sky * np.float32(sky_gain), tex, math=math, disk_tilt=tilt, **{**KW, **kw})


def _read(r):
    from bhr_amd import _lib
    return dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), final=r.read_layer(_lib.LAYER_FINAL),
                steps=r.counters()["ray_steps"])


def _observer(r, view, beta, sky=True, **kw):
    r.render_async(list(view), OC.FOV, observer=beta, observer_sky=sky, **kw)
    return _read(r)


# ---- 1. at rest the frame is the strict march's --------------------------------------------------------------------------------
@pytest.mark.parametrize("supersample", (1, 2))
@pytest.mark.parametrize("tilt", OC.TILTS)
@pytest.mark.parametrize("size", ((96, 64), (61, 43), (5, 3)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_at_rest(size, tilt, supersample, hip_lib):
    r = _mk(*size, tilt=tilt, supersample=supersample)
    try:
        for view in OC.VIEWS:
            r.render_async(list(view), OC.FOV, math="strict")
            want = _read(r)
            for sky in (True, False):
                got = _observer(r, view, (0.0, 0.0, 0.0), sky)
                for layer in ("bg", "disk", "final"):
                    assert np.array_equal(got[layer], want[layer]), f"{layer} at {view}, sky_shift {sky}: {int((got[layer] != want[layer]).any(axis=2).sum())} pixels differ"
                assert got["steps"] == want["steps"] > 0
            assert r.counters()["rays"] == supersample * supersample * size[0] * size[1]
    finally:
        r.close()


# ---- 2. against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OC.CASES, ids=lambda c: c.name)
def test_device_against_observer_ref_float64(case, hip_lib):
    r64, r32 = OC.reference(case, np.float64), OC.reference(case, np.float32)
    r = _mk(tilt=case.tilt)
    try:
        got = _observer(r, case.view, case.beta, case.sky, skip_bloom=True)
    finally:
        r.close()
    for layer in ("bg", "disk"):
        d32, d = OC.rmse(r32[layer], r64[layer]), OC.rmse(got[layer], r64[layer])
        bar = np.maximum(2.0 * d32, BAR_FLOOR)
        print(f"[observer] {case.name} {layer}: device {d} from binary64, the float32 reference {d32}, bar {bar}")
        assert (d <= bar).all(), (case.name, layer, d, bar)
    share = OC.off_share((got["bg"], got["disk"]), (r64["bg"], r64["disk"]))
    steps32 = int(r32["steps"].sum())
    print(f"[observer] {case.name}: {share:.5f} of the pixels off by more than 1e-3; ray_steps {got['steps']} (float32 reference {steps32}, "
          f"binary64 {int(r64['steps'].sum())}); BG reaches {float(got['bg'].max()):.3f}")
    assert share <= OFF_SHARE
    assert abs(got["steps"] - steps32) <= STEPS_RTOL * steps32
    assert np.isfinite(got["bg"]).all() and np.isfinite(got["disk"]).all()


def test_motion_shows(hip_lib):
    """Aberration moves the picture and the Doppler factor changes its brightness: the frame of a moving camera is not the
    frame at rest, the plain sky differs from the shifted one in BG alone, and BG goes above 1 ahead of a fast camera (under
    a sky twice as bright as the tests' own, whose samples the factor of at most 1.5^1.5 leaves under 1)."""
    r = _mk(sky_gain=2.0)
    try:
        view = OC.VIEWS[0]
        rest = _observer(r, view, (0.0, 0.0, 0.0), skip_bloom=True)
        fwd = OC.CASES[3]
        shifted, plain = _observer(r, view, fwd.beta, True, skip_bloom=True), _observer(r, view, fwd.beta, False, skip_bloom=True)
        assert (shifted["bg"] != rest["bg"]).mean() > 0.2 and (shifted["disk"] != rest["disk"]).any()
        assert np.array_equal(shifted["disk"], plain["disk"]) and shifted["steps"] == plain["steps"]
        assert shifted["bg"].max() > 1.0 and shifted["final"].max() <= 1.0
        assert (shifted["bg"][..., 1] > 1.5 * plain["bg"][..., 1]).any()                # I = Ds^1.5 reaches 1.84 dead ahead
        # flying at the hole squeezes its image towards the centre of the frame: the shadow covers fewer pixels
        dark = lambda f: int(((f["bg"].max(axis=2) == 0) & (f["disk"].max(axis=2) == 0)).sum())
        assert dark(plain) < dark(rest)
    finally:
        r.close()


# ---- 3. supersampling ------------------------------------------------------------------------------------------------------------
def test_supersampled_frame_is_the_box_filter_of_the_fine_frame(hip_lib):
    """bhr_set_supersample's contract: the k = 2 frame of 48 x 32 is, bit for bit, the pairwise-tree box filter of the 96 x 64
    frame of the same view and velocity (a context has one frame size, so the fine frame comes from a second context)."""
    ss, fine = _mk(OC.W // 2, OC.H // 2, tilt=25.0, supersample=2), _mk(OC.W, OC.H, tilt=25.0)
    try:
        a, b = _observer(ss, OC.VIEWS[1], MOVING, skip_bloom=True), _observer(fine, OC.VIEWS[1], MOVING, skip_bloom=True)
        for layer in ("bg", "disk"):
            want = box_resolve(b[layer], 2)
            assert np.array_equal(a[layer], want), f"{layer}: {int((a[layer] != want).any(axis=2).sum())} pixels are not the box filter of the fine frame"
        assert a["steps"] == b["steps"] and ss.counters()["rays"] == OC.W * OC.H
        assert a["disk"].max() > 0 and a["bg"].max() > 0
    finally:
        ss.close()
        fine.close()


# ---- 4. two frames in flight ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ("strict", "hybrid"))
def test_frames_in_flight_keep_their_own_velocity(math, hip_lib):
    """The velocity travels with the call: four frames queued without a sync alternate two velocities, and each is the frame of
    the same call made alone (the post-pass follows the context's arithmetic, so the whole frame is compared)."""
    betas = (OC.CASES[0].beta, MOVING, OC.CASES[0].beta, MOVING)
    one, two = _mk(math=math, frame_slots=1), _mk(math=math, frame_slots=2)
    try:
        assert two.frame_slots == 2
        want = [_observer(one, OC.VIEWS[0], b) for b in betas[:2]]
        assert not np.array_equal(want[0]["bg"], want[1]["bg"])
        for last in range(len(betas)):
            for k in range(last + 1):
                two.render_async(list(OC.VIEWS[0]), OC.FOV, observer=betas[k])
            got = _read(two)
            for layer in ("bg", "disk", "final"):
                assert np.array_equal(got[layer], want[last % 2][layer]), f"frame {last} {layer}"
            assert got["steps"] == want[last % 2]["steps"]
    finally:
        one.close()
        two.close()


# ---- 5. downstream of the march ---------------------------------------------------------------------------------------------------
def _inject(r, layers):
    from bhr_amd import _lib
    r.write_layer(_lib.LAYER_BG, layers["bg"])
    r.write_layer(_lib.LAYER_DISK, layers["disk"])


def test_graded_and_flared_frames_are_the_stages_on_the_observers_layers(hip_lib):
    from bhr_amd import _lib
    fwd = OC.CASES[3]                                   # BG above 1: the grade and the HDR plane see the headroom
    grade = dict(tonemap="aces", exposure=-0.5, transfer="srgb", keep_hdr=True)
    r, plain = _mk(sky_gain=2.0), _mk(sky_gain=2.0)
    try:
        r.set_grade(**grade)
        graded = _observer(r, fwd.view, fwd.beta)
        hdr = r.read_hdr()
        assert graded["bg"].max() > 1.0 and hdr.max() > 1.0
        _inject(plain, graded)
        plain.bloom_only()
        plain.set_grade(**grade)
        plain.grade_frame()
        assert np.array_equal(plain.read_layer(_lib.LAYER_FINAL), graded["final"])
        assert np.array_equal(plain.read_hdr(), hdr)
        assert np.array_equal(plain.read_final_u8(), r.read_final_u8())
        plain.set_grade(None)
        r.set_grade(None)
        flared = _observer(r, fwd.view, fwd.beta, lens_flare=True)
        _inject(plain, flared)
        plain.bloom_only()
        unflared = plain.read_layer(_lib.LAYER_FINAL)
        plain.apply_lens_flare()
        assert np.array_equal(plain.read_layer(_lib.LAYER_FINAL), flared["final"])
        assert not np.array_equal(unflared, flared["final"])
    finally:
        r.close()
        plain.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def _refused(r, hip_lib, word, beta=(0.1, 0.0, 0.0), flags=0):
    import ctypes as C
    from bhr_amd import _lib
    cam = r.camera_uniforms(list(OC.VIEWS[0]), OC.FOV)
    obs = _lib.Observer()
    obs.beta[:] = beta
    obs.sky_shift = 1
    before = r.counters()
    assert hip_lib.bhr_render_observer(r._ctx, C.byref(cam), C.byref(obs), flags) == _lib.BHR_ERR_INVALID
    msg = hip_lib.bhr_last_error().decode()
    assert "bhr_render_observer" in msg and word in msg, msg
    after = r.counters()
    assert all(after[k] == before[k] for k in ("rays", "ray_steps", "frames_timed"))       # nothing was launched


def _renders_as_ever(r, want=None):
    r.render_async(list(OC.VIEWS[0]), OC.FOV, skip_bloom=True)
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
        cam, obs = r.camera_uniforms(list(OC.VIEWS[0]), OC.FOV), _lib.Observer()
        for args in ((None, C.byref(cam), C.byref(obs)), (r._ctx, None, C.byref(obs)), (r._ctx, C.byref(cam), None)):
            assert hip_lib.bhr_render_observer(*args, 0) == _lib.BHR_ERR_INVALID
            assert "null" in hip_lib.bhr_last_error().decode()
        for beta in ((0.996, 0.0, 0.0), (0.7, 0.7, 0.2), (float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0)):
            _refused(r, hip_lib, "0.995", beta=beta)
        for flag in (_lib.SKIP_DIFFERENTIALS, _lib.PERSISTENT, _lib.FORCE_FAST, _lib.FORCE_STRICT, _lib.FORCE_HYBRID, 1 << 20):
            _refused(r, hip_lib, "flags", flags=flag)
        with pytest.raises(ValueError):                          # the Python layer checks the velocity itself
            r.render_async(list(OC.VIEWS[0]), OC.FOV, observer=(1.0, 0.0, 0.0))
        with pytest.raises(ValueError, match="flags"):
            r.render_async(list(OC.VIEWS[0]), OC.FOV, observer=(0.1, 0.0, 0.0), math="fast")
        r.set_supersample(2, 0.05)
        _refused(r, hip_lib, "adaptive supersampling")
        r.set_supersample(1)
        r.set_spin(0.5)
        _refused(r, hip_lib, "spin")
        r.set_spin(0.0, force_kerr=True)
        _refused(r, hip_lib, "spin")
        r.set_redshift("exact")
        _refused(r, hip_lib, "exact redshift")
        r.set_redshift("model")
        r.set_spin(0.0)
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
        _refused(aa, hip_lib, "anti_alias")
        _renders_as_ever(aa)
    finally:
        aa.close()
    block = _mk(w, h, rows=(0, 8))
    try:
        _refused(block, hip_lib, "row-block")
        _renders_as_ever(block)
    finally:
        block.close()


def test_refused_calls_do_not_disturb_the_next_frames(hip_lib):
    """After each kind of refusal on one context, the ordinary frame and the observer frame are what they were."""
    r = _mk(32, 16)
    try:
        want, want_obs = _renders_as_ever(r), _observer(r, OC.VIEWS[0], MOVING, skip_bloom=True)
        _refused(r, hip_lib, "0.995", beta=(0.0, 0.0, 0.999))
        _refused(r, hip_lib, "flags", flags=4096)
        r.set_spin(0.3)
        _refused(r, hip_lib, "spin")
        r.set_spin(0.0)
        _renders_as_ever(r, want)
        got = _observer(r, OC.VIEWS[0], MOVING, skip_bloom=True)
        for layer in ("bg", "disk", "final"):
            assert np.array_equal(got[layer], want_obs[layer]), layer
    finally:
        r.close()


# ---- 7. resources ------------------------------------------------------------------------------------------------------------------
def test_resources(hip_lib):
    import ctypes as C
    from bhr_amd import _lib
    for ss in (0, 1):
        out = (C.c_int32 * 3)()
        assert hip_lib.bhr_observer_resources(ss, out) == _lib.BHR_OK
        vgprs, lds, scratch = (int(v) for v in out)
        print(f"[observer] march kernel (supersampled {ss}): {vgprs} VGPRs, {lds} bytes of LDS, {scratch} bytes of scratch")
        assert scratch == 0 and 0 < vgprs <= 128 and lds > 0
    assert hip_lib.bhr_observer_resources(0, None) == _lib.BHR_ERR_INVALID
