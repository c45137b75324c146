"""The projections on the device (bhr_render_projected; csrc/ray_projected.h) against their CPU reference tests/projection_ref.py in
binary64, against a sky whose colour is its direction, at rest with and without an observer block, under supersampling, with
frames in flight, through the stages downstream of the march, and their refusals and resources.

Bars: tests/test_gpu_observer.py's, as they are.  The device evaluates the reference's float32 operations in their order (sinf
and cosf apart, whose bits are not pinned), so per layer and channel it is allowed twice the distance the float32 run of
projection_ref keeps from its binary64 run on the same case, and never less than the project's 1e-4; at most 0.5 % of the pixels
may be off by more than 1e-3 in any channel (tests/test_projection_ref.py shows the float32 reference itself under that cap on
every case), and the step total stays within 2e-4 of the float32 reference's.  The fisheye's mask is IEEE arithmetic only: the
device's blank pixels contain the float32 reference's mask exactly."""
import ctypes as C

import numpy as np
import pytest

import projection_cases as PC
import projection_ref as P
from supersample_ref import box_resolve

pytestmark = pytest.mark.gpu

KW = dict(step_size=PC.STEP, r_max=PC.R_MAX, r_disk_inner=PC.R_INNER, r_disk_outer=PC.R_OUTER, anti_alias="disabled")
BAR_FLOOR = 1e-4
OFF_SHARE = 0.005
STEPS_RTOL = 2e-4
MOVING = (0.3, -0.4, 0.5)
EQ, FISH = ("equirect", (360.0, 180.0)), ("fisheye", (180.0,))


def _mk(width, height, tilt=0.0, math="strict", sky=None, **kw):
    from bhr_amd import HipRenderer
    s, tex = PC.scene()
    return HipRenderer(width, height, s if sky is None else sky, tex, math=math, disk_tilt=tilt, **{**KW, **kw})


def _read(r):
    from bhr_amd import _lib
    return dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), final=r.read_layer(_lib.LAYER_FINAL),
                steps=r.counters()["ray_steps"])


def _projected(r, view, proj, beta=None, sky=True, **kw):
    r.render_async(list(view), None, projection=proj[0], projection_fov=proj[1], **({} if beta is None else {"observer": beta, "observer_sky": sky}), **kw)
    return _read(r)


def _same(got, want, what, layers=("bg", "disk", "final")):
    for layer in layers:
        assert np.array_equal(got[layer], want[layer]), f"{what} {layer}: {int((got[layer] != want[layer]).any(axis=2).sum())} pixels differ"
    assert got["steps"] == want["steps"], what


# ---- 1. against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.name)
def test_device_against_projection_ref_float64(case, hip_lib):
    r64, r32 = PC.reference(case, np.float64), PC.reference(case, np.float32)
    r = _mk(*case.size, tilt=case.tilt)
    try:
        got = _projected(r, case.view, (case.kind, case.fov), case.beta, case.sky, skip_bloom=True)
        rays = r.counters()["rays"]
    finally:
        r.close()
    for layer in ("bg", "disk"):
        d32, d = PC.rmse(r32[layer], r64[layer]), PC.rmse(got[layer], r64[layer])
        bar = np.maximum(2.0 * d32, BAR_FLOOR)
        print(f"[projection] {case.name} {layer}: device {d} from binary64, the float32 reference {d32}, bar {bar}")
        assert (d <= bar).all(), (case.name, layer, d, bar)
    share = PC.off_share((got["bg"], got["disk"]), (r64["bg"], r64["disk"]))
    steps32 = int(r32["steps"].sum())
    print(f"[projection] {case.name}: {share:.5f} of the pixels off by more than 1e-3; ray_steps {got['steps']} (float32 reference {steps32}, "
          f"binary64 {int(r64['steps'].sum())}); {int((~r32['inside']).sum())} pixels outside the image circle")
    assert share <= OFF_SHARE
    assert abs(got["steps"] - steps32) <= STEPS_RTOL * steps32
    assert np.isfinite(got["bg"]).all() and np.isfinite(got["disk"]).all()
    assert rays == case.size[0] * case.size[1]
    if case.kind == P.FISHEYE:
        outside = ~r32["inside"]
        assert outside.any() and np.array_equal(r32["inside"], r64["inside"])
        blank = (got["bg"] == 0).all(axis=2) & (got["disk"] == 0).all(axis=2)
        assert blank[outside].all(), f"{int((~blank[outside]).sum())} pixels outside the image circle are not exactly 0"


# ---- 2. orientation, from the sky sampler's convention alone ----------------------------------------------------------------------
def _direction_sky(h=256, w=512):
    """A sky whose colour is 0.5 + 0.4 (x, y, z) of the texel's own direction: texel (v, u) is sampled at theta = acos z =
    pi v / h and phi = atan2(y, x) = 2 pi u / w."""
    theta = (np.pi * np.arange(h) / h)[:, None]
    phi = (2.0 * np.pi * np.arange(w) / w)[None, :]
    d = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta) * np.ones_like(phi)], axis=-1)
    return (0.5 + 0.4 * d).astype(np.float32)


@pytest.mark.parametrize("proj,size", ((("equirect", (360.0, 180.0)), (32, 16)), (("fisheye", (360.0,)), (32, 32))), ids=("equirect", "fisheye360"))
def test_pixels_look_where_the_formulas_say(proj, size, hip_lib):
    """Away from the hole the sky is seen almost undeflected: from r0 = 40 an outward ray bends by at most r_s / r0 = 0.025 rad,
    the ramp's slope is at most 0.4 per radian (0.01), the rest of the 0.03 is texel interpolation.  A mirrored or swapped axis
    misses by tenths."""
    pos = (40.0, 0.0, 5.0)
    r = _mk(*size, sky=_direction_sky())
    try:
        got = _projected(r, pos, proj, skip_bloom=True)
    finally:
        r.close()
    n, inside = P.directions(PC.camera(pos, *size), proj[0], proj[1])
    away = inside & ((n @ np.array(pos)) > 0)
    assert away.sum() > 0.3 * size[0] * size[1]
    err = np.abs(got["bg"].astype(np.float64) - (0.5 + 0.4 * n))[away]
    print(f"[projection] orientation {proj[0]}: {int(away.sum())} pixels look away from the hole, largest |BG - ramp| {err.max():.4f}")
    assert err.max() <= 0.03


# ---- 3. no observer block is the observer at rest ----------------------------------------------------------------------------------
@pytest.mark.parametrize("proj", (EQ, FISH), ids=("equirect", "fisheye"))
@pytest.mark.parametrize("size", ((96, 48), (61, 43), (5, 3), (1, 1)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_null_observer_is_the_observer_at_rest(size, proj, hip_lib):
    r = _mk(*size)
    try:
        for view in (PC.V0, PC.V1):
            want = _projected(r, view, proj)
            assert want["steps"] > 0
            for sky in (False, True):
                _same(_projected(r, view, proj, (0.0, 0.0, 0.0), sky), want, f"{view} sky_shift {sky}")
            assert r.counters()["rays"] == size[0] * size[1]
    finally:
        r.close()


# ---- 4. supersampling --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proj,size", ((EQ, (48, 24)), (("fisheye", (180.0,)), (32, 32))), ids=("equirect", "fisheye"))
def test_supersampled_frame_is_the_box_filter_of_the_fine_frame(proj, size, hip_lib):
    """bhr_set_supersample's contract: the k = 2 frame is, bit for bit, the pairwise-tree box filter of the frame of twice the
    size of the same call; the fisheye's blank pixels enter it as zeros."""
    w, h = size
    ss, fine = _mk(w, h, tilt=25.0, supersample=2), _mk(2 * w, 2 * h, tilt=25.0)
    try:
        a, b = _projected(ss, PC.V1, proj, MOVING, skip_bloom=True), _projected(fine, PC.V1, proj, MOVING, skip_bloom=True)
        for layer in ("bg", "disk"):
            want = box_resolve(b[layer], 2)
            assert np.array_equal(a[layer], want), f"{layer}: {int((a[layer] != want).any(axis=2).sum())} pixels are not the box filter of the fine frame"
        assert a["steps"] == b["steps"] > 0 and ss.counters()["rays"] == 4 * w * h
        assert a["disk"].max() > 0 and a["bg"].max() > 0
    finally:
        ss.close()
        fine.close()


# ---- 5. frames in flight -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ("strict", "hybrid"))
def test_frames_in_flight_keep_their_own_projection_and_velocity(math, hip_lib):
    """The projection and the velocity travel with the call: four frames queued without a sync alternate two of each, and each
    is the frame of the same call made alone (the post-pass follows the context's arithmetic: the whole frame is compared)."""
    calls = ((EQ, PC.MOVING[0].beta), (FISH, MOVING), (EQ, PC.MOVING[0].beta), (FISH, MOVING))
    one, two = _mk(96, 48, math=math, frame_slots=1), _mk(96, 48, math=math, frame_slots=2)
    try:
        assert two.frame_slots == 2
        want = [_projected(one, PC.V0, p, b) for p, b in calls[:2]]
        assert not np.array_equal(want[0]["bg"], want[1]["bg"])
        for last in range(len(calls)):
            for k in range(last + 1):
                two.render_async(list(PC.V0), None, projection=calls[k][0][0], projection_fov=calls[k][0][1], observer=calls[k][1])
            _same(_read(two), want[last % 2], f"frame {last}")
    finally:
        one.close()
        two.close()


# ---- 6. downstream of the march ---------------------------------------------------------------------------------------------------
def _inject(r, layers):
    from bhr_amd import _lib
    r.write_layer(_lib.LAYER_BG, layers["bg"])
    r.write_layer(_lib.LAYER_DISK, layers["disk"])


def test_graded_and_flared_frames_are_the_stages_on_the_projected_layers(hip_lib):
    from bhr_amd import _lib
    grade = dict(tonemap="aces", exposure=-0.5, transfer="srgb", keep_hdr=True)
    sky = PC.scene()[0] * np.float32(2.0)               # BG above 1 ahead of the camera: the grade and the HDR plane see the headroom
    r, plain = _mk(96, 48, sky=sky), _mk(96, 48, sky=sky)
    try:
        r.set_grade(**grade)
        graded = _projected(r, PC.V0, EQ, PC.FORWARD_09)
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
        flared = _projected(r, PC.V0, FISH, PC.FORWARD_09, lens_flare=True)
        _inject(plain, flared)
        plain.bloom_only()
        unflared = plain.read_layer(_lib.LAYER_FINAL)
        plain.apply_lens_flare()
        assert np.array_equal(plain.read_layer(_lib.LAYER_FINAL), flared["final"])
        assert not np.array_equal(unflared, flared["final"])
    finally:
        r.close()
        plain.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def _proj(kind=1, h=360.0, v=180.0):
    from bhr_amd import _lib
    return _lib.Projection(kind, h, v, 0)


def _refused(r, hip_lib, word, proj=None, beta=None, flags=0):
    from bhr_amd import _lib
    cam = r.camera_uniforms(list(PC.V0), 90.0)
    proj = _proj() if proj is None else proj
    obs = None
    if beta is not None:
        obs = _lib.Observer()
        obs.beta[:] = beta
        obs.sky_shift = 1
    before = r.counters()
    assert hip_lib.bhr_render_projected(r._ctx, C.byref(cam), C.byref(proj), None if obs is None else C.byref(obs), flags) == _lib.BHR_ERR_INVALID
    msg = hip_lib.bhr_last_error().decode()
    assert "bhr_render_projected" in msg and word in msg, msg
    after = r.counters()
    assert all(after[k] == before[k] for k in ("rays", "ray_steps", "frames_timed"))       # nothing was launched


def _renders_as_ever(r, want=None, want_proj=None):
    r.render_async(list(PC.V0), 90.0, skip_bloom=True)
    got = _read(r)
    assert got["steps"] > 0 and got["final"].shape == (r.rows, r.width, 3)
    if want is not None:
        _same(got, want, "the ordinary frame")
    if want_proj is not None:
        _same(_projected(r, PC.V0, FISH, MOVING, skip_bloom=True), want_proj, "the projected frame")
    return got


def test_refusals_name_the_combination_and_leave_the_context_alone(hip_lib):
    from bhr_amd import _lib
    from bhr_amd.disk_v2 import DiskV2Params
    w, h = 32, 16
    nan = float("nan")
    r = _mk(w, h)
    try:
        want, want_proj = _renders_as_ever(r), _projected(r, PC.V0, FISH, MOVING, skip_bloom=True)
        cam, proj = r.camera_uniforms(list(PC.V0), 90.0), _proj()
        for args in ((None, C.byref(cam), C.byref(proj)), (r._ctx, None, C.byref(proj)), (r._ctx, C.byref(cam), None)):
            assert hip_lib.bhr_render_projected(*args, None, 0) == _lib.BHR_ERR_INVALID
            msg = hip_lib.bhr_last_error().decode()
            assert "bhr_render_projected" in msg and "null" in msg
        for kind in (0, 3, -1):
            _refused(r, hip_lib, "kind", proj=_proj(kind))
        for kind, fh, fv, word in ((1, 0.0, 180.0, "fov_h_deg"), (1, 360.5, 180.0, "fov_h_deg"), (1, nan, 180.0, "fov_h_deg"), (1, -90.0, 90.0, "fov_h_deg"),
                                   (1, 360.0, 0.0, "fov_v_deg"), (1, 360.0, 180.5, "fov_v_deg"), (1, 360.0, nan, "fov_v_deg"),
                                   (2, 0.0, 0.0, "fov_h_deg"), (2, 361.0, 0.0, "fov_h_deg"), (2, nan, 0.0, "fov_h_deg"), (2, float("inf"), 0.0, "fov_h_deg")):
            _refused(r, hip_lib, word, proj=_proj(kind, fh, fv))
        for flag in (_lib.SKIP_DIFFERENTIALS, _lib.PERSISTENT, _lib.FORCE_FAST, _lib.FORCE_STRICT, _lib.FORCE_HYBRID, 1 << 20):
            _refused(r, hip_lib, "flags", flags=flag)
        for beta in ((0.996, 0.0, 0.0), (0.7, 0.7, 0.2), (nan, 0.0, 0.0), (0.0, float("inf"), 0.0)):      # what bhr_render_observer refuses for its obs
            _refused(r, hip_lib, "0.995", beta=beta)
        with pytest.raises(ValueError):                          # the Python layer checks its arguments itself
            r.render_async(list(PC.V0), None, projection="cube")
        with pytest.raises(ValueError):
            r.render_async(list(PC.V0), None, projection="fisheye", projection_fov=(400.0,))
        with pytest.raises(ValueError):
            r.render_async(list(PC.V0), None, projection="equirect", observer=(1.0, 0.0, 0.0))
        with pytest.raises(ValueError, match="flags"):
            r.render_async(list(PC.V0), None, projection="equirect", math="fast")
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
        _renders_as_ever(r, want, want_proj)                     # after every refusal that leaves the context usable: both frames are what they were
        r.use_disk_v2(DiskV2Params())                            # (params=None would switch back to the texture)
        _refused(r, hip_lib, "Disk V2")
    finally:
        r.close()
    r = _mk(w, h)
    try:
        _renders_as_ever(r, want, want_proj)                     # a context like the one the refusals met renders the frames it rendered before them
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


# ---- 8. resources ------------------------------------------------------------------------------------------------------------------
def test_resources(hip_lib):
    from bhr_amd import _lib
    for ss in (0, 1):
        out = (C.c_int32 * 3)()
        assert hip_lib.bhr_projected_resources(ss, out) == _lib.BHR_OK
        vgprs, lds, scratch = (int(v) for v in out)
        print(f"[projection] march kernel (supersampled {ss}): {vgprs} VGPRs, {lds} bytes of LDS, {scratch} bytes of scratch")
        assert scratch == 0 and 0 < vgprs <= 128 and lds > 0
    assert hip_lib.bhr_projected_resources(0, None) == _lib.BHR_ERR_INVALID
    r = _mk(8, 8)
    try:
        out = (C.c_int32 * 3)()
        assert hip_lib.bhr_projected_resources(1, out) == _lib.BHR_OK
        assert r.projected_resources(supersampled=True) == dict(vgprs=int(out[0]), lds_bytes=int(out[1]), scratch_bytes=int(out[2]))
    finally:
        r.close()
