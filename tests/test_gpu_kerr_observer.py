"""The Kerr camera on the device (bhr_render_kerr_view; csrc/ray_kerr_observer.h): bit for bit the Kerr frame at rest under the
pinhole, against its CPU reference tests/kerr_observer_ref.py in binary64, at A = 0 against the Schwarzschild observer's and
projection's frames, its mirror symmetry, supersampling, the fisheye's rim, frames in flight, refusals, resources and what sits
downstream of the march.

Bars: those of tests/test_gpu_kerr.py.  Per layer, twice what the float32 run of the reference keeps from its binary64 run on the
same case, never under 1e-4; pixels whose fate or crossing count differs sit on a discontinuity of the picture, are counted apart
(at most 0.5 % of a frame) and left out of the RMSE.  The device's fates and crossing counts are read from a probe frame -- a white
sky, rendered plain, and a disk of opacity 1/2 per crossing -- as there."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import kerr_cases as KC
import kerr_observer_cases as VC
from supersample_ref import box_resolve
from test_gpu_kerr import BAR_FLOOR, FATE_SHARE, KW, _fates, _probe_scene, _same_as_reference

pytestmark = pytest.mark.gpu

STEPS_RTOL = 2e-4
MOVING = (0.3, -0.4, 0.5)


def _mk(width, height, A, force=False, redshift="model", scene=None, sky_gain=1.0, **kw):
    from bhr_amd import HipRenderer
    sky, tex = scene or KC.scene()
    r = HipRenderer(width, height, sky * np.float32(sky_gain), tex, math="strict", **{**KW, **kw})
    r.set_spin(A, force_kerr=force)
    if redshift == "exact":
        r.set_redshift("exact")
    return r


def _read(r):
    from bhr_amd import _lib
    c = r.counters()
    return dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), final=r.read_layer(_lib.LAYER_FINAL),
                steps=c["ray_steps"], rays=c["rays"])


def _view(r, view, beta="rest", sky=True, projection=None, pfov=None, fov=KC.FOV, **kw):
    """One frame of the Kerr camera; beta "rest": the call without a velocity."""
    r.render_async(list(view), fov, kerr_observer=beta, kerr_observer_sky=sky, kerr_projection=projection, kerr_projection_fov=pfov, **kw)
    return _read(r)


@functools.lru_cache(maxsize=None)
def _device(case, supersample=1):
    """Layers, counters and probe read-out of one device frame of a kerr_observer_cases.Case."""
    beta = VC.beta_of(case)
    out = {}
    for name, scene in (("frame", None), ("probe", _probe_scene())):
        r = _mk(case.width, case.height, case.A, case.force, case.redshift, scene=scene, supersample=supersample)
        try:
            got = _view(r, case.view, "rest" if beta is None else beta, case.sky and name == "frame", case.projection, case.pfov, case.fov, skip_bloom=True)
        finally:
            r.close()
        out[name] = got
    out["counters"] = dict(ray_steps=out["frame"]["steps"], rays=out["frame"]["rays"])
    return out


def _states(dev):
    sky, n, dark_hit = _fates(dev["probe"])
    return np.stack([sky.astype(np.int64), n, dark_hit.astype(np.int64)], axis=-1)


# ---- 1. at rest under the pinhole the frame is the Kerr march's ------------------------------------------------------------------
@pytest.mark.parametrize("redshift", ("model", "exact"))
@pytest.mark.parametrize("A,force", ((0.9, False), (-0.6, False), (0.0, True)), ids=("A0.9", "A-0.6", "forced0"))
def test_identity_at_rest(A, force, redshift, hip_lib):
    view = KC.VIEWS[1]
    for size in ((96, 64), (61, 43), (5, 3)):
        for k in (1, 2):
            r = _mk(*size, A, force, redshift, supersample=k)
            try:
                r.render_async(list(view), KC.FOV)
                want = _read(r)
                for beta, sky in (("rest", True), ((0.0, 0.0, 0.0), True), ((0.0, 0.0, 0.0), False)):
                    got = _view(r, view, beta, sky)
                    for layer in ("bg", "disk", "final"):
                        assert np.array_equal(got[layer], want[layer]), \
                            f"{layer} at {size}, k = {k}, beta {beta}, sky_shift {sky}: {int((got[layer] != want[layer]).any(axis=2).sum())} pixels differ"
                    assert got["steps"] == want["steps"] > 0
                    assert got["rays"] == k * k * size[0] * size[1]
                assert want["disk"].max() > 0 or size == (5, 3)
            finally:
                r.close()


# ---- 2. against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", VC.REFERENCE, ids=lambda c: c.id)
def test_device_against_the_reference_float64(case, hip_lib):
    r64, r32 = VC.reference(case, np.float64), VC.reference(case, np.float32)
    d32, share32 = VC.float32_distance(case)
    dev = _device(case)
    same = _same_as_reference(dev, r64)
    got = KC.distance(dev["frame"], r64, same)
    differing, pixels = int((~same).sum()), case.width * case.height
    steps32 = int(r32["steps"].sum())
    print(f"{case.id}: fate / crossing count differs on {differing} of {pixels} pixels (float32 reference {share32:.3%}); device vs f64 {got}; "
          f"float32 reference vs f64 {d32}; ray_steps {dev['frame']['steps']} (float32 reference {steps32}); BG reaches {float(dev['frame']['bg'].max()):.3f}")
    assert all(np.isfinite(dev["frame"][k]).all() for k in ("bg", "disk", "final"))
    assert dev["frame"]["disk"].max() > 0 and dev["frame"]["bg"].max() > 0
    assert dev["frame"]["rays"] == pixels
    assert differing <= FATE_SHARE * pixels
    for layer in ("bg", "disk", "final"):
        bar = max(2.0 * d32[layer], BAR_FLOOR)
        assert got[layer] <= bar, f"{layer}: RMSE {got[layer]:.3g} over the bar {bar:.3g}"
    assert abs(dev["frame"]["steps"] - steps32) <= STEPS_RTOL * steps32


# ---- 3. the forced Kerr march at A = 0 against the Schwarzschild marches -----------------------------------------------------------
@pytest.mark.parametrize("case", VC.SCHWARZSCHILD, ids=lambda c: c.id)
def test_forced_kerr_at_spin_zero_against_the_schwarzschild_cameras(case, hip_lib):
    """bhr_render_observer's / bhr_render_projected's frame of the same view and velocity, within twice the binary64 distance between
    the two references (tests/test_kerr_observer_ref.py prints it), floor 1e-4."""
    from bhr_amd import HipRenderer
    d_ref, _ = VC.schwarzschild_distance(case)
    kerr = _device(case)
    beta = VC.beta_of(case)
    schw = {}
    for name, (sky, tex) in (("frame", KC.scene()), ("probe", _probe_scene())):
        r = HipRenderer(case.width, case.height, sky, tex, math="strict", **KW)
        try:
            r.render_async(list(case.view), case.fov, skip_bloom=True, observer=beta, observer_sky=case.sky and name == "frame",
                           projection=case.projection, projection_fov=case.pfov)
            schw[name] = _read(r)
        finally:
            r.close()
    here, there = _states(kerr), _states(schw)
    same = ~(here != there).any(axis=-1)
    got = KC.distance(kerr["frame"], schw["frame"], same)
    share = float((~same).mean())
    print(f"{case.id}: forced Kerr camera vs the Schwarzschild march: fate / crossing count differs on {share:.3%}; distance {got}; references' {d_ref}")
    assert share <= FATE_SHARE
    assert kerr["frame"]["disk"].max() > 0 and kerr["frame"]["bg"].max() > 0
    for layer in ("bg", "disk", "final"):
        bar = max(2.0 * d_ref[layer], BAR_FLOOR)
        assert got[layer] <= bar, f"{layer}: RMSE {got[layer]:.3g} over the bar {bar:.3g}"


# ---- 4. mirror ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (VC.Case(0.9, (3.0, 2.0, 0.3), (0.3, -0.4, 0.2)), VC.Case(-0.6, (4.0, -3.0, -0.4), (0.1, 0.5, -0.3), redshift="exact"),
                                  VC.Case(0.9, (3.0, 2.0, 0.3), (0.3, -0.4, 0.2), projection="fisheye", pfov=(200.0,), width=64, height=64)),
                         ids=lambda c: c.id)
def test_opposite_spin_mirrored_camera_is_the_flipped_frame(case, hip_lib):
    """y -> -y with a -> -a maps the metric onto itself, and the velocity goes with the camera: no reference involved.  The
    tolerance is tests/test_gpu_kerr_edges.py's for its mirrors."""
    x, y, z = case.view
    bx, by, bz = case.beta
    here = _states(_device(case))
    there = _states(_device(case._replace(A=-case.A, view=(x, -y, z), beta=(bx, -by, bz))))
    share = float((here != there[:, ::-1]).any(axis=-1).mean())
    own = float((here != here[:, ::-1]).any(axis=-1).mean())
    print(f"{case.id}: {share:.3%} of the pixels differ from the flipped frame of the mirrored camera; {own:.1%} from the frame's own flip")
    assert share <= FATE_SHARE
    assert here[..., 0].any() and not here[..., 0].all()
    assert own > 0.1


# ---- 5. supersampling, 6. the fisheye's rim ----------------------------------------------------------------------------------------
FINE = (VC.Case(0.6, KC.VIEWS[0], MOVING), VC.Case(0.6, KC.VIEWS[0], MOVING, redshift="exact", projection="fisheye", pfov=(220.0,), width=64, height=64))


@pytest.mark.parametrize("fine", FINE, ids=lambda c: c.id)
def test_supersampled_frame_is_the_box_filter_of_the_fine_frame(fine, hip_lib):
    k = 2
    coarse = fine._replace(width=fine.width // k, height=fine.height // k)
    ss, ref = _device(coarse, supersample=k), _device(fine)
    for layer in ("bg", "disk"):
        want = box_resolve(ref["frame"][layer], k)
        bad = int((ss["frame"][layer] != want).any(axis=2).sum())
        assert bad == 0, f"{layer}: {bad} pixels differ from the box filter of the {fine.width} x {fine.height} frame"
    assert ss["frame"]["rays"] == fine.width * fine.height
    assert ss["frame"]["steps"] == ref["frame"]["steps"] > 0
    assert ss["frame"]["disk"].max() > 0
    if fine.projection == "fisheye":                           # rim zeros enter the filter: a rim pixel is neither black nor whole
        inside = VC.reference(fine)["inside"]
        part = box_resolve(inside[..., None].astype(np.float32), k)[..., 0]
        rim = (part > 0) & (part < 1)
        assert rim.sum() > 10 and np.all(ss["frame"]["bg"][part == 0] == 0) and np.all(ss["frame"]["disk"][part == 0] == 0)


def test_fisheye_rim_is_exactly_zero_and_adds_no_steps(hip_lib):
    """Outside the image circle BG and DISK are exactly 0.  The circle is inscribed in the shorter side: a wider frame is the
    square one with more rim, the same rays to the bit and not one step more."""
    square = VC.Case(0.6, KC.VIEWS[0], MOVING, projection="fisheye", pfov=(220.0,), width=64, height=64)
    wide = square._replace(width=96)
    s, w = _device(square), _device(wide)
    inside = VC.reference(square)["inside"]
    assert 0.7 < inside.mean() < 0.8                           # pi / 4 of the square
    for layer in ("bg", "disk"):
        assert np.all(s["frame"][layer][~inside] == 0)
        assert np.array_equal(w["frame"][layer][:, 16:80], s["frame"][layer])
        assert np.all(w["frame"][layer][:, :16] == 0) and np.all(w["frame"][layer][:, 80:] == 0)
    assert s["frame"]["bg"][inside].min() >= 0 and (s["frame"]["bg"].max(axis=2)[inside] > 0).mean() > 0.5
    assert (s["frame"]["rays"], w["frame"]["rays"]) == (64 * 64, 96 * 64)
    assert w["frame"]["steps"] == s["frame"]["steps"] > 0
    two = _device(square._replace(width=32, height=32), supersample=2)
    assert two["frame"]["rays"] == 4 * 32 * 32


# ---- 7. frames in flight -----------------------------------------------------------------------------------------------------------
def test_frames_in_flight_keep_their_own_velocity_and_projection(hip_lib):
    from bhr_amd import HipRenderer
    sky, tex = KC.scene()
    frames = (dict(beta=MOVING, sky=True), dict(beta=(-0.2, 0.1, 0.0), sky=False, projection="fisheye", pfov=(200.0,)),
              dict(beta="rest", projection="equirect", pfov=(360.0, 180.0)))
    one, two = (HipRenderer(96, 64, sky, tex, frame_slots=s, **KW) for s in (1, 2))
    try:
        assert (one.frame_slots, two.frame_slots) == (1, 2)
        for r in (one, two):
            r.set_spin(0.9)
        want = [_view(one, KC.VIEWS[1], **f) for f in frames]
        assert not np.array_equal(want[0]["bg"], want[1]["bg"]) and not np.array_equal(want[1]["bg"], want[2]["bg"])
        for order in ((0, 1), (1, 0), (2, 0, 1), (0, 1, 2)):
            for k in order[:-1]:
                two.render_async(list(KC.VIEWS[1]), KC.FOV, kerr_observer=frames[k]["beta"], kerr_observer_sky=frames[k].get("sky", True),
                                 kerr_projection=frames[k].get("projection"), kerr_projection_fov=frames[k].get("pfov"))
            got = _view(two, KC.VIEWS[1], **frames[order[-1]])
            for layer in ("bg", "disk", "final"):
                assert np.array_equal(got[layer], want[order[-1]][layer]), (order, layer)
    finally:
        one.close()
        two.close()


# ---- 8. motion shows ---------------------------------------------------------------------------------------------------------------
def test_motion_shows(hip_lib):
    """tests/test_gpu_observer.py's test around a spinning hole: under a sky twice as bright as the tests' own."""
    view = KC.VIEWS[0]
    ahead = tuple(-0.6 * v / np.linalg.norm(view) for v in view)       # at the hole
    r = _mk(KC.W, KC.H, 0.9, sky_gain=2.0)
    try:
        rest = _view(r, view, (0.0, 0.0, 0.0), skip_bloom=True)
        shifted, plain = _view(r, view, ahead, True, skip_bloom=True), _view(r, view, ahead, False, skip_bloom=True)
        assert (shifted["bg"] != rest["bg"]).mean() > 0.2 and (shifted["disk"] != rest["disk"]).any()
        assert np.array_equal(shifted["disk"], plain["disk"]) and shifted["steps"] == plain["steps"]
        assert not np.array_equal(shifted["bg"], plain["bg"])
        assert shifted["bg"].max() > 1.0 and shifted["final"].max() <= 1.0
        dark = lambda f: int(((f["bg"].max(axis=2) == 0) & (f["disk"].max(axis=2) == 0)).sum())
        assert dark(plain) < dark(rest)                          # flying at the hole squeezes its image
    finally:
        r.close()


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------
def _refused(r, lib, word, cam=None, beta=(0.1, 0.0, 0.0), proj=None, flags=0):
    from bhr_amd import _lib
    obs = _lib.Observer()
    obs.beta[:] = beta
    obs.sky_shift = 1
    cam = r.camera_uniforms(list(KC.VIEWS[1]), KC.FOV) if cam is None else cam
    rc = lib.bhr_render_kerr_view(r._ctx, C.byref(cam), C.byref(obs), None if proj is None else C.byref(proj), flags)
    msg = lib.bhr_last_error().decode()
    assert rc == _lib.BHR_ERR_INVALID, (word, rc)
    assert "bhr_render_kerr_view" in msg and word in msg, msg


def test_refusals_name_the_combination_and_leave_the_context_alone(hip_lib):
    from bhr_amd import HipRenderer, _lib
    from bhr_amd.disk_v2 import DiskV2Params
    nan = float("nan")
    sky, tex = KC.scene()
    r = HipRenderer(32, 16, sky, tex, math="strict", **KW)
    try:
        P = lambda kind, h=180.0, v=90.0: _lib.Projection(kind, h, v, 0)
        _refused(r, hip_lib, "without the Kerr march")                         # no spin and no forced Kerr
        r.render_async(list(KC.VIEWS[1]), KC.FOV, skip_bloom=True)
        schwarzschild = _read(r)
        r.set_spin(0.9)
        want = _view(r, KC.VIEWS[1], MOVING, skip_bloom=True)
        cam = r.camera_uniforms(list(KC.VIEWS[1]), KC.FOV)
        for args in ((None, C.byref(cam)), (r._ctx, None)):
            assert hip_lib.bhr_render_kerr_view(*args, None, None, 0) == _lib.BHR_ERR_INVALID
            assert "bhr_render_kerr_view" in hip_lib.bhr_last_error().decode()
        for beta in ((0.996, 0.0, 0.0), (0.7, 0.7, 0.2), (nan, 0.0, 0.0), (0.0, float("inf"), 0.0)):
            _refused(r, hip_lib, "0.995", beta=beta)
        for kind in (0, 3, -1):
            _refused(r, hip_lib, "kind", proj=P(kind))
        for kind, fh, fv, word in ((1, 0.0, 180.0, "fov_h_deg"), (1, 360.5, 180.0, "fov_h_deg"), (1, nan, 180.0, "fov_h_deg"), (1, 360.0, 0.0, "fov_v_deg"),
                                   (1, 360.0, 180.5, "fov_v_deg"), (1, 360.0, nan, "fov_v_deg"), (2, 0.0, 0.0, "fov_h_deg"), (2, 361.0, 0.0, "fov_h_deg")):
            _refused(r, hip_lib, word, proj=P(kind, fh, fv))
        for flag in (_lib.SKIP_DIFFERENTIALS, _lib.PERSISTENT, _lib.FORCE_FAST, _lib.FORCE_STRICT, _lib.FORCE_HYBRID, 1 << 20):
            _refused(r, hip_lib, "flags", flags=flag)
        for A, pos in KC.INSIDE_STATIC_LIMIT:
            r.set_spin(A)
            _refused(r, hip_lib, "static limit", cam=r.camera_uniforms(list(pos), KC.FOV))
        r.set_spin(0.9)
        with pytest.raises(ValueError):                              # the Python layer checks its arguments itself
            r.render_async(list(KC.VIEWS[1]), KC.FOV, kerr_projection="cube")
        with pytest.raises(ValueError):
            r.render_async(list(KC.VIEWS[1]), KC.FOV, kerr_observer=(1.0, 0.0, 0.0))
        # bhr_render_observer and bhr_render_projected with a spin are refused as ever
        for kw in (dict(observer=MOVING), dict(projection="fisheye")):
            with pytest.raises(ValueError, match="spin"):
                r.render_async(list(KC.VIEWS[1]), KC.FOV, **kw)
        got = _view(r, KC.VIEWS[1], MOVING, skip_bloom=True)          # after every refusal: the frame is what it was
        for layer in ("bg", "disk", "final"):
            assert np.array_equal(got[layer], want[layer]), layer
        assert got["steps"] == want["steps"]
        r.set_spin(0.0)
        r.render_async(list(KC.VIEWS[1]), KC.FOV, skip_bloom=True)
        again = _read(r)
        assert np.array_equal(again["bg"], schwarzschild["bg"]) and np.array_equal(again["disk"], schwarzschild["disk"])
        # what bhr_set_spin refuses it refuses ahead of this call: no context can have a spin and any of these
        r.set_supersample(2, 0.05)
        with pytest.raises(ValueError, match="adaptive supersampling"):
            r.set_spin(0.9)
        r.set_supersample(1)
        r.use_disk_v2(DiskV2Params())
        with pytest.raises(ValueError, match="Disk V2"):
            r.set_spin(0.9)
        _refused(r, hip_lib, "without the Kerr march")
    finally:
        r.close()
    for kw, word in ((dict(disk_tilt=10.0), "tilt"), (dict(anti_alias="lod_radius"), "anti_alias")):
        r = HipRenderer(32, 16, sky, tex, math="strict", **{**KW, **kw})
        try:
            with pytest.raises(ValueError, match=word):
                r.set_spin(0.9)
            _refused(r, hip_lib, "without the Kerr march")
        finally:
            r.close()
    r = HipRenderer(32, 16, sky, tex, math="strict", rows=(0, 8), **KW)
    try:
        with pytest.raises(ValueError):
            r.set_spin(0.9)
        _refused(r, hip_lib, "without the Kerr march")
    finally:
        r.close()


# ---- 10. resources and downstream --------------------------------------------------------------------------------------------------
def test_resources(hip_lib):
    from bhr_amd import HipRenderer
    sky, tex = KC.scene()
    r = HipRenderer(32, 16, sky, tex, **KW)
    try:
        for exact in (False, True):
            for ss in (False, True):
                res = r.kerr_view_resources(exact=exact, supersampled=ss)
                print(f"Kerr camera kernel (exact {exact}, supersampled {ss}): {res}")
                assert res["scratch_bytes"] == 0 and 0 < res["vgprs"] <= 128 and res["lds_bytes"] > 0
    finally:
        r.close()


def test_flared_and_graded_frame_is_finite(hip_lib):
    r = _mk(KC.W, KC.H, 0.9, lens_flare=True)
    try:
        r.set_grade(tonemap="aces", exposure=0.5, white=2.5, transfer="srgb")
        got = _view(r, KC.VIEWS[0], MOVING, projection="fisheye", pfov=(200.0,))
        assert np.isfinite(got["final"]).all() and got["final"].max() > 0.05 and 0 <= got["final"].min() and got["final"].max() <= 1
    finally:
        r.close()


def test_orbit_video_from_the_circular_camera(tmp_path, hip_lib):
    from bhr_amd import drivers
    w, h, n = 64, 32, 6
    pov = [3.0, 2.0, 0.0]
    r, _, _, _ = drivers.make_renderer(w, h, pov, 90, n_stars=200, tex_w=256, tex_h=128, spin=0.9)
    try:
        out = os.path.join(str(tmp_path), "v.mp4")
        drivers.render_video(r, w, h, n_frames=n, fps=30, output_path=out, fov=90, static_cam_pos=pov, orbit=True, assemble=False,
                             video_stream="off", kerr_view=dict(observer="circular"))
    finally:
        r.close()
    files = sorted(f for f in os.listdir(drivers._frames_dir(out)) if f.startswith("frame_"))
    assert files == [f"frame_{f:04d}.png" for f in range(n)]
    from PIL import Image
    first = np.asarray(Image.open(os.path.join(drivers._frames_dir(out), files[0])).convert("RGB"))
    assert first.shape == (h, w, 3) and first.max() > 50
