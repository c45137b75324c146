"""The Kerr march on the device beyond the two views of tests/test_gpu_kerr.py: a rolled disk (t_offset), views from the pole,
the plane, below it, close in, far out and wide, ragged and tiny frames, rays with three and more disk crossings (the in-loop
flush of the parking slots), supersampling at 4 and 8, symmetries that need no reference, frames in flight with the spin and the
redshift changing between them, and the camera the library refuses.  tests/test_kerr_edges_ref.py shows, without a device,
that the inputs are fair.

Bars: those of tests/test_gpu_kerr.py.  Per layer the device is allowed twice the distance the float32 run of the reference
keeps from its float64 run on the same case (per-channel RMSE over the pixels of equal fate and crossing count), never less than
1e-4; pixels whose fate or crossing count differs from the float64 run are at most 0.5 % of a frame (at most one pixel of a
frame of fewer than 200)."""
import functools
import os

import numpy as np
import pytest

import kerr_cases as KC
import kerr_ref as K
from supersample_ref import box_resolve
from test_gpu_kerr import BAR_FLOOR, FATE_SHARE, _fates, _probe_scene, _same_as_reference

pytestmark = pytest.mark.gpu


def _kw(case):
    return dict(step_size=KC.STEP, r_max=KC.R_MAX, r_disk_inner=case.r_inner, r_disk_outer=KC.R_OUTER, disk_tilt=0.0,
                anti_alias="disabled", disk_rotation_speed=case.speed)


def _read(r):
    from bhr_amd import _lib
    return dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK), final=r.read_layer(_lib.LAYER_FINAL))


@functools.lru_cache(maxsize=None)
def _device(case, supersample=1):
    """Layers, counters and probe read-out of one device frame of an Edge, rendered as the video loop renders frame
    `case.frame`: the roll comes from the frame number and the context's rotation speed."""
    from bhr_amd import HipRenderer
    out = {}
    for name, (sky, tex) in (("frame", KC.edge_scene(case)), ("probe", _probe_scene())):
        r = HipRenderer(case.width, case.height, sky, tex, math="strict", supersample=supersample, **_kw(case))
        try:
            r.set_spin(case.A, force_kerr=case.force)
            if case.redshift == "exact":
                r.set_redshift("exact")
            # the reference is handed the very float32 roll the camera block carries
            assert r.camera_uniforms(list(case.view), case.fov, case.frame).t_offset == case.t_offset
            r.render_async(list(case.view), case.fov, frame=case.frame, skip_bloom=True)
            out[name] = _read(r)
            if name == "frame":
                out["counters"] = r.counters()
        finally:
            r.close()
    return out


def _against_reference(case):
    """The fate cap and the three colour bars of a case; returns (device frame, float64 reference, pixels that agree)."""
    r64 = KC.edge_reference(case, np.float64)
    d32, share32 = KC.float32_distance(case)
    dev = _device(case)
    same = _same_as_reference(dev, r64)
    got = KC.distance(dev["frame"], r64, same)
    differing, pixels = int((~same).sum()), case.width * case.height
    print(f"{case.id}: fate / crossing count differs on {differing} of {pixels} pixels ({differing / pixels:.3%}; float32 reference "
          f"{share32:.3%}); device vs f64 {got}; float32 reference vs f64 {d32}")
    assert all(np.isfinite(dev["frame"][k]).all() for k in ("bg", "disk", "final"))
    assert dev["frame"]["disk"].max() > 0 and dev["frame"]["bg"].max() > 0
    assert dev["counters"]["rays"] == pixels
    assert differing <= (FATE_SHARE * pixels if pixels >= 200 else 1)
    for layer in ("bg", "disk", "final"):
        bar = max(2.0 * d32[layer], BAR_FLOOR)
        assert got[layer] <= bar, f"{layer}: RMSE {got[layer]:.3g} over the bar {bar:.3g}"
    return dev, r64, same


# ----------------------------------------------------------------------------------------------- 1. the roll
@pytest.mark.parametrize("case", KC.ROLL, ids=lambda c: c.id)
def test_rolled_disk_against_the_reference(case, hip_lib):
    dev, _, _ = _against_reference(case)
    still = _device(case._replace(frame=0, speed=0.1))
    moved = KC.rmse(dev["frame"]["disk"], still["frame"]["disk"])
    print(f"{case.id}: the DISK layer is {moved:.3g} RMSE from the same context's frame 0")
    assert moved > 1e-2
    assert np.array_equal(dev["probe"]["bg"], still["probe"]["bg"])              # the roll moves no ray
    assert dev["counters"]["ray_steps"] == still["counters"]["ray_steps"]


def test_a_texture_without_phi_does_not_see_the_roll(hip_lib):
    """No reference in the comparison: a disk that is constant along phi looks the same however far it has turned, up to the
    rounding of the bilinear weights, which the float32 reference's own two frames measure (d; test_kerr_edges_ref.py
    bounds it)."""
    ref_still, ref_rolled = (KC.edge_reference(c, np.float32) for c in KC.RINGS)
    d = max(float(np.abs(ref_still[k].astype(np.float64) - ref_rolled[k]).max()) for k in ("bg", "disk"))
    still, rolled = (_device(c)["frame"] for c in KC.RINGS)
    got = {k: float(np.abs(still[k].astype(np.float64) - rolled[k]).max()) for k in ("bg", "disk")}
    print(f"rings texture, t_offset 0 against {KC.RINGS[1].t_offset}: device frames differ by at most {got}; float32 reference's by {d:.3g}")
    assert still["disk"].max() > 0.05 and np.ptp(still["disk"]) > 0.05
    for k in ("bg", "disk"):
        assert got[k] <= max(2.0 * d, 1e-6), k
    for case in KC.RINGS:
        _against_reference(case)


# ----------------------------------------------------------------------------------------------- 2. views, 3. frame sizes
@pytest.mark.parametrize("case", KC.VIEW_EDGES, ids=lambda c: c.id)
def test_views_against_the_reference(case, hip_lib):
    _against_reference(case)


@pytest.mark.parametrize("case", KC.RAGGED, ids=lambda c: c.id)
def test_ragged_and_tiny_frames_against_the_reference(case, hip_lib):
    dev, r64, _ = _against_reference(case)
    assert dev["counters"]["rays"] == case.width * case.height
    assert dev["counters"]["ray_steps"] > 0
    sky, _, dark_hit = _fates(dev["probe"])
    assert sky.any() and (~sky).any() and dev["frame"]["bg"].shape == (case.height, case.width, 3)


# ----------------------------------------------------------------------------------------------- 4. many crossings
@pytest.mark.parametrize("case", KC.CROSSINGS, ids=lambda c: c.id)
def test_rays_with_three_and_more_crossings(case, hip_lib):
    dev, r64, same = _against_reference(case)
    _, n, _ = _fates(dev["probe"])
    want, got = int((r64["n_hits"] >= 3).sum()), int((n >= 3).sum())
    agree = int(((n >= 3) & same).sum())
    print(f"{case.id}: pixels with three or more crossings: device {got} (at most {int(n.max())}), reference {want} (at most "
          f"{int(r64['n_hits'].max())}); {agree} of the device's agree with the reference in fate and count")
    assert want >= 40
    assert got >= want / 2 and agree >= want / 2


# ----------------------------------------------------------------------------------------------- 5. supersampling
FINE = KC.Edge(0.6, KC.VIEWS[0])


@pytest.mark.parametrize("k,fine", [(2, FINE), (4, FINE), (8, FINE), (4, FINE._replace(redshift="exact")),
                                    (2, FINE._replace(width=62, height=42))], ids=lambda v: f"k{v}" if isinstance(v, int) else v.id)
def test_supersampled_frames_are_the_box_filter_of_the_fine_frame(k, fine, hip_lib):
    """The closeness rule of tests/test_gpu_supersample.py: the resolved layers equal the box filter of the k = 1 frame."""
    assert fine.width % k == 0 and fine.height % k == 0
    coarse = fine._replace(width=fine.width // k, height=fine.height // k)
    ss, ref = _device(coarse, supersample=k), _device(fine)
    for layer in ("bg", "disk"):
        want = box_resolve(ref["frame"][layer], k)
        off = np.abs(ss["frame"][layer].astype(np.float64) - want)
        ulps = off / np.spacing(np.maximum(np.abs(ss["frame"][layer]), np.abs(want))).astype(np.float64)
        bad = int((ss["frame"][layer] != want).any(axis=2).sum())
        print(f"{coarse.id} k={k} {layer}: {bad} pixels differ from the box filter of the fine frame; largest difference {off.max():.3g}, {ulps.max():.3g} ulp")
        assert bad == 0, f"{layer}: {bad} pixels differ from the box filter of the {fine.width} x {fine.height} frame"
    assert ss["counters"]["rays"] == fine.width * fine.height
    assert ss["counters"]["ray_steps"] == ref["counters"]["ray_steps"]
    assert ss["frame"]["disk"].max() > 0


# ----------------------------------------------------------------------------------------------- 6. symmetries
def _states(dev):
    sky, n, dark_hit = _fates(dev["probe"])
    return np.stack([sky.astype(np.int64), n, dark_hit.astype(np.int64)], axis=-1)


@pytest.mark.parametrize("A,view", KC.MIRRORS, ids=lambda v: str(v))
def test_a_hole_of_the_opposite_spin_is_the_mirror_image(A, view, hip_lib):
    """y -> -y with a -> -a maps the metric onto itself: no reference involved."""
    here = _states(_device(KC.Edge(A, view)))
    there = _states(_device(KC.Edge(-A, (view[0], -view[1], view[2]))))
    share = float((here != there[:, ::-1]).any(axis=-1).mean())
    own = float((here != here[:, ::-1]).any(axis=-1).mean())
    print(f"A={A} {view}: {share:.3%} of the pixels differ from the flipped frame of the opposite spin; {own:.1%} from the frame's own flip")
    assert share <= FATE_SHARE
    assert here[..., 0].any() and not here[..., 0].all()
    if view[0] != 0 or view[1] != 0:                   # from the pole the picture is its own flip
        assert own > 0.3


@pytest.mark.parametrize("case", KC.UP_DOWN, ids=lambda c: c.id)
def test_the_equatorial_view_is_its_own_top_bottom_flip(case, hip_lib):
    ref = KC.edge_reference(case, np.float32)
    bar = max(2.0 * KC.rmse(ref["disk"], ref["disk"][::-1]), BAR_FLOOR)
    dev = _device(case)
    states = _states(dev)
    differing = int((states != states[::-1]).any(axis=-1).sum())
    disk = KC.rmse(dev["frame"]["disk"], dev["frame"]["disk"][::-1])
    probe = {k: KC.rmse(dev["probe"][k], dev["probe"][k][::-1]) for k in ("bg", "disk")}
    print(f"{case.id}: {differing} pixels differ in fate or count from the top-bottom flip; DISK {disk:.3g}, probe {probe}; bar {bar:.3g}")
    assert differing <= FATE_SHARE * states.shape[0] * states.shape[1]
    same = ~(states != states[::-1]).any(axis=-1)
    assert KC.rmse(dev["frame"]["disk"][same], dev["frame"]["disk"][::-1][same]) <= bar
    for k in ("bg", "disk"):
        assert KC.rmse(dev["probe"][k][same], dev["probe"][k][::-1][same]) <= bar, k
    assert dev["frame"]["disk"].max() > 0.05 and KC.rmse(dev["frame"]["bg"], dev["frame"]["bg"][::-1]) > 1e-2     # a real frame under a real sky


# ----------------------------------------------------------------------------------------------- 7. frames in flight
IN_FLIGHT = ((0.6, "model"), (-0.9, "exact"), (0.0, "model"), (0.998, "exact"), (0.6, "exact"), (-0.9, "model"), (0.0, "model"), (0.998, "model"))


def _queue(r, k):
    """Frame k of the sequence: a new spin (0: the strict Schwarzschild kernel again), a new redshift, a new roll."""
    A, redshift = IN_FLIGHT[k]
    if redshift == "model":
        r.set_redshift("model")
        r.set_spin(A)
    else:
        r.set_spin(A)
        r.set_redshift("exact")
    r.render_async(list(KC.VIEWS[k % 2]), KC.FOV, frame=7 * k)


def test_spin_redshift_and_roll_change_between_frames_in_flight(hip_lib):
    """Eight frames on a two-slot context, each with another spin, redshift and roll, all queued before anything is read: every
    one is, bit for bit, the frame of a context that renders one at a time.  A read shows the last frame only, so frame k is
    read after the frames up to k have been queued afresh; the last turn is the whole sequence."""
    from bhr_amd import HipRenderer, _lib
    sky, tex = KC.scene()
    one, two = (HipRenderer(256, 144, sky, tex, frame_slots=s, disk_tilt=0.0, anti_alias="disabled") for s in (1, 2))
    try:
        assert (one.frame_slots, two.frame_slots) == (1, 2)
        want = []
        for k in range(len(IN_FLIGHT)):
            _queue(one, k)
            want.append({name: one.read_layer(layer) for name, layer in (("bg", _lib.LAYER_BG), ("disk", _lib.LAYER_DISK))})
        for a, b in ((0, 1), (1, 2), (2, 3), (0, 4), (3, 7)):               # the frames really differ
            assert not np.array_equal(want[a]["disk"], want[b]["disk"])
        for last in range(len(IN_FLIGHT)):
            for k in range(last + 1):
                _queue(two, k)
            for name, layer in (("bg", _lib.LAYER_BG), ("disk", _lib.LAYER_DISK)):
                got = two.read_layer(layer)
                assert np.array_equal(got, want[last][name]), f"frame {last} {name}: {int((got != want[last][name]).any(axis=2).sum())} pixels differ"
    finally:
        one.close()
        two.close()


def _video(tmp, tag, frame_slots, png_level, pairs_on_host):
    from bhr_amd import drivers
    w, h, n = 160, 96, 12
    r, _, _, _ = drivers.make_renderer(w, h, [6, 0, 0.5], 90, n_stars=600, tex_w=512, tex_h=256, frame_slots=frame_slots, spin=0.6)
    assert r.frame_slots == frame_slots and r.spin == 0.6
    if pairs_on_host:
        r.accumulate_entity_layer = functools.partial(r.accumulate_entity_layer, pairs_on_host=True)
    out = os.path.join(tmp, tag, "v.mp4")
    drivers.render_video(r, w, h, n_frames=n, fps=30, output_path=out, fov=90, static_cam_pos=[6, 0, 0.5], orbit=True, assemble=False,
                         png_level=png_level, video_stream="off")
    r.close()
    return drivers._frames_dir(out), n


def test_overlapped_video_loop_around_a_spinning_hole(tmp_path, hip_lib):
    """tests/test_gpu_video_overlap.py's comparison with a spin: the files of the loop that keeps two frames in flight decode
    to the frames of the loop that runs one at a time."""
    from PIL import Image
    from bhr_amd.output import DEVICE
    serial, n = _video(str(tmp_path), "serial", frame_slots=1, png_level=0, pairs_on_host=True)
    overlapped, _ = _video(str(tmp_path), "overlapped", frame_slots=2, png_level=DEVICE, pairs_on_host=False)
    differing = []
    for f in range(n):
        a = np.asarray(Image.open(os.path.join(serial, f"frame_{f:04d}.png")).convert("RGB"))
        b = np.asarray(Image.open(os.path.join(overlapped, f"frame_{f:04d}.png")).convert("RGB"))
        if not np.array_equal(a, b):
            differing.append((f, int((a != b).any(axis=2).sum())))
    assert not differing, f"frames that differ (frame, pixels): {differing[:10]}"
    first = np.asarray(Image.open(os.path.join(serial, "frame_0000.png")).convert("RGB"))
    last = np.asarray(Image.open(os.path.join(serial, f"frame_{n - 1:04d}.png")).convert("RGB"))
    assert first.max() > 100 and (first != last).mean() > 0.01      # the frames are real and the scene moves


# ----------------------------------------------------------------------------------------------- 8. the camera's domain
def test_a_camera_inside_the_static_limit_is_refused(hip_lib):
    from bhr_amd import HipRenderer
    sky, tex = KC.scene()
    good = KC.Edge(0.998, KC.VIEWS[0], width=32, height=16)
    r = HipRenderer(good.width, good.height, sky, tex, math="strict", **_kw(good))
    try:
        r.set_spin(good.A)
        r.render_async(list(good.view), good.fov, skip_bloom=True)
        want, before = _read(r), r.counters()
        for redshift in ("model", "exact"):
            r.set_redshift(redshift)
            for A, view in KC.INSIDE_STATIC_LIMIT:
                assert K.camera_f(view, A)[0] >= 1.0
                r.set_spin(A)
                with pytest.raises(ValueError) as e:
                    r.render_async(list(view), good.fov, skip_bloom=True)
                assert "static limit" in str(e.value).lower() and "bhr_render" in str(e.value), str(e.value)
                with pytest.raises(ValueError, match="static limit"):               # the reference agrees on the domain
                    K.render(K.build_camera(list(view), good.fov, good.width, good.height, KC.R_MAX), A, sky, tex)
        with pytest.raises(ValueError, match="static limit"):                       # inside the horizon f may fall under 1 again
            r.render_async([0.3, 0.2, 0.1], good.fov, skip_bloom=True)
        # nothing was launched, and the context renders as before
        r.set_redshift("model")
        after = r.counters()
        assert all(after[k] == before[k] for k in ("rays", "ray_steps", "frames_timed"))
        r.render_async(list(good.view), good.fov, skip_bloom=True)
        again = _read(r)
        for layer in ("bg", "disk", "final"):
            assert np.array_equal(again[layer], want[layer]), layer
        # the rule is the Kerr march's: without a spin the strict march takes the same camera as ever
        r.set_spin(0.0)
        r.render_async(list(KC.INSIDE_STATIC_LIMIT[0][1]), good.fov, skip_bloom=True)
        assert _read(r)["final"].shape == (good.height, good.width, 3)
        # ... and the forced Kerr march at spin 0 has its static limit at r = 1
        r.set_spin(0.0, force_kerr=True)
        with pytest.raises(ValueError, match="static limit"):
            r.render_async([0.9, 0.0, 0.1], good.fov, skip_bloom=True)
    finally:
        r.close()
