"""The cases of the observer and projection edge tests (tests/test_observer_edges_ref.py without a device;
tests/test_gpu_observer_edges.py and tests/test_gpu_projection_edges.py on one), their observer_ref / projection_ref frames,
each computed once, and the one statement of the bars and of a device frame that the two device files share.

What tests/observer_cases.py and tests/projection_cases.py fix -- the field of view, the frame size, the inner radius, r_max, the
disk's roll -- is a field of an Edge here.  The roll is given the way the video loop gives it, as a frame number and the disk's
rotation speed; t_offset is the float32 product the camera block carries."""
import functools
import typing

import numpy as np

import kerr_ref as K
import observer_cases as OC
import observer_ref as R
import projection_ref as P

STEP, R_OUTER = 0.1, 15.0
PINHOLE = "pinhole"
V0, V1 = OC.VIEWS                                  # (6, 0, 0.5) and (3, 2, 0.3)
MOVING = (0.3, -0.4, 0.5)
POLAR_BETA = (0.3, 0.2, -0.4)
SLOW = (0.2, 0.1, 0.0)
MANY = (0.0, 0.6, 0.3)

BAR_FLOOR, OFF_SHARE, OFF_TOL, STEPS_RTOL, STEPS_SLACK, SMALL_FRAME = 1e-4, 0.005, 1e-3, 2e-4, 2, 200    # tests/test_gpu_observer.py's bars


class Edge(typing.NamedTuple):
    name: str
    view: tuple = V0
    beta: typing.Optional[tuple] = MOVING          # None: no observer block (projections only): the camera stands still
    kind: str = PINHOLE                            # or projection_ref.EQUIRECT / FISHEYE
    fov: typing.Any = 90.0                         # pinhole: degrees; equirect: (h, v); fisheye: (full angle,)
    size: tuple = (48, 32)
    tilt: float = 0.0
    r_inner: float = 2.0
    r_max: float = 10.0
    frame: int = 0
    speed: float = 0.1
    sky: bool = True
    fates: str = "both"                            # what the frame holds: "both" captured and escaped rays, or "escaped" rays only

    @property
    def t_offset(self):
        return float(np.float32(float(self.frame) * self.speed))

    @property
    def pixels(self):
        return self.size[0] * self.size[1]


def _along(direction, speed):
    """A velocity of `speed` along `direction`, as the three float32 the call carries; where their rounding takes |beta| over
    0.995 (the library's limit) it is shortened by parts in 1e7 until it does not."""
    d = np.array(direction, dtype=np.float64)
    b = speed * d / np.linalg.norm(d)
    while np.linalg.norm(b.astype(np.float32).astype(np.float64)) > R.BETA_MAX:
        b *= 1.0 - 1e-7
    return tuple(float(v) for v in b.astype(np.float32))


def _named(kind, view):
    return tuple(float(v) for v in R.velocity(kind, view))


def ahead(view, speed):
    return _along(-np.array(view), speed)


def sideways(view, speed):
    """Along the circular orbit's direction, normalize(r_hat x z_hat)."""
    return _along(np.cross(np.array(view, dtype=np.float64), [0.0, 0.0, 1.0]), speed)


# ----------------------------------------------------------------------------------------------- the pinhole observer
VIEW_EDGES = (Edge("pole", (0.0, 0.0, 6.0), POLAR_BETA),                       # build_camera's fallback up vector
              Edge("near_pole", (0.05, 0.0, 6.0), POLAR_BETA),
              Edge("in_plane", (6.0, 0.0, 0.0), _named("circular", (6.0, 0.0, 0.0))),      # f_old = 0 at the start
              Edge("below", (5.0, 1.0, -2.0), _named("infall", (5.0, 1.0, -2.0))),
              Edge("close", (1.6, 0.0, 0.2), _named("infall", (1.6, 0.0, 0.2))),
              Edge("closer_wide", (1.2, 0.1, 0.1), _named("infall", (1.2, 0.1, 0.1)), fov=120.0, r_inner=1.5),
              Edge("wide", (9.5, 0.0, 1.0), SLOW, fov=150.0),
              Edge("far", (35.0, 0.0, 3.0), SLOW, fov=30.0, r_max=40.0))
AHEAD_995 = Edge("ahead_0.995", V0, ahead(V0, 0.995), fates="escaped")             # D reaches 17: above the cap of 1.5
SIDEWAYS_995 = Edge("sideways_0.995", V0, sideways(V0, 0.995), fates="escaped")    # D falls to 0.055: below the sky's clamp of 0.1
VELOCITIES = (AHEAD_995, SIDEWAYS_995, Edge("away_0.6", V0, ahead(V0, -0.6)))
# The radial cases look from (6, 0, 0.75) and not from (6, 0, 0.5), where they were planned: an odd frame's middle pixel looks along
# -pos, but from (6, 0, 0.5) the float32 d x p of that pixel is 2e-6 (pinhole) and 3e-8 (fisheye), not 0 -- forward_z 6 and
# forward_x 0.5 round apart.  With pos_z / pos_x = 1 / 8 the two products are equal bit for bit, with and without the velocity.
RADIAL_VIEW = (6.0, 0.0, 0.75)
RADIAL_PINHOLE = Edge("33x33_ahead_0.9", RADIAL_VIEW, ahead(RADIAL_VIEW, 0.9), size=(33, 33))     # beta lies along -pos too
RAGGED = (Edge("61x43", V1, size=(61, 43)),
          RADIAL_PINHOLE,
          Edge("5x3_circular", V0, _named("circular", V0), size=(5, 3)),
          Edge("1x1", V0, size=(1, 1), fates="escaped"),
          Edge("1x7", V0, size=(1, 7)),
          Edge("130x3", V1, size=(130, 3)),
          Edge("9x65_circular_tilt25", V1, _named("circular", V1), size=(9, 65), tilt=25.0))
ROLL_PINHOLE = Edge("roll_f375", V0, _named("circular", V0), frame=375, speed=0.1)          # t_offset 37.5
CROSSINGS_PINHOLE = Edge("crossings", (6.0, 0.0, 0.1), MANY, fov=24.0, size=(96, 32), r_inner=1.2)
PINHOLE_COMPARED = VIEW_EDGES + VELOCITIES + RAGGED

# ----------------------------------------------------------------------------------------------- the projections
EQ_FULL, FISH_180 = (360.0, 180.0), (180.0,)
FISH_CENTRE = Edge("fish180_33x33_rest", RADIAL_VIEW, beta=None, kind=P.FISHEYE, fov=FISH_180, size=(33, 33))      # the rho == 0 pixel
PROJECTIONS = (Edge("eq_61x31", V1, kind=P.EQUIRECT, fov=EQ_FULL, size=(61, 31)),
               Edge("eq_7x3_rest", beta=None, kind=P.EQUIRECT, fov=EQ_FULL, size=(7, 3)),
               Edge("eq_1x1", kind=P.EQUIRECT, fov=EQ_FULL, size=(1, 1), fates="escaped"),
               Edge("eq_130x5", kind=P.EQUIRECT, fov=EQ_FULL, size=(130, 5)),
               Edge("eq_10x5deg", kind=P.EQUIRECT, fov=(10.0, 5.0), size=(64, 32), fates="escaped"),
               Edge("eq_pole", (0.0, 0.0, 6.0), POLAR_BETA, kind=P.EQUIRECT, fov=EQ_FULL, size=(64, 32)),
               Edge("eq_ahead_0.995", beta=ahead(V0, 0.995), kind=P.EQUIRECT, fov=EQ_FULL, size=(64, 32), fates="escaped"),
               FISH_CENTRE,
               Edge("fish10", kind=P.FISHEYE, fov=(10.0,), size=(33, 33), fates="escaped"),
               Edge("fish360_45x29_tilt25", V1, kind=P.FISHEYE, fov=(360.0,), size=(45, 29), tilt=25.0),
               Edge("fish220_29x45_ahead_0.9", beta=ahead(V0, 0.9), kind=P.FISHEYE, fov=(220.0,), size=(29, 45)),
               Edge("fish360_sideways_0.995", beta=sideways(V0, 0.995), kind=P.FISHEYE, fov=(360.0,), size=(31, 31)),
               Edge("fish_1x1", kind=P.FISHEYE, fov=FISH_180, size=(1, 1), fates="escaped"))
ROLL_EQUIRECT = Edge("eq_roll_f400", kind=P.EQUIRECT, fov=EQ_FULL, size=(64, 32), frame=400, speed=-0.1)      # t_offset -40
CROSSINGS_EQUIRECT = Edge("eq_crossings", (6.0, 0.0, 0.05), MANY, kind=P.EQUIRECT, fov=(60.0, 20.0), size=(96, 32), r_inner=1.2)

ROLL = (ROLL_PINHOLE, ROLL_EQUIRECT)
CROSSINGS = (CROSSINGS_PINHOLE, CROSSINGS_EQUIRECT)
RADIAL = (RADIAL_PINHOLE, FISH_CENTRE)                                         # a ray with L = 0: m15L2 = 0 and Lv = 0
CLAMPS = (AHEAD_995, SIDEWAYS_995)
CLAMPS_PROJECTED = tuple(c for c in PROJECTIONS if "0.995" in c.name)
ALL = PINHOLE_COMPARED + PROJECTIONS + ROLL + CROSSINGS


def scene():
    return OC.scene()


def camera(case):
    """The camera block of a case (a projection uses its basis and position only: any field of view)."""
    return K.build_camera(list(case.view), case.fov if case.kind == PINHOLE else 90.0, case.size[0], case.size[1], case.r_max)


@functools.lru_cache(maxsize=None)
def reference(case, dtype=np.float64):
    """observer_ref's or projection_ref's frame of a case (read-only: shared between tests)."""
    sky, tex = scene()
    kw = dict(h_base=STEP, r_inner=case.r_inner, r_outer=R_OUTER, tilt_deg=case.tilt, t_offset=case.t_offset, sky_shift_on=case.sky, dtype=dtype)
    if case.kind == PINHOLE:
        out = R.render(camera(case), case.beta, sky, tex, **kw)
        out["inside"] = np.ones(out["fate"].shape, dtype=bool)
    else:
        out = P.render(camera(case), case.kind, case.fov, case.beta, sky, tex, **kw)
    for v in out.values():
        v.setflags(write=False)
    return out


rmse, off_share = OC.rmse, OC.off_share


def off_pixels(a, b):
    """The number of pixels that differ by more than 1e-3 in any channel of any of the layer pairs (a[k], b[k])."""
    return int(round(off_share(a, b, OFF_TOL) * a[0].shape[0] * a[0].shape[1]))


def steps_bar(steps32):
    """The step total's bar: 2e-4 of the float32 reference's, never tighter than 2 steps (a ray that ends within rounding of
    r_escape may take one step more or fewer, and a tiny frame must be allowed one such ray)."""
    return max(STEPS_RTOL * steps32, STEPS_SLACK)


def off_cap(pixels):
    """The number of pixels that may be off by more than 1e-3: 0.5 % of a frame, one pixel of a frame of fewer than 200."""
    return OFF_SHARE * pixels if pixels >= SMALL_FRAME else 1


# ----------------------------------------------------------------------------------------------- the device's frame of a case
def probe_scene():
    """A white sky and a disk of constant opacity 1/2 per crossing: under a plain sky BG = 2^-crossings for a ray that reaches the
    sky and 0 for any other."""
    sky = np.ones((16, 32, 3), dtype=np.float32)
    tex = np.ones((8, 16, 4), dtype=np.float32)
    tex[..., 3] = np.float32(1.0 - 0.5 ** (1.0 / K.DISK_ALPHA_GAIN))
    return sky, tex


def device_frames(case, frames, supersample=1, probe=False, size=None):
    """BG, DISK, the step total and the ray count of the frames numbered `frames` of a case on one context, each rendered as
    the video loop renders it: the roll comes from the frame number and the context's rotation speed.  probe: the probe scene.
    size: another frame size than the case's (the fine frame of a supersampled one)."""
    from bhr_amd import HipRenderer, _lib
    sky, tex = probe_scene() if probe else scene()
    w, h = case.size if size is None else size
    r = HipRenderer(w, h, sky, tex, math="strict", disk_tilt=case.tilt, supersample=supersample, step_size=STEP, r_max=case.r_max,
                    r_disk_inner=case.r_inner, r_disk_outer=R_OUTER, anti_alias="disabled", disk_rotation_speed=case.speed)
    try:
        fov = case.fov if case.kind == PINHOLE else 90.0
        # the reference is handed the very float32 roll the camera block carries
        assert r.camera_uniforms(list(case.view), fov, case.frame).t_offset == case.t_offset
        kw = {} if case.beta is None else dict(observer=case.beta, observer_sky=case.sky)
        if case.kind != PINHOLE:
            kw.update(projection=case.kind, projection_fov=case.fov)
        out = []
        for frame in frames:
            r.render_async(list(case.view), None if case.kind != PINHOLE else fov, frame=frame, skip_bloom=True, **kw)
            layers = dict(bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK))
            c = r.counters()
            out.append(dict(layers, steps=c["ray_steps"], rays=c["rays"]))
        return out
    finally:
        r.close()


def device_frame(case, **kw):
    """Frame `case.frame` of a case on a context of its own."""
    return device_frames(case, (case.frame,), **kw)[0]


def crossings_of(probe):
    """(reached the sky, crossings of such a ray or -1) of a probe frame rendered under a plain sky."""
    bg = probe["bg"][..., 0].astype(np.float64)
    sky = bg > 0
    return sky, np.where(sky, np.rint(-np.log2(np.where(sky, bg, 1.0))), -1).astype(np.int64)


def check_frame_bars(case, got, tag):
    """tests/test_gpu_observer.py's bars on the device frame `got` of a case, each figure printed ahead of its assertion:
    per layer and channel the RMSE to binary64 is at most max(2 x the float32 reference's own, 1e-4); at most 0.5 % of the pixels
    (one pixel of a frame of fewer than 200) are off by more than 1e-3; the step total is within 2e-4 of the float32 reference's
    (never tighter than 2 steps); the layers are finite; rays == W x H; a fisheye's pixels outside the float32 mask are exactly 0."""
    r64, r32 = reference(case, np.float64), reference(case, np.float32)
    w, h = case.size
    assert got["bg"].shape == got["disk"].shape == (h, w, 3)
    assert np.isfinite(got["bg"]).all() and np.isfinite(got["disk"]).all()
    verdict = []
    for layer in ("bg", "disk"):
        d32, d = rmse(r32[layer], r64[layer]), rmse(got[layer], r64[layer])
        bar = np.maximum(2.0 * d32, BAR_FLOOR)
        print(f"[{tag}] {case.name} {layer}: device {d} from binary64, the float32 reference {d32}, bar {bar}")
        verdict.append(((d <= bar).all(), (case.name, layer, d, bar)))
    off = off_pixels((got["bg"], got["disk"]), (r64["bg"], r64["disk"]))
    off32 = off_pixels((r32["bg"], r32["disk"]), (r64["bg"], r64["disk"]))
    steps32 = int(r32["steps"].sum())
    print(f"[{tag}] {case.name}: {off} of {case.pixels} pixels off by more than 1e-3 (float32 reference {off32}; at most {off_cap(case.pixels):g}); "
          f"ray_steps {got['steps']} (float32 reference {steps32}, binary64 {int(r64['steps'].sum())}); "
          f"{int((~r32['inside']).sum())} pixels outside the image circle")
    for ok, what in verdict:
        assert ok, what
    assert off <= off_cap(case.pixels)
    assert abs(got["steps"] - steps32) <= steps_bar(steps32)
    assert got["rays"] == case.pixels
    if case.kind == P.FISHEYE:
        outside = ~r32["inside"]
        blank = (got["bg"] == 0).all(axis=2) & (got["disk"] == 0).all(axis=2)
        assert blank[outside].all(), f"{int((~blank[outside]).sum())} pixels outside the image circle are not exactly 0"
    return r64, r32


# ----------------------------------------------------------------------------------------------- the checks the two device files share
def check_against_reference(case, tag):
    got = device_frame(case)
    check_frame_bars(case, got, tag)
    return got


def check_many_crossings(case, tag):
    """The frame bars, and on the pixels where the binary64 reference has three or more crossings -- a handful, which a frame's
    RMSE does not see -- the largest |device - binary64| in DISK and in BG is at most max(2 x the float32 reference's largest
    difference on those same pixels, 1e-3).  The device's own crossing counts come from a probe frame."""
    got = device_frame(case)
    r64, r32 = check_frame_bars(case, got, tag)
    many = r64["n_hits"] >= 3
    sky, n = crossings_of(device_frame(case._replace(sky=False), probe=True))
    agree = (n >= 3) & (r64["fate"] == 1) & (n == r64["n_hits"])
    print(f"[{tag}] {case.name}: pixels with three or more crossings: device {int((n >= 3).sum())} among the rays that reach the sky (at most "
          f"{int(n.max())}), reference {int((many & (r64['fate'] == 1)).sum())} among those and {int(many.sum())} in all (at most "
          f"{int(r64['n_hits'].max())}); {int(agree.sum())} of the device's have the reference's fate and count")
    assert (n >= 3).sum() >= 10 and agree.sum() >= 10
    for layer in ("disk", "bg"):
        d = float(np.abs(got[layer].astype(np.float64) - r64[layer])[many].max())
        d32 = float(np.abs(r32[layer].astype(np.float64) - r64[layer])[many].max())
        bar = max(2.0 * d32, 1e-3)
        print(f"[{tag}] {case.name} {layer} on the {int(many.sum())} pixels with three or more crossings: largest |device - binary64| {d:.3g}, "
              f"the float32 reference's {d32:.3g}, bar {bar:.3g}")
        assert d <= bar, (case.name, layer, d, bar)


def check_roll(case, tag):
    """Against the reference; the DISK layer differs from the same context's frame 0; under the probe scene, whose disk the roll
    cannot show on, BG is bit for bit frame 0's and the step totals are equal: the roll moves no ray."""
    rolled, still = device_frames(case, (case.frame, 0))
    check_frame_bars(case, rolled, tag)
    moved = rmse(rolled["disk"], still["disk"]).max()
    print(f"[{tag}] {case.name}: t_offset {case.t_offset!r}; the DISK layer is {moved:.3g} RMSE from the same context's frame 0")
    assert moved > 1e-2
    assert rolled["steps"] == still["steps"]
    probe_rolled, probe_still = device_frames(case, (case.frame, 0), probe=True)
    assert probe_still["bg"].max() > 0 and probe_still["disk"].max() > 0
    assert np.array_equal(probe_rolled["bg"], probe_still["bg"])
    assert probe_rolled["steps"] == probe_still["steps"] == rolled["steps"]


def check_supersampled(case, k, tag):
    """bhr_set_supersample's contract at factor k: the frame is, bit for bit, supersample_ref.box_resolve of the fine frame of
    the same call, takes its steps, and counts k^2 W H rays."""
    from supersample_ref import box_resolve
    w, h = case.size
    ss, fine = device_frame(case, supersample=k), device_frame(case, size=(k * w, k * h))
    for layer in ("bg", "disk"):
        want = box_resolve(fine[layer], k)
        bad = int((ss[layer] != want).any(axis=2).sum())
        print(f"[{tag}] {case.name} k={k} {layer}: {bad} of {w * h} pixels differ from the box filter of the {k * w} x {k * h} frame; "
              f"largest difference {np.abs(ss[layer].astype(np.float64) - want).max():.3g}")
        assert ss[layer].shape == (h, w, 3) and bad == 0, f"{layer}: {bad} pixels are not the box filter of the fine frame"
    assert ss["steps"] == fine["steps"] > 0
    assert ss["rays"] == k * k * w * h == fine["rays"]
    assert ss["disk"].max() > 0 and ss["bg"].max() > 0
    return ss, fine


def check_sky_clamps(case, tag):
    """observer_sky on against off: DISK and the steps are the same, BG differs, and the shifted BG is the plain BG times the
    reference's sky_shift factors of the pixel's D, to the frame bars -- the clamps of D to [0.1, 1.5] apart from the march."""
    r64, r32 = reference(case, np.float64), reference(case, np.float32)
    shifted, plain = device_frame(case), device_frame(case._replace(sky=False))
    assert np.array_equal(shifted["disk"], plain["disk"]) and shifted["steps"] == plain["steps"]
    apart = rmse(shifted["bg"], plain["bg"]).max()
    want = R.sky_shift(plain["bg"].astype(np.float64).reshape(-1, 3), r64["D"].reshape(-1)).reshape(plain["bg"].shape)
    d, d32 = rmse(shifted["bg"], want), rmse(r32["bg"], r64["bg"])
    bar = np.maximum(2.0 * d32, BAR_FLOOR)
    off = off_pixels((shifted["bg"],), (want,))
    seen = (r64["fate"] == 1) & r64["inside"]
    print(f"[{tag}] {case.name}: BG with the sky shifted is {apart:.3g} RMSE from the plain one, and {d} from the plain one times the reference's "
          f"factors (bar {bar}), {off} pixels off by more than 1e-3; D on the sky {r64['D'][seen].min():.4f} .. {r64['D'][seen].max():.3f}")
    assert apart > 1e-2
    assert (d <= bar).all() and off <= off_cap(case.pixels)
