"""Motion blur from the Kerr ray map (bhr_kerr_raymap_render_shutter; include/bhr.h states the frame): the BG and DISK layers are
the sequential f32 mean (tests/shutter_ref.py) of the layers its samples' single Kerr map frames store -- bhr_kerr_raymap_render_view
of a turned camera, bhr_kerr_raymap_render of the build pose -- and the post-pass is bhr_bloom's on the resolved layers.  Two routes
give those bits: one fused launch (a k = 1 map without overflow pixels, option "kerr_raymap_shutter_fused" not 0, n > 1) and, sample
by sample, the existing shade, fix and accumulation launches.  Every comparison here is for zero differing values.

Scene and constants: tests/kerr_cases.py.  The orbit: camera.orbit_position over 512 positions from pov (6, 0, 0.5), shutter 0.5,
disk speed 0.1, frames 0 and 5.  Frames: 61 x 43, 21 x 13 (partial tiles on both sides), 8 x 8 (one tile), 5 x 3 (less than one),
48 x 32 at fov 40 (rays with two crossings: overflow pixels with one slot), 64 x 40 (video)."""
import functools
import json
import os

import numpy as np
import pytest

import kerr_cases as KC
from shutter_ref import resolve

pytestmark = pytest.mark.gpu

KW = dict(step_size=KC.STEP, r_max=KC.R_MAX, r_disk_inner=KC.R_INNER, r_disk_outer=KC.R_OUTER, disk_tilt=0.0, anti_alias="disabled",
          disk_rotation_speed=0.1)
POV, FOV, N_ORBIT, S, SPEED = KC.VIEWS[0], KC.FOV, 512, 0.5, 0.1
LAYERS = ("final", "bg", "disk", "blur")
OPTION = "kerr_raymap_shutter_fused"


def _mk(A, redshift="model", force=False, width=21, height=13, math="strict", **kw):
    from bhr_amd import HipRenderer
    sky, tex = KC.scene()
    r = HipRenderer(width, height, sky, tex, math=math, **{**KW, **kw})
    if A != 0.0 or force:
        r.set_spin(A, force_kerr=force)
    if redshift == "exact":
        r.set_redshift("exact")
    return r


def _cam(k, pov=POV):
    from bhr_amd.camera import orbit_position
    return [float(v) for v in orbit_position(list(pov), k, N_ORBIT)]


def _read(r, names=LAYERS, u8=True):
    from bhr_amd import _lib
    ids = dict(final=_lib.LAYER_FINAL, bg=_lib.LAYER_BG, disk=_lib.LAYER_DISK, blur=_lib.LAYER_BLUR, hdr=_lib.LAYER_HDR)
    out = {k: r.read_layer(ids[k]) for k in names}
    if u8:
        out["u8"] = r.read_final_u8()
    return out


def _assert_equal(got, want, tag, names=LAYERS + ("u8",)):
    for k in names:
        bad = int((got[k] != want[k]).sum())
        assert bad == 0, f"{tag} {k}: {bad} values differ (max |d| {np.abs(got[k].astype(np.float64) - want[k]).max():.3g})"


def _orbit_samples(f, n, pov=POV):
    """What render_video's shutter loop hands frame f of the 512-position orbit: positions and t_offsets of its n samples."""
    from bhr_amd import drivers
    u = drivers.shutter_times(f, S, n)
    return [_cam(t, pov) for t in u], [(t - f) * SPEED for t in u]


def _bloom_of(r, layers, lens_flare=False):
    """bhr_bloom of the given BG and DISK in context r: FINAL, BLUR, u8 (and the layers back)."""
    from bhr_amd import _lib
    r.write_layer(_lib.LAYER_BG, layers["bg"])
    r.write_layer(_lib.LAYER_DISK, layers["disk"])
    r.bloom_only()
    if lens_flare:
        r.apply_lens_flare()
    return _read(r)


class Hole(tuple):
    """(A, redshift, force, W, H, fov, pov, r_inner, slots, k): what a context and its map are made of (hashable: the references are cached)."""
    def __new__(cls, A, redshift="model", force=False, W=21, H=13, fov=FOV, pov=POV, r_inner=KC.R_INNER, slots=None, k=1):
        return super().__new__(cls, (A, redshift, force, W, H, fov, tuple(pov), r_inner, slots, k))

    A, redshift, force, W, H, fov, pov, r_inner, slots, k = (property(lambda self, i=i: self[i]) for i in range(10))

    def renderer(self, **kw):
        opts = dict(kw.pop("options", {}))
        if self.slots is not None:
            opts["raymap_slots"] = self.slots
        return _mk(self.A, self.redshift, self.force, self.W, self.H, r_disk_inner=self.r_inner, options=opts, **kw)

    def build(self, r, still=False):
        r.build_kerr_ray_map(list(self.pov) if still else _cam(0, self.pov), self.fov, supersample=self.k)

    @property
    def tag(self):
        return f"A={self.A} {self.redshift} {self.W}x{self.H} K={self.slots} k={self.k}"


@functools.lru_cache(maxsize=None)
def _reference(hole, f, n, still=False):
    """The n single Kerr map frames of an exposure, rendered one by one on ONE other context, resolved on the host; and the sum of
    their overflow re-marches' steps.  still: the build camera itself at the orbit exposure's t_offsets."""
    r = hole.renderer()
    hole.build(r, still)
    pos, toff = _orbit_samples(f, n, hole.pov)
    singles, steps = [], 0
    for p, t in zip(pos, toff):
        r.render_from_kerr_ray_map_async(t_offset=t, cam_pos=None if still else p, skip_bloom=True)
        singles.append(_read(r, ("bg", "disk"), u8=False))
        steps += r.counters()["ray_steps"]
    r.close()
    out = {k: resolve([s[k] for s in singles]) for k in ("bg", "disk")}
    for a in out.values():
        a.setflags(write=False)
    out["steps"] = steps
    out["differ"] = n > 1 and bool((singles[0]["bg"] != singles[-1]["bg"]).any() and (singles[0]["disk"] != singles[-1]["disk"]).any())
    return out


def _composition(hole, n, fused, frames=(0, 5), still=False):
    r = hole.renderer(options={OPTION: fused})
    hole.build(r, still)
    info = r.kerr_ray_map_info()
    for f in frames:
        tag = f"{hole.tag} n={n} f={f} fused={fused} still={still}"
        want = _reference(hole, f, n, still)
        pos, toff = _orbit_samples(f, n, hole.pov)
        if f == 0 and n == 3 and not still:
            assert pos[1] == _cam(0, hole.pov) and toff[1] == 0.0      # a sample exactly at the build camera, inside a ROT launch
        timed = r.counters()["frames_timed"]
        r.render_shutter_from_kerr_ray_map_async(toff, None if still else pos, skip_bloom=True)
        got = _read(r, ("bg", "disk"), u8=False)
        c = r.counters()
        _assert_equal(got, want, tag, ("bg", "disk"))
        assert want["differ"] == (n > 1), tag                           # the samples really differ: the test can fail
        assert c["rays"] == n * hole.k * hole.k * hole.W * hole.H and c["frames_timed"] == timed + 1     # one entry in the timing ring
        assert c["ray_steps"] == want["steps"], tag
        assert (c["ray_steps"] > 0) == (info["overflow_pixels"] > 0)
        # with the post-pass: BG / DISK unchanged, and the rest is bhr_bloom of the resolved layers in this context
        r.render_shutter_from_kerr_ray_map_async(toff, None if still else pos)
        full = _read(r)
        _assert_equal(full, want, tag + " bloom", ("bg", "disk"))
        _assert_equal(full, _bloom_of(r, want), tag + " bloom")
        assert (full["disk"] > 0).any() and (full["bg"] > 0).any()
    r.close()
    return info


# ---- 1. orbit exposures against the host-resolved single frames ---------------------------------------------------------------
ORBIT = [(21, 13, 0.6, "model", False, 3), (21, 13, 0.6, "exact", False, 2), (21, 13, -0.9, "model", False, 8), (21, 13, -0.9, "exact", False, 3),
         (21, 13, 0.998, "model", False, 2), (21, 13, 0.998, "exact", False, 8), (21, 13, 0.0, "model", True, 3), (21, 13, 0.6, "model", False, 1),
         (61, 43, 0.6, "model", False, 3), (61, 43, -0.9, "exact", False, 8), (61, 43, 0.998, "exact", False, 1),
         (8, 8, 0.998, "exact", False, 2), (8, 8, 0.6, "model", False, 3), (5, 3, 0.6, "model", False, 1), (5, 3, -0.9, "exact", False, 3),
         (5, 3, 0.998, "model", False, 8)]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("W, H, A, redshift, force, n", ORBIT, ids=lambda v: str(v))
def test_orbit_exposure_is_the_mean_of_its_kerr_map_frames(W, H, A, redshift, force, n, fused, hip_lib):
    info = _composition(Hole(A, redshift, force, W, H), n, fused)
    assert info["overflow_pixels"] == 0 and info["supersample"] == 1 and info["redshift"] == redshift


@pytest.mark.parametrize("fused", [1, 0])
def test_sixty_four_samples(fused, hip_lib):
    _composition(Hole(0.6, "exact"), 64, fused, frames=(5,))


# ---- 2. still camera against code this change does not touch ------------------------------------------------------------------
def _still_frames(n):
    """Frame numbers whose float32(frame * 0.1) are the samples' t_offsets: the marched frame takes a frame number."""
    return [40 + 3 * j for j in range(n)]


def _t_of(frame):
    return float(np.float32(float(frame) * SPEED))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("n", [2, 5])
@pytest.mark.parametrize("A, redshift", [(0.6, "model"), (-0.9, "exact")])
def test_still_exposure_is_the_mean_of_marched_kerr_frames(A, redshift, n, fused, hip_lib):
    W, H = 48, 32
    r = _mk(A, redshift, width=W, height=H, options={OPTION: fused})
    marched = []
    for f in _still_frames(n):
        r.render_async(list(POV), FOV, frame=f, skip_bloom=True)
        marched.append(_read(r, ("bg", "disk"), u8=False))
    want = {k: resolve([m[k] for m in marched]) for k in ("bg", "disk")}
    assert (marched[0]["disk"] != marched[-1]["disk"]).any()         # the roll shows
    r.build_kerr_ray_map(list(POV), FOV)
    assert r.kerr_ray_map_info()["overflow_pixels"] == 0
    r.render_shutter_from_kerr_ray_map_async([_t_of(f) for f in _still_frames(n)])
    got = _read(r)
    tag = f"A={A} {redshift} n={n} fused={fused}"
    _assert_equal(got, want, tag, ("bg", "disk"))
    _assert_equal(got, _bloom_of(r, want), tag + " post-pass")
    r.close()
    assert (got["disk"] > 0).any() and (got["bg"] > 0).any() and got["blur"].max() > 0.0


@pytest.mark.parametrize("fused", [1, 0])
def test_lens_flare_under_a_grade_with_the_hdr_plane(fused, hip_lib):
    """Two samples at one and the same t_offset: (L + L) * 0.5 is L exactly, so the exposure is the marched Kerr frame of that
    t_offset in every layer -- with the lens flare, under a grade that keeps the HDR plane."""
    W, H, frame = 48, 32, 73
    r = _mk(0.6, "exact", width=W, height=H, options={OPTION: fused})
    r.build_kerr_ray_map(list(POV), FOV)
    r.render_async(list(POV), FOV, frame=frame, lens_flare=False)
    plain = _read(r)
    r.set_grade("aces", exposure=1.0, transfer="srgb", keep_hdr=True)
    names = LAYERS + ("hdr",)
    r.render_async(list(POV), FOV, frame=frame, lens_flare=True)
    want = _read(r, names)
    r.render_async(list(POV), FOV, frame=frame, lens_flare=False)
    no_flare = _read(r, names)
    r.render_shutter_from_kerr_ray_map_async([_t_of(frame)] * 2, lens_flare=True)
    got = _read(r, names)
    r.close()
    _assert_equal(got, want, f"flare + grade fused={fused}", names + ("u8",))
    assert (want["final"] != no_flare["final"]).any() and (no_flare["final"] != plain["final"]).any()      # the flare and the grade are there


@pytest.mark.parametrize("fused", [1, 0])
def test_hybrid_context_gets_its_own_post_pass(fused, hip_lib):
    hole, n, f = Hole(0.6, "model", W=61, H=43), 3, 5
    want = _reference(hole, f, n)
    pos, toff = _orbit_samples(f, n)
    r = hole.renderer(math="hybrid", options={OPTION: fused})
    hole.build(r)
    r.render_shutter_from_kerr_ray_map_async(toff, pos)
    got = _read(r)
    buf = np.empty(16, dtype=np.uint8)                           # the frame went through the split-f16 post-pass: its operands exist
    assert hip_lib.bhr_debug_read(r._ctx, 0, buf.ctypes.data, buf.nbytes, None) == 0, hip_lib.bhr_last_error()
    _assert_equal(got, want, f"hybrid fused={fused}", ("bg", "disk"))
    _assert_equal(got, _bloom_of(r, want), f"hybrid fused={fused} post-pass")
    r.close()
    assert got["blur"].max() > 0.0


@pytest.mark.parametrize("fused", [1, 0])
def test_frames_on_two_slots_equal_one_slot(fused, hip_lib):
    """Four shutter frames in a row, alternating with plain Kerr map frames: every frame of the two-slot context equals the same
    frame of a fresh one-slot context -- no shared or stale sums."""
    hole = Hole(-0.9, "exact", W=61, H=43)

    def sequence(slots):
        r = hole.renderer(math="hybrid", frame_slots=slots, options={OPTION: fused})
        assert r.frame_slots == slots
        hole.build(r)
        frames = []
        for k, n in enumerate((5, 2, 8, 3)):
            pos, toff = _orbit_samples(10 * k + 3, n)
            r.render_shutter_from_kerr_ray_map_async(toff, pos)
            frames.append(_read(r))
            r.render_from_kerr_ray_map_async(frame=k, cam_pos=_cam(7 * k))
            frames.append(_read(r))
        r.close()
        return frames

    one, two = sequence(1), sequence(2)
    for k, (g, w) in enumerate(zip(two, one)):
        _assert_equal(g, w, f"frame {k} fused={fused}")
    assert (two[0]["final"] != two[2]["final"]).any() and (two[0]["final"] != two[1]["final"]).any()


# ---- 3. overflow ----------------------------------------------------------------------------------------------------------------
def _crossings_hole(slots):
    e = KC.CROSSINGS[0]                                          # A 0.998, fov 40, r_inner 0.7: rays that cross the annulus twice
    return Hole(e.A, "model", W=48, H=32, fov=e.fov, pov=e.view, r_inner=e.r_inner, slots=slots)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("slots", [1, 8])
def test_map_with_overflow_pixels(slots, n, fused, hip_lib):
    info = _composition(_crossings_hole(slots), n, fused)
    assert info["slots"] == slots and (info["overflow_pixels"] > 0) == (slots == 1)


# ---- 4. supersampled maps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("still", [False, True], ids=["orbit", "still"])
@pytest.mark.parametrize("k, W, H, A, redshift", [(2, 21, 13, 0.6, "model"), (4, 12, 8, -0.9, "exact")])
def test_supersampled_map_resolves_each_sample_then_takes_the_mean(k, W, H, A, redshift, still, fused, hip_lib):
    # eight slots: no group of either context is on an overflow list
    info = _composition(Hole(A, redshift, W=W, H=H, slots=8, k=k), 3, fused, still=still)
    assert info["supersample"] == k and info["overflow_pixels"] == 0


# ---- 5. which route ran ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what, fused, launches", [("plain", None, 0), ("plain", 1, 0), ("plain", 0, 3), ("overflow", 1, 3), ("overflow", 0, 3),
                                                   ("k2", 1, 3), ("k2", 0, 3)])
def test_which_route_ran(what, fused, launches, hip_lib):
    """The two routes give the same bits, so the frames cannot tell which one ran.  The accumulation launches can: under option
    "shutter_timing" every one of them is bracketed and counted (bhr_debug_read, which = 5), the sample-by-sample route has n of
    them and the fused launch none.  A k = 1 map without overflow pixels takes the fused launch unless the option says 0 (None:
    the option as bhr_create leaves it); a map with overflow pixels and a supersampled map never do."""
    n = 3
    hole = {"plain": Hole(0.6, "model", W=61, H=43), "overflow": _crossings_hole(1), "k2": Hole(0.6, "model", k=2)}[what]
    r = hole.renderer(options={"shutter_timing": 1, **({} if fused is None else {OPTION: fused})})
    hole.build(r)
    info = r.kerr_ray_map_info()
    assert (info["overflow_pixels"] > 0) == (what == "overflow") and info["supersample"] == hole.k
    pos, toff = _orbit_samples(5, n, hole.pov)
    if what == "plain" and fused == 1:                           # an unfused frame first: its count must not linger
        r.set_option(OPTION, 0)
        r.render_shutter_from_kerr_ray_map_async(toff, pos)
        assert r.shutter_timing()["launches"] == n
        r.set_option(OPTION, 1)
    r.render_shutter_from_kerr_ray_map_async(toff, pos)
    assert r.shutter_timing()["launches"] == launches
    r.render_shutter_from_kerr_ray_map_async(toff[:1], pos[:1])   # one sample: the one map frame, nothing to accumulate
    assert r.shutter_timing()["launches"] == 0
    r.close()


def test_option_default_and_environment(hip_lib):
    n = 3
    hole = Hole(0.6, "model")
    pos, toff = _orbit_samples(5, n)
    saved = os.environ.get("BHR_KERR_RAYMAP_SHUTTER_FUSED")
    os.environ["BHR_KERR_RAYMAP_SHUTTER_FUSED"] = "0"
    try:
        r = hole.renderer(options={"shutter_timing": 1})         # read once by bhr_create
    finally:
        if saved is None:
            os.environ.pop("BHR_KERR_RAYMAP_SHUTTER_FUSED", None)
        else:
            os.environ["BHR_KERR_RAYMAP_SHUTTER_FUSED"] = saved
    hole.build(r)
    r.render_shutter_from_kerr_ray_map_async(toff, pos)
    assert r.shutter_timing()["launches"] == n
    r.set_option("raymap_shutter_fused", 1)                      # the Schwarzschild map's option is not this one
    r.render_shutter_from_kerr_ray_map_async(toff, pos)
    assert r.shutter_timing()["launches"] == n
    r.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_context_usable(hip_lib):
    from bhr_amd import _lib
    lib = hip_lib
    n, A = 5, 0.6
    r = _mk(A)
    pos, toff = _orbit_samples(5, n)

    def cams_of(positions, offsets, count=None):
        cams = (_lib.Camera * (count or len(positions)))()
        for j, (p, t) in enumerate(zip(positions, offsets)):
            cams[j] = r.camera_uniforms(p, FOV, t_offset=t)
        return cams

    good = cams_of(pos, toff)

    def refused(ctx, cams, count, flags, code, *words):
        rc = lib.bhr_kerr_raymap_render_shutter(ctx, cams, count, flags)
        assert rc == code, (rc, lib.bhr_last_error())
        assert b"bhr_kerr_raymap_render_shutter" in lib.bhr_last_error()
        for word in words:
            assert word in lib.bhr_last_error(), lib.bhr_last_error()

    refused(r._ctx, good, n, 0, _lib.BHR_ERR_STATE, b"no Kerr ray map")      # before a build
    r.build_kerr_ray_map(_cam(0), FOV)
    r.render_from_kerr_ray_map_async(frame=5)
    want = _read(r)

    def still_renders():
        before = r.counters()["frames_timed"]
        r.render_from_kerr_ray_map_async(frame=5)
        _assert_equal(_read(r), want, "after a refusal")
        return before

    frames = still_renders()
    big = cams_of([pos[j % n] for j in range(65)], [0.01 * j for j in range(65)])
    for count in (0, 65, -1):
        refused(r._ctx, big, count, 0, _lib.BHR_ERR_INVALID, b"samples")
    for flags in (_lib.SKIP_DIFFERENTIALS, _lib.PERSISTENT, _lib.FORCE_FAST, _lib.ROW_COSTS):
        refused(r._ctx, good, n, flags, _lib.BHR_ERR_INVALID, b"flags")
    refused(r._ctx, None, n, 0, _lib.BHR_ERR_INVALID, b"null")
    refused(None, good, n, 0, _lib.BHR_ERR_INVALID, b"null")
    nan = cams_of(pos, toff)
    nan[3].t_offset = float("nan")
    refused(r._ctx, nan, n, 0, _lib.BHR_ERR_INVALID, b"sample 3: t_offset")
    inf = cams_of(pos, toff)
    inf[4].t_offset = float("inf")
    refused(r._ctx, inf, n, 0, _lib.BHR_ERR_INVALID, b"sample 4: t_offset")
    high = cams_of(pos[:2] + [_cam(5, pov=(6.0, 0.0, 0.6))] + pos[3:], toff)               # sample 2 at another height
    refused(r._ctx, high, n, 0, _lib.BHR_ERR_INVALID, b"sample 2", b"height")
    far = cams_of(pos[:4] + [[7.0, 0.0, 0.5]], toff)                                       # sample 4 at another distance from the axis
    refused(r._ctx, far, n, 0, _lib.BHR_ERR_INVALID, b"sample 4")
    # a Kerr polarisation: a mean of frames has no Stokes planes
    r.set_kerr_polarization("toroidal")
    refused(r._ctx, good, n, 0, _lib.BHR_ERR_STATE, b"bhr_set_kerr_polarization")
    r.set_kerr_polarization(None)
    # the context's own supersampling
    r.set_supersample(2)
    refused(r._ctx, good, n, 0, _lib.BHR_ERR_INVALID, b"supersampling")
    r.set_supersample(1)
    assert r.counters()["frames_timed"] == frames + 1          # nothing but still_renders' frame was launched
    still_renders()
    # the spin or the redshift changed since the build
    frames = r.counters()["frames_timed"]
    r.set_spin(0.7)
    refused(r._ctx, good, n, 0, _lib.BHR_ERR_STATE, b"spin")
    r.set_spin(A)
    r.set_redshift("exact")
    refused(r._ctx, good, n, 0, _lib.BHR_ERR_STATE, b"redshift")
    r.set_redshift("model")
    assert r.counters()["frames_timed"] == frames
    still_renders()
    # the Python surface maps the codes as everywhere else
    with pytest.raises(ValueError):
        r.render_shutter_from_kerr_ray_map_async(toff, pos[:2] + [_cam(5, pov=(6.0, 0.0, 0.6))] + pos[3:])
    with pytest.raises(ValueError):
        r.render_shutter_from_kerr_ray_map_async(toff, pos[:2])                # mismatched lengths
    with pytest.raises(ValueError):
        r.render_shutter_from_kerr_ray_map_async([])                           # no sample
    # the two old entry points refuse the combination as before
    frames = r.counters()["frames_timed"]
    assert lib.bhr_render_shutter(r._ctx, good, n, 0) == _lib.BHR_ERR_INVALID
    assert b"bhr_render_shutter" in lib.bhr_last_error() and b"shutter frames march Schwarzschild rays" in lib.bhr_last_error()
    assert lib.bhr_raymap_render_shutter(r._ctx, good, n, 0) == _lib.BHR_ERR_INVALID
    assert b"bhr_raymap_render_shutter" in lib.bhr_last_error() and b"a ray map holds Schwarzschild rays" in lib.bhr_last_error()
    assert r.counters()["frames_timed"] == frames
    r.free_kerr_ray_map()
    refused(r._ctx, good, n, 0, _lib.BHR_ERR_STATE, b"no Kerr ray map")
    r.build_kerr_ray_map(_cam(0), FOV)
    still_renders()
    r.render_shutter_from_kerr_ray_map_async(toff, pos)         # ... and the exposure itself works on this context
    assert np.isfinite(_read(r)["final"]).all()
    r.close()


# ---- 7. video drivers -----------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


@pytest.mark.parametrize("orbit, k", [(False, 1), (True, 1), (False, 2)], ids=["still", "orbit", "still-k2"])
def test_video_frames_are_the_method_called_with_the_drivers_samples(orbit, k, tmp_path, hip_lib):
    """render_video(spin_shutter_map=True): every frame file holds the u8 rows of render_shutter_from_kerr_ray_map_async called with
    shutter_times' positions and t_offsets, on a context driven through the same lifecycle steps."""
    from bhr_amd import drivers
    from bhr_amd.camera import orbit_position
    W, H, N, NS = 64, 40, 4, 3
    cam0, deg = list(POV), 90.0
    out = str(tmp_path / "v" / "v.mp4")
    extra = {} if k == 1 else {"spin_map_supersample": k}
    r = _mk(0.6, width=W, height=H)
    drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=out, fov=FOV, static_cam_pos=cam0, orbit=orbit, orbit_degrees=deg,
                         disk_rotation_speed=SPEED, video_stream="off", assemble=False, shutter=S, shutter_samples=NS, spin_shutter_map=True, **extra)
    assert r.kerr_ray_map_info()["built"] == 0                   # freed at the end
    r.close()
    d = drivers._frames_dir(out)
    with open(os.path.join(d, "progress.json")) as fh:
        params = json.load(fh)["params"]
    assert params["spin_shutter_map"] is True and params.get("spin_map_supersample", 1) == k and "spin_map" not in params

    r = _mk(0.6, width=W, height=H)
    r.set_outputs("u8")
    factories = drivers.init_lifecycle_system(r, r.dtex_h, r.dtex_w, seed=42)
    r.build_kerr_ray_map(orbit_position(cam0, 0, N, deg) if orbit else cam0, FOV, supersample=k)
    assert r.kerr_ray_map_info()["supersample"] == k
    frames = []
    for f in range(N):
        drivers.advance_lifecycle_frame(r, factories, f * SPEED, SPEED, recompute_stats=(f % 60 == 0), compose=True)
        times = drivers.shutter_times(f, S, NS)
        toff = [(u - f) * SPEED for u in times]
        r.render_shutter_from_kerr_ray_map_async(toff, [orbit_position(cam0, u, N, deg) for u in times] if orbit else None)
        frames.append(r.read_final_u8())
    r.close()
    for f in range(N):
        np.testing.assert_array_equal(_png(os.path.join(d, f"frame_{f:04d}.png")), frames[f], err_msg=f"frame {f}")
    assert (frames[0] != frames[N - 1]).any()
