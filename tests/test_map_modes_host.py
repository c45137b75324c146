"""A video's map as one mode (drivers.render_video; ray_map, orbit_map, shutter_map, spin_map): every refusal of the five map
checks, whole and in order; the calls render_video makes on the renderer, against a recording; and the clean-up when a frame
raises.  No device is touched: the renderer, the frame sink and the lifecycle system are fakes that write one log.

The recording (tests/golden/render_video_map_calls.json) is this module's own: `python tests/test_map_modes_host.py` writes it."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_video_map_calls.json")


# ---- 1. every refusal, whole ----------------------------------------------------------------------------------------------------------
# (check, keywords that reach the refusal first, the message)
REFUSALS = [
    ("check_ray_map", dict(orbit=True), "a ray map is one view: --ray_map does not combine with --orbit"),
    ("check_ray_map", dict(shutter=0.5), "shutter frames are marched: --ray_map does not combine with --shutter"),
    ("check_ray_map", dict(supersample=2), "a ray map holds one ray per pixel: --ray_map does not combine with --supersample > 1"),
    ("check_ray_map", dict(disk_model="v2"), "a ray map shades the disk texture: --ray_map does not combine with --disk_model v2 / v2_volume"),
    ("check_ray_map", dict(gpus=2), "a ray map lives on one GPU: --ray_map does not combine with --gpus > 1 or several ranks"),
    ("check_ray_map", dict(world=2), "a ray map lives on one GPU: --ray_map does not combine with --gpus > 1 or several ranks"),
    ("check_orbit_map", dict(video=False), "--orbit_map needs --video: it is the ray map of an orbit video"),
    ("check_orbit_map", dict(orbit=False), "--orbit_map needs --orbit: a camera that stands still takes --ray_map"),
    ("check_orbit_map", dict(ray_map=True), "--orbit_map does not combine with --ray_map: that is the map of a camera that stands still"),
    ("check_orbit_map", dict(disk_tilt=20.0), "the orbit is a symmetry of an untilted disk only: --orbit_map needs --disk_tilt 0"),
    ("check_orbit_map", dict(shutter=0.5), "shutter frames are marched: --orbit_map does not combine with --shutter"),
    ("check_orbit_map", dict(supersample=4), "a ray map holds one ray per pixel: --orbit_map does not combine with --supersample > 1"),
    ("check_orbit_map", dict(disk_model="v2_volume"), "a ray map shades the disk texture: --orbit_map does not combine with --disk_model v2 / v2_volume"),
    ("check_orbit_map", dict(gpus=2), "a ray map lives on one GPU: --orbit_map does not combine with --gpus > 1 or several ranks"),
    ("check_orbit_map", dict(world=3), "a ray map lives on one GPU: --orbit_map does not combine with --gpus > 1 or several ranks"),
    ("check_shutter_map", dict(shutter=0.0), "--shutter_map needs --shutter > 0: an instantaneous exposure takes --ray_map or --orbit_map"),
    ("check_shutter_map", dict(ray_map=True), "--shutter_map does not combine with --ray_map: that is the map of an instantaneous exposure"),
    ("check_shutter_map", dict(orbit_map=True), "--shutter_map does not combine with --orbit_map: that is the map of an instantaneous exposure"),
    ("check_shutter_map", dict(orbit=True, disk_tilt=-0.5), "the orbit is a symmetry of an untilted disk only: --shutter_map with --orbit needs --disk_tilt 0"),
    ("check_shutter_map", dict(supersample=2), "a ray map holds one ray per pixel: --shutter_map does not combine with --supersample > 1"),
    ("check_shutter_map", dict(disk_model="v2"), "a ray map shades the disk texture: --shutter_map does not combine with --disk_model v2 / v2_volume"),
    ("check_shutter_map", dict(gpus=2), "a ray map lives on one GPU: --shutter_map does not combine with --gpus > 1 or several ranks"),
    ("check_shutter_map", dict(world=2), "a ray map lives on one GPU: --shutter_map does not combine with --gpus > 1 or several ranks"),
    ("check_spin_map", dict(spin=0.0, redshift="model"), "--spin_map needs --spin or --redshift exact: it is the ray map of the Kerr march; a hole that does "
     "not spin takes --ray_map or --orbit_map"),
    ("check_spin_map", dict(video=False), "--spin_map needs --video: it is the ray map of a video"),
    ("check_spin_map", dict(shutter=0.25), "shutter frames are marched: --spin_map does not combine with --shutter"),
    ("check_spin_map", dict(supersample=2), "a Kerr ray map holds one ray per pixel: --spin_map does not combine with --supersample > 1"),
    ("check_spin_map", dict(supersample=None), "a Kerr ray map holds one ray per pixel: --spin_map does not combine with --supersample > 1"),
    ("check_spin_map", dict(map_supersample=2), "a Kerr ray map has no supersampled form: --spin_map does not combine with --map_supersample > 1"),
    ("check_spin_map", dict(gpus=2), "a ray map lives on one GPU: --spin_map does not combine with --gpus > 1 or several ranks"),
    ("check_spin_map", dict(world=2), "a ray map lives on one GPU: --spin_map does not combine with --gpus > 1 or several ranks"),
    ("check_spin_map", dict(ray_map=True), "--spin_map does not combine with --ray_map: that is a map of Schwarzschild rays"),
    ("check_spin_map", dict(orbit_map=True), "--spin_map does not combine with --orbit_map: that is a map of Schwarzschild rays"),
    ("check_spin_map", dict(shutter_map=True), "--spin_map does not combine with --shutter_map: that is a map of Schwarzschild rays"),
    ("check_spin_map", dict(observer=True), "--spin_map does not combine with --observer: the observer march is Schwarzschild's"),
    ("check_spin_map", dict(projection=True), "--spin_map does not combine with --projection: the projected march is Schwarzschild's"),
    ("check_spin_map", dict(light_delay=True), "--spin_map does not combine with --light_delay: the delayed march is Schwarzschild's"),
    ("check_spin_map", dict(stars=True), "--spin_map does not combine with --stars point: point stars are rendered through the map of Schwarzschild rays"),
    ("check_spin_map", dict(polarization=True), "--spin_map does not combine with --polarization: the transport rule is Schwarzschild's"),
]
# two conditions violated at once: the refusal is the one the check names first
ORDER = [
    ("check_ray_map", dict(orbit=True, shutter=0.5, world=2), "a ray map is one view: --ray_map does not combine with --orbit"),
    ("check_ray_map", dict(supersample=2, disk_model="v2"), "a ray map holds one ray per pixel: --ray_map does not combine with --supersample > 1"),
    ("check_orbit_map", dict(orbit=False, video=False), "--orbit_map needs --video: it is the ray map of an orbit video"),
    ("check_orbit_map", dict(disk_tilt=5.0, ray_map=True), "--orbit_map does not combine with --ray_map: that is the map of a camera that stands still"),
    ("check_orbit_map", dict(gpus=2, shutter=0.5), "shutter frames are marched: --orbit_map does not combine with --shutter"),
    ("check_shutter_map", dict(shutter=0, ray_map=True), "--shutter_map needs --shutter > 0: an instantaneous exposure takes --ray_map or --orbit_map"),
    ("check_shutter_map", dict(orbit_map=True, orbit=True, disk_tilt=3.0), "--shutter_map does not combine with --orbit_map: that is the map of an instantaneous exposure"),
    ("check_shutter_map", dict(disk_model="v2", supersample=2), "a ray map holds one ray per pixel: --shutter_map does not combine with --supersample > 1"),
    ("check_spin_map", dict(spin=0.0, video=False), "--spin_map needs --spin or --redshift exact: it is the ray map of the Kerr march; a hole that does not "
     "spin takes --ray_map or --orbit_map"),
    ("check_spin_map", dict(map_supersample=2, supersample=2), "a Kerr ray map holds one ray per pixel: --spin_map does not combine with --supersample > 1"),
    ("check_spin_map", dict(polarization=True, shutter_map=True), "--spin_map does not combine with --shutter_map: that is a map of Schwarzschild rays"),
    ("check_spin_map", dict(stars=True, observer=True, world=2), "a ray map lives on one GPU: --spin_map does not combine with --gpus > 1 or several ranks"),
]


def _call_check(name, kw):
    from bhr_amd import drivers
    if name == "check_spin_map":                              # its defaults refuse (no spin): the good call has one
        kw = {"spin": 0.6, **kw}
    getattr(drivers, name)(True, **kw)


@pytest.mark.parametrize("name, kw, message", REFUSALS + ORDER, ids=lambda v: None if isinstance(v, str) and " " in v else str(v).replace(" ", ""))
def test_a_map_check_refuses_with_the_whole_message(name, kw, message):
    with pytest.raises(ValueError) as e:
        _call_check(name, kw)
    assert str(e.value) == message


@pytest.mark.parametrize("k, kw, message", [
    (3, {}, "map_supersample must be 1, 2, 4 or 8, got 3"), (True, {}, "map_supersample must be 1, 2, 4 or 8, got True"),
    (2.0, dict(ray_map=True), "map_supersample must be 1, 2, 4 or 8, got 2.0"),
    (2, {}, "--map_supersample is a ray map's factor: it needs --ray_map, --orbit_map or --shutter_map (marched frames take --supersample)"),
    (16, {}, "map_supersample must be 1, 2, 4 or 8, got 16")])            # both violated: the value first
def test_check_map_supersample_refuses_with_the_whole_message(k, kw, message):
    from bhr_amd import drivers
    with pytest.raises(ValueError) as e:
        drivers.check_map_supersample(k, **kw)
    assert str(e.value) == message


def test_the_map_checks_accept_what_they_accepted():
    from bhr_amd import drivers
    for name in ("check_ray_map", "check_orbit_map", "check_shutter_map", "check_spin_map"):
        assert getattr(drivers, name)(False, supersample=4, gpus=3, world=2) is None      # off: nothing is checked
        assert _call_check(name, {}) is None
    assert drivers.check_ray_map(True, supersample=None) is None and drivers.check_spin_map(True, redshift="exact") is None
    for k, kw in ((1, {}), (2, dict(ray_map=True)), (4, dict(orbit_map=True)), (8, dict(shutter_map=True))):
        assert drivers.check_map_supersample(k, **kw) is None


# ---- 2. render_video on a renderer that records ---------------------------------------------------------------------------------------
def _plain(v):
    if isinstance(v, np.ndarray):
        return f"ndarray{list(v.shape)}"
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (np.floating, np.integer)):
        return v.item()
    return v


class Raised(Exception):
    pass


class Recorder:
    """A renderer that does nothing but write down what it is asked: [name, args, kwargs] per call, settings as attributes.
    raise_in: (method, n) -- the n-th call of that method raises Raised."""
    supersample = 1
    supersample_threshold = None
    disk_tilt = 0.0
    anti_alias = "disabled"
    _dv2 = None
    outputs = "f32"
    dither = "none"
    grade = None
    dtex_h, dtex_w = 4, 8
    _RETURNS = dict(ray_map_info=dict(slots=4, overflow_pixels=7, device_bytes=12_000_000),
                    kerr_ray_map_info=dict(slots=4, overflow_pixels=3, device_bytes=5_000_000, spin=0.6, redshift="model"),
                    stars_info=dict(n=0))

    def __init__(self, spin=0.0, redshift="model", raise_in=None):
        self.spin, self.redshift, self.raise_in = spin, redshift, raise_in
        self.log, self.counts = [], {}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*args, **kw):
            self.log.append([name, _plain(args), _plain(kw)])
            self.counts[name] = self.counts.get(name, 0) + 1
            if self.raise_in == (name, self.counts[name]):
                raise Raised(name)
            if name == "stokes_cells":
                return np.zeros((2, 3, 3), dtype=np.float32)
            return self._RETURNS.get(name)
        return call


def _patch(monkeypatch, log):
    """The driver's device-side helpers write into the renderer's log: the frame sink and the lifecycle system."""
    from bhr_amd import drivers

    class Sink:
        workers = 0

        def __init__(self, renderer, **kw):
            log.append(["FrameSink", [], _plain(kw)])

        def submit(self, path):
            log.append(["sink.submit", [os.path.basename(path)], {}])

        def drain(self):
            log.append(["sink.drain", [], {}])
            return 0, 0

        def close(self):
            log.append(["sink.close", [], {}])
    monkeypatch.setattr(drivers, "FrameSink", Sink)
    monkeypatch.setattr(drivers, "init_lifecycle_system", lambda renderer, n_r, n_phi, seed=42: log.append(["init_lifecycle_system", [n_r, n_phi], {}]) or {})
    monkeypatch.setattr(drivers, "advance_lifecycle_frame",
                        lambda renderer, factories, t, dt, **kw: log.append(["advance_lifecycle_frame", [t, dt], _plain(kw)]))


POV = [6.0, 0.0, 0.5]
SHUTTER = dict(shutter=0.5, shutter_samples=3)
# name -> (the renderer's spin, render_video's keywords): each mode, with and without an orbit where the mode takes one
RUNS = {
    "marched": (0.0, {}), "marched_orbit": (0.0, dict(orbit=True)),
    "ray_map": (0.0, dict(ray_map=True)), "ray_map_ss2": (0.0, dict(ray_map=True, map_supersample=2)),
    "ray_map_polarization": (0.0, dict(ray_map=True, polarization=dict(field="toroidal"))),
    "orbit_map": (0.0, dict(orbit=True, orbit_map=True)),
    "shutter_map": (0.0, dict(shutter_map=True, **SHUTTER)), "shutter_map_orbit": (0.0, dict(orbit=True, shutter_map=True, **SHUTTER)),
    "shutter_marched": (0.0, dict(**SHUTTER)),
    "spin_map": (0.6, dict(spin_map=True)), "spin_map_orbit": (0.6, dict(orbit=True, spin_map=True)),
}
# what a run restores on return: a JPEG video (the outputs), a dither and a grade that are not the renderer's
RESTORES = dict(video_codec="mjpeg", dither="blue", grade=dict(tonemap="reinhard", exposure=1.0))


def _run(monkeypatch, tmp_path, renderer, kw, n_frames=4):
    """render_video(**kw) on `renderer`: -> its log and the lines the builds printed."""
    from bhr_amd import drivers
    _patch(monkeypatch, renderer.log)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        drivers.render_video(renderer, 48, 27, n_frames, 24, os.path.join(str(tmp_path), "v.mp4"), 90.0, POV, video_stream="off", assemble=False, **kw)
    return renderer.log, [line for line in out.getvalue().splitlines() if "map built" in line]


@pytest.mark.parametrize("name", list(RUNS))
def test_render_video_calls_the_renderer_as_recorded(name, monkeypatch, tmp_path):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    spin, kw = RUNS[name]
    log, printed = _run(monkeypatch, tmp_path, Recorder(spin), kw)
    assert printed == want["printed"]
    got = json.loads(json.dumps(log))
    for n, (g, w) in enumerate(zip(got, want["calls"])):
        assert g == w, f"{name}: call {n} is {g}, recorded {w}"
    assert len(got) == len(want["calls"])


# the frame call of each mode, and the free of its map
MODES = {"ray_map": ("render_from_ray_map_async", "free_ray_map"), "ray_map_polarization": ("render_from_ray_map_async", "free_ray_map"),
         "orbit_map": ("render_from_ray_map_async", "free_ray_map"), "shutter_map": ("render_shutter_from_ray_map_async", "free_ray_map"),
         "shutter_map_orbit": ("render_shutter_from_ray_map_async", "free_ray_map"),
         "spin_map": ("render_from_kerr_ray_map_async", "free_kerr_ray_map"), "spin_map_orbit": ("render_from_kerr_ray_map_async", "free_kerr_ray_map")}
SETTERS = ("free_ray_map", "free_kerr_ray_map", "set_dither", "set_grade", "set_outputs", "set_polarization")


@pytest.mark.parametrize("name", list(MODES))
def test_render_video_cleans_up_when_a_frame_raises(name, monkeypatch, tmp_path):
    """The third frame's call raises: the map is freed once, and dither, grade, outputs and polarisation are set back exactly as
    on a clean return.  (The one test of this module that fails on the commit before the maps became one mode: there the frees
    and the three restores came behind the loop and were skipped when it raised.)"""
    spin, kw = RUNS[name]
    frame_call, free = MODES[name]
    kw = dict(kw, **RESTORES)
    clean, _ = _run(monkeypatch, tmp_path / "clean", Recorder(spin), kw)
    r = Recorder(spin, raise_in=(frame_call, 3))
    with pytest.raises(Raised):
        _run(monkeypatch, tmp_path / "raised", r, kw)
    raised = r.log
    settings = lambda log: [c for c in log if c[0] in SETTERS]
    assert [c[0] for c in raised].count(frame_call) == 3 and [c[0] for c in clean].count(frame_call) == 4
    assert [c[0] for c in raised].count(free) == 1
    assert {"set_dither", "set_grade", "set_outputs"} <= {c[0] for c in clean} and (name != "ray_map_polarization" or ["set_polarization", [None], {}] in clean)
    assert settings(raised) == settings(clean)


if __name__ == "__main__":
    # the recording: each run of RUNS on the driver as it is
    import tempfile
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    recording = {}
    for run, (run_spin, run_kw) in RUNS.items():
        with pytest.MonkeyPatch.context() as mp, tempfile.TemporaryDirectory() as tmp:
            calls, lines = _run(mp, tmp, Recorder(run_spin), run_kw)
        recording[run] = dict(calls=calls, printed=lines)
    with open(GOLDEN, "w") as f:
        json.dump(recording, f, sort_keys=True)
        f.write("\n")
