"""--spin_observer / --spin_projection on the command line and in the drivers: the flags parse, a line without them parses to the
namespace it always did, every refusal is an argparse error that names the flags before any device is touched, the keywords reach
the drivers and the renderer, and a --video --orbit evaluates the velocity at every frame's own position.  No GPU."""
import numpy as np
import pytest

from bhr_amd import cli, drivers, observer
from bhr_amd.camera import orbit_position

SPIN = ["--spin", "0.9", "--pov", "3", "2", "0"]
NEW_KEYS = ("spin_observer", "spin_observer_velocity", "spin_observer_sky", "spin_projection", "spin_projection_fov")


def test_the_flags_parse():
    ns = cli.parse_args(SPIN + ["--spin_observer", "circular", "--spin_observer_sky", "plain", "--spin_projection", "fisheye", "--spin_projection_fov", "220"])
    assert (ns.spin_observer, ns.spin_observer_sky, ns.spin_projection, ns.spin_projection_fov) == ("circular", "plain", "fisheye", [220.0])
    view = cli.kerr_view_from_args(ns)["kerr_view"]
    assert view == dict(observer="circular", velocity=None, sky="plain", projection="fisheye", projection_fov=(220.0,))
    ns = cli.parse_args(["--redshift", "exact", "--spin_observer_velocity", "0.3", "-0.4", "0.5"])
    assert cli.kerr_view_from_args(ns)["kerr_view"]["velocity"] == (0.3, -0.4, 0.5)
    checked = drivers.check_kerr_view(cli.kerr_view_from_args(ns)["kerr_view"], spin=0.0, redshift="exact")
    assert checked["sky"] == "shift" and checked["projection"] is None
    ns = cli.parse_args(SPIN + ["--spin_projection", "equirect"])
    assert drivers.check_kerr_view(cli.kerr_view_from_args(ns)["kerr_view"], spin=0.9)["projection_fov"] == (360.0, 180.0)


def test_without_the_flags_the_namespace_is_what_it_was():
    """(No key at all: tests/test_projection_cli.py pins the default namespace key for key.)"""
    for line in ([], ["--spin", "0.6"], ["--video", "--orbit", "--supersample", "2"], ["--spin", "0.6", "--video", "--spin_map"]):
        ns = vars(cli.parse_args(line))
        assert not any(k in ns for k in NEW_KEYS)
        assert cli.kerr_view_from_args(cli.parse_args(line)) == {}
    plain = vars(cli.parse_args(SPIN + ["--video", "--orbit"]))
    with_view = vars(cli.parse_args(SPIN + ["--video", "--orbit", "--spin_observer", "circular"]))
    assert {k: v for k, v in with_view.items() if k not in NEW_KEYS} == plain and with_view["spin_observer"] == "circular"


REFUSALS = [
    (["--spin_observer", "zamo"], "needs --spin or --redshift exact"),
    (SPIN + ["--spin_observer", "infall"], "infall is not offered"),
    (SPIN + ["--spin_observer", "circular", "--spin_observer_velocity", "0.1", "0", "0"], "take one of the two"),
    (SPIN + ["--spin_observer_sky", "plain"], "needs --spin_observer or --spin_observer_velocity"),
    (SPIN + ["--spin_projection_fov", "180"], "needs --spin_projection"),
    (SPIN + ["--spin_observer_velocity", "0.9", "0.9", "0"], "at most 0.995"),
    (SPIN + ["--spin_observer_velocity", "nan", "0", "0"], "no NaN"),
    (SPIN + ["--spin_projection", "fisheye", "--spin_projection_fov", "400"], "outside"),
    (SPIN + ["--spin_projection", "equirect", "--spin_projection_fov", "360"], "takes projection_fov"),
    (SPIN + ["--spin_projection", "equirect", "--fov", "60"], "does not combine with --fov"),
    (["--spin", "0.9", "--pov", "3", "2", "0.3", "--spin_observer", "circular"], "off the equatorial plane"),
    (["--spin", "-0.9", "--pov", "2.01", "0", "0", "--spin_observer", "circular"], "at most 0.995"),
    (SPIN + ["--spin_observer", "zamo", "--video", "--spin_map"], "--spin_map or --spin_polarization"),
    (SPIN + ["--spin_observer", "zamo", "--spin_polarization", "toroidal"], "--spin_map or --spin_polarization"),
    (SPIN + ["--spin_observer", "zamo", "--observer", "static"], "--observer, --projection or --light_delay"),
    (SPIN + ["--spin_observer", "zamo", "--projection", "fisheye"], "--observer, --projection or --light_delay"),
    (SPIN + ["--spin_observer", "zamo", "--light_delay"], "--observer, --projection or --light_delay"),
    (SPIN + ["--spin_observer", "zamo", "--disk_tilt", "10"], "disk_tilt"),
    (SPIN + ["--spin_observer", "zamo", "--anti_alias", "lod_radius"], "anti_alias"),
    (SPIN + ["--spin_observer", "zamo", "--disk_model", "v2"], "disk_model"),
    (SPIN + ["--spin_observer", "zamo", "--supersample", "2", "--supersample_threshold", "0.1"], "supersample_threshold"),
    (SPIN + ["--spin_observer", "zamo", "--gpus", "2"], "one GPU"),
    (SPIN + ["--spin_observer", "zamo", "--passes", "p.npz"], "passes"),
    (SPIN + ["--spin_observer", "zamo", "--video", "--shutter", "0.5"], "shutter"),
    (SPIN + ["--spin_observer", "zamo", "--video", "--ray_map"], "ray_map"),
    (SPIN + ["--spin_observer", "zamo", "--stars", "point"], "point stars"),
]


@pytest.mark.parametrize("line,word", REFUSALS, ids=lambda v: " ".join(v[3:]) if isinstance(v, list) else None)
def test_refusals_are_argparse_errors(line, word, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(line)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert word in err, err
    structural = ("take one of the two", "needs --spin_", "infall", "at most", "NaN", "outside", "takes projection_fov", "equatorial", "--fov")
    assert "--spin_observer" in err or "--spin_projection" in err or any(w in err for w in structural)


def test_driver_checks_need_no_device():
    assert drivers.check_kerr_view(None) is None
    with pytest.raises(ValueError, match="takes observer"):
        drivers.check_kerr_view(dict(kind="zamo"), spin=0.5)
    with pytest.raises(ValueError, match="needs an observer"):
        drivers.check_kerr_view({}, spin=0.5)
    view = drivers.check_kerr_view(dict(observer="zamo"), spin=0.998)
    assert drivers.kerr_view_beta(view, (3.0, 2.0, 0.3), 0.998) == tuple(float(v) for v in observer.kerr_velocity("zamo", (3.0, 2.0, 0.3), 0.998))
    assert drivers.kerr_view_beta(drivers.check_kerr_view(dict(projection="fisheye"), spin=0.5), (6, 0, 0), 0.5) is None
    with pytest.raises(ValueError, match="needs --spin"):
        drivers.render_image(64, 32, [6, 0, 0.5], 90, 0.1, kerr_view=dict(observer="static"))
    with pytest.raises(ValueError, match="static limit"):
        drivers.render_image(64, 32, [1.01, 0, 0], 90, 0.1, spin=0.998, kerr_view=dict(observer="zamo"))


def test_progress_params_carry_the_camera_only_when_set():
    base = drivers.progress_params(4, 90, True, 0.1, 360.0)
    assert "kerr_view" not in base
    view = drivers.check_kerr_view(dict(observer="circular", projection="fisheye"), spin=0.9)
    with_view = drivers.progress_params(4, 90, True, 0.1, 360.0, kerr_view=view)
    assert with_view == {**base, "kerr_view": dict(observer="circular", velocity=None, sky="shift", projection="fisheye", projection_fov=[180.0])}


def test_video_orbit_evaluates_the_velocity_at_every_frames_position():
    n, pov, A = 6, [3.0, 2.0, 0.0], 0.9
    plan = observer.kerr_frame_plan(n, pov, A, "circular", None, True, 360.0)
    assert len(plan) == n
    for f, (pos, beta) in enumerate(plan):
        want_pos = [float(v) for v in orbit_position(pov, f, n, 360.0)]
        assert pos == want_pos
        assert beta == tuple(float(v) for v in observer.kerr_velocity("circular", want_pos, A))
    speeds = [np.linalg.norm(b) for _, b in plan]
    assert np.ptp(speeds) < 1e-12 and speeds[0] > 0.3                        # one orbit, one speed ...
    assert np.linalg.norm(np.subtract(plan[0][1], plan[3][1])) > 0.5         # ... whose direction turns with the camera
    fixed = observer.kerr_frame_plan(n, pov, A, None, (0.1, 0.2, 0.0), True, 360.0)
    assert all(b == (0.1, 0.2, 0.0) for _, b in fixed)
    still = observer.kerr_frame_plan(3, pov, A, "zamo")
    assert all(p == pov and b == still[0][1] for p, b in still)


def test_the_camera_reaches_the_drivers(monkeypatch):
    seen = {}
    monkeypatch.setattr(drivers, "render_image", lambda **kw: seen.update(kw) or np.zeros((4, 4, 3), np.float32))
    monkeypatch.setattr(drivers, "save_image", lambda *a, **k: None)
    assert cli.main(SPIN + ["--spin_observer", "circular", "--spin_projection", "fisheye", "--resolution", "fhd"]) == 0
    assert seen["kerr_view"] == dict(observer="circular", velocity=None, sky=None, projection="fisheye", projection_fov=None)
    assert (seen["width"], seen["height"]) == (1080, 1080) and seen["spin"] == 0.9          # --projection's frame-size rule
    seen.clear()
    assert cli.main(SPIN + ["--resolution", "fhd"]) == 0
    assert "kerr_view" not in seen and (seen["width"], seen["height"]) == (1920, 1080)


def test_the_renderer_keywords_are_refused_with_the_schwarzschild_ones():
    from bhr_amd.renderer import HipRenderer
    r = HipRenderer.__new__(HipRenderer)
    for kw in (dict(observer=(0, 0, 0)), dict(projection="fisheye"), dict(light_delay=1.0), dict(math="strict")):
        with pytest.raises(ValueError, match="kerr_observer / kerr_projection do not combine"):
            HipRenderer.render_async(r, [6, 0, 0.5], 90, kerr_observer=(0.1, 0, 0), **kw)
    with pytest.raises(ValueError, match="kerr_projection_fov without kerr_projection"):
        HipRenderer.render_async(r, [6, 0, 0.5], 90, kerr_projection_fov=(180,))
