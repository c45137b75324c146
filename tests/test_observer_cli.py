"""--observer on the command line: it parses, its refusals fire before any device is touched, the defaults change nothing, and
the per-frame plan of a video (positions and velocities) is what the drivers render."""
import numpy as np
import pytest

from bhr_amd import cli, drivers, observer


def test_observer_parses():
    a = cli.parse_args(["--observer", "circular"])
    assert (a.observer, a.observer_velocity, a.observer_sky, a.infall_to) == ("circular", None, "shift", None)
    cli.validate_args(a)
    assert cli.observer_beta(a) == pytest.approx(tuple(observer.velocity("circular", [6, 0, 0.5])))
    a = cli.parse_args(["--observer_velocity", "0.3", "-0.4", "0.5", "--observer_sky", "plain"])
    assert a.observer is None and a.observer_velocity == [0.3, -0.4, 0.5] and a.observer_sky == "plain"
    assert cli.observer_beta(a) == (0.3, -0.4, 0.5)
    assert cli.observer_beta(cli.parse_args(["--observer", "static"])) == (0.0, 0.0, 0.0)
    assert cli.observer_beta(cli.parse_args([])) is None
    # plain supersampling, a tilted disk, the lens flare, grading, HDR, video and an orbit all go with a moving camera
    cli.parse_args(["--observer", "circular", "--supersample", "2", "--disk_tilt", "20", "--lens_flare", "--tonemap", "aces", "--video",
                    "--orbit", "--video_hdr", "pq", "--math", "fast"])
    a = cli.parse_args(["--observer", "infall", "--video", "--infall_to", "2"])
    assert a.infall_to == 2.0


def test_defaults_change_nothing():
    new = {"observer": None, "observer_velocity": None, "observer_sky": "shift", "infall_to": None}
    for line in ([], ["--video", "--orbit", "--supersample", "2"], ["--disk_tilt", "20", "--anti_alias", "lod_radius", "--gpus", "2"],
                 ["--spin", "0.5"], ["--video", "--shutter", "0.5", "--shutter_map"]):
        ns = vars(cli.parse_args(line))
        assert {k: ns[k] for k in new} == new
        static = vars(cli.parse_args(line + ["--observer", "static"])) if line in ([], ["--video", "--orbit", "--supersample", "2"]) else None
        if static is not None:                                    # the same line with a camera at rest differs in that key alone
            assert {k: v for k, v in static.items() if k != "observer"} == {k: v for k, v in ns.items() if k != "observer"}


FLAGS = (["--observer", "circular"], ["--observer_velocity", "0.1", "0.2", "0.3"], ["--observer", "static", "--observer_sky", "plain"])


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: f[0] + "_" + f[1])
@pytest.mark.parametrize("extra, word", [
    (["--spin", "0.7"], "--spin"),
    (["--redshift", "exact"], "--redshift exact"),
    (["--anti_alias", "lod_radius"], "--anti_alias"),
    (["--disk_model", "v2"], "--disk_model"),
    (["--disk_model", "v2_volume"], "--disk_model"),
    (["--supersample", "2", "--supersample_threshold", "0.1"], "--supersample_threshold"),
    (["--gpus", "2"], "--gpus"),
    (["--video", "--shutter", "0.5"], "--shutter"),
    (["--video", "--ray_map"], "--ray_map"),
    (["--video", "--orbit", "--orbit_map"], "--orbit_map"),
    (["--video", "--shutter", "0.5", "--shutter_map"], "--shutter"),
    (["--passes", "x.npz"], "--passes"),
])
def test_observer_refusals_are_argparse_errors(flags, extra, word, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(flags + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert flags[0] in err and word in err
    cli.parse_args(extra)                                         # the same line with a camera that stands still parses
    cli.parse_args(flags)


@pytest.mark.parametrize("line, word", [
    (["--observer", "infall", "--observer_velocity", "0.1", "0", "0"], "one of the two"),
    (["--observer_sky", "plain"], "needs --observer"),
    (["--infall_to", "2", "--video"], "needs --observer"),
    (["--observer", "circular", "--infall_to", "2", "--video"], "--observer infall"),
    (["--observer", "infall", "--infall_to", "2"], "--video"),
    (["--observer", "infall", "--infall_to", "2", "--video", "--orbit"], "--orbit"),
    (["--observer", "infall", "--infall_to", "1.04", "--video"], "1.05"),
    (["--observer", "infall", "--infall_to", "7", "--video"], "inwards"),
    (["--observer", "circular", "--pov", "1.4", "0", "0.1"], "1.5"),
    (["--observer", "circular", "--pov", "1.5", "0", "0"], "1.5"),
    (["--observer", "circular", "--pov", "0", "0", "4"], "z axis"),
    (["--observer", "circular", "--video", "--orbit", "--pov", "1.2", "0", "0.2"], "1.5"),
    (["--observer_velocity", "0.8", "0.6", "0.1"], "0.995"),
    (["--observer_velocity", "nan", "0", "0"], "0.995"),
    (["--observer", "infall", "--pov", "1.005", "0", "0"], "0.995"),
])
def test_observer_argument_errors(line, word, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(line)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_orbit_plan_velocities():
    """--video --orbit --observer circular: every frame's velocity is the circular one at that frame's own camera position."""
    a = cli.parse_args(["--observer", "circular", "--video", "--orbit", "--n_frames", "4"])
    plan = observer.frame_plan(a.n_frames, a.pov, a.observer, a.observer_velocity, a.orbit, a.orbit_degrees, a.infall_to)
    assert len(plan) == 4
    r = float(np.linalg.norm([np.linalg.norm(a.pov), a.pov[2]]))   # the orbit's radius is |pov| in the plane, at the pov's height
    speed = np.sqrt(0.5 / (r - 1.0))
    for f, (pos, beta) in enumerate(plan):
        ang = np.radians(90.0 * f)
        assert pos == pytest.approx([np.linalg.norm(a.pov) * np.cos(ang), np.linalg.norm(a.pov) * np.sin(ang), 0.5], abs=1e-12)
        assert beta == pytest.approx((speed * np.sin(ang), -speed * np.cos(ang), 0.0), abs=1e-12)      # r_hat x z_hat, turned with the camera
        assert all(type(v) is float for v in beta)
    # a fixed velocity stays what it is; a camera that stands still keeps its position
    plan = observer.frame_plan(3, [6, 0, 0.5], None, (0.1, 0.2, 0.3), True, 360.0, None)
    assert [b for _, b in plan] == [(0.1, 0.2, 0.3)] * 3
    assert observer.frame_plan(2, [6, 0, 0.5], "infall") == [([6.0, 0.0, 0.5], tuple(float(v) for v in observer.velocity("infall", [6, 0, 0.5])))] * 2


def test_infall_plan_positions():
    a = cli.parse_args(["--observer", "infall", "--video", "--infall_to", "2", "--n_frames", "5", "--pov", "3", "4", "0"])
    plan = observer.frame_plan(a.n_frames, a.pov, a.observer, None, False, 360.0, a.infall_to)
    radii = observer.infall_radii(5.0, 2.0, 5)
    for (pos, beta), r in zip(plan, radii):
        assert pos == pytest.approx([0.6 * r, 0.8 * r, 0.0], abs=1e-12)                # along pov
        assert beta == pytest.approx((-0.6 * np.sqrt(1 / r), -0.8 * np.sqrt(1 / r), 0.0), abs=1e-12)
    assert plan[0][0] == pytest.approx([3.0, 4.0, 0.0]) and np.linalg.norm(plan[-1][0]) == pytest.approx(2.0)
    with pytest.raises(ValueError):
        observer.frame_plan(5, [3, 4, 0], "infall", orbit=True, infall_to=2.0)


def test_driver_checks_need_no_device():
    drivers.check_observer(None, anti_alias="lod_radius", gpus=4, spin=0.9)          # a camera that stands still: nothing to check
    drivers.check_observer((0.1, 0.0, 0.0))
    for kw in (dict(anti_alias="lod_radius"), dict(disk_model="v2"), dict(supersample_threshold=0.1), dict(gpus=2), dict(spin=0.5),
               dict(redshift="exact"), dict(passes=True), dict(shutter=0.5), dict(maps=True)):
        with pytest.raises(ValueError):
            drivers.check_observer((0.1, 0.0, 0.0), **kw)
    with pytest.raises(ValueError):
        drivers.check_observer((1.0, 0.0, 0.0))
    assert "observer" not in drivers.progress_params(4, 90.0, True, 0.1, 360.0)
    assert drivers.progress_params(4, 90.0, True, 0.1, 360.0, observer={"kind": "circular"})["observer"] == {"kind": "circular"}
