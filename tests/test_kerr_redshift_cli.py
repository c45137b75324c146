"""--redshift on the command line: it parses, --redshift exact takes --spin's refusals even at --spin 0 before any device is
touched, and the default hands the drivers no keyword."""
import numpy as np
import pytest

from bhr_amd import cli, drivers, kerr


def test_redshift_parses():
    assert cli.parse_args([]).redshift == "model"
    assert cli.parse_args(["--redshift", "model", "--disk_tilt", "20", "--gpus", "2"]).redshift == "model"
    args = cli.parse_args(["--redshift", "exact", "--spin", "-0.9"])
    assert args.redshift == "exact" and args.spin == -0.9
    cli.validate_args(args)
    assert cli.parse_args(["--redshift", "exact"]).spin == 0.0                 # a Schwarzschild hole under the exact redshift
    # supersampling, the lens flare, grading, video and an orbit all go with it
    cli.parse_args(["--redshift", "exact", "--spin", "0.5", "--supersample", "2", "--lens_flare", "--tonemap", "aces", "--video", "--orbit"])
    cli.parse_args(["--redshift", "exact", "--video", "--video_codec", "mjpeg", "--bit_depth", "8"])
    with pytest.raises(SystemExit):
        cli.parse_args(["--redshift", "doppler"])


@pytest.mark.parametrize("spin", [[], ["--spin", "0"], ["--spin", "0.7"]], ids=["no_spin", "spin0", "spin0.7"])
@pytest.mark.parametrize("extra, word", [
    (["--disk_tilt", "10"], "--disk_tilt"),
    (["--anti_alias", "lod_radius"], "--anti_alias"),
    (["--disk_model", "v2"], "--disk_model"),
    (["--disk_model", "v2_volume"], "--disk_model"),
    (["--supersample", "2", "--supersample_threshold", "0.1"], "--supersample_threshold"),
    (["--video", "--ray_map"], "--ray_map"),
    (["--video", "--orbit", "--orbit_map"], "--orbit_map"),
    (["--video", "--shutter", "0.5", "--shutter_map"], "--shutter_map"),
    (["--passes", "x.npz"], "--passes"),
    (["--video", "--shutter", "0.5"], "--shutter"),
    (["--gpus", "2"], "--gpus"),
])
def test_exact_takes_the_spin_refusals_as_argparse_errors(extra, word, spin, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--redshift", "exact"] + spin + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert word in err and ("--redshift exact" in err or "--spin" in err)
    if spin != ["--spin", "0.7"]:
        assert "--redshift exact" in err
        cli.parse_args(["--redshift", "model"] + spin + extra)                 # the same line under the model parses


def test_isco_note_under_exact():
    note = cli.spin_note(cli.parse_args(["--redshift", "exact"]))             # --ar1 2 inside the Schwarzschild ISCO at 3
    assert note and "ISCO" in note and "plunge" in note and "3.0000" in note
    assert cli.spin_note(cli.parse_args(["--redshift", "exact", "--ar1", "3.5"])) is None
    note = cli.spin_note(cli.parse_args(["--redshift", "exact", "--spin", "-0.9", "--ar1", "3"]))
    assert note and "plunge" in note and f"{kerr.disk_isco(-0.9):.4f}" in note
    assert "picture only" in cli.spin_note(cli.parse_args(["--spin", "-0.9", "--ar1", "3"]))     # the model's note is as it was


def test_isco_orbit_numbers():
    # Schwarzschild: r = 6 M = 3, E = sqrt(8 / 9), L = sqrt(12) M
    r, E, L = kerr.disk_isco_orbit(0.0)
    assert (r, E, L) == pytest.approx((3.0, np.sqrt(8.0 / 9.0), np.sqrt(12.0) * 0.5), abs=1e-12)
    for A in (0.6, -0.9, 0.998):
        r, E, L = kerr.disk_isco_orbit(A)
        assert r == kerr.disk_isco(A) and E * E == pytest.approx(1.0 - 1.0 / (3.0 * r), abs=1e-12)      # 1 - E^2 = 2 M / (3 r_isco)
    with pytest.raises(ValueError):
        kerr.check_redshift("doppler")


def _run_main(monkeypatch, argv):
    seen = {}

    def render_image(**kw):
        seen["image"] = kw
        return np.zeros((2, 2, 3), dtype=np.float32)

    def make_renderer(*a, **kw):
        seen["video"] = kw
        raise RuntimeError("stop here")

    monkeypatch.setattr(drivers, "render_image", render_image)
    monkeypatch.setattr(drivers, "make_renderer", make_renderer)
    monkeypatch.setattr(drivers, "save_image", lambda *a, **kw: None)
    try:
        cli.main(argv)
    except RuntimeError as e:
        assert str(e) == "stop here"
    return seen


def test_the_default_passes_no_keyword(monkeypatch):
    for argv in ([], ["--redshift", "model"], ["--spin", "0.5"], ["--spin", "0.5", "--redshift", "model"]):
        assert "redshift" not in _run_main(monkeypatch, argv)["image"], argv
        assert "redshift" not in _run_main(monkeypatch, argv + ["--video"])["video"], argv
    kw = _run_main(monkeypatch, ["--redshift", "exact"])["image"]
    assert kw["redshift"] == "exact" and "spin" not in kw
    kw = _run_main(monkeypatch, ["--redshift", "exact", "--spin", "-0.9", "--video", "--orbit"])["video"]
    assert kw["redshift"] == "exact" and kw["spin"] == -0.9
