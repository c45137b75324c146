"""--spin on the command line: it parses, its refusals fire before any device is touched, and --spin 0 changes nothing."""
import pytest

from bhr_amd import cli, kerr


def test_spin_parses():
    args = cli.parse_args(["--spin", "0.9"])
    assert args.spin == 0.9
    assert cli.parse_args(["--spin", "-0.998", "--supersample", "4"]).spin == -0.998
    assert cli.parse_args([]).spin == 0.0
    cli.validate_args(args)
    # plain supersampling, the lens flare, grading, video and an orbit all go with a spin
    cli.parse_args(["--spin", "0.5", "--supersample", "2", "--lens_flare", "--tonemap", "aces", "--video", "--orbit"])


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
def test_spin_refusals_are_argparse_errors(extra, word, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--spin", "0.7"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--spin" in err and word in err
    cli.parse_args(extra)                              # the same line without a spin parses


@pytest.mark.parametrize("value", ["0.999", "-1", "2", "nan"])
def test_spin_range(value, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--spin=" + value])
    assert e.value.code == 2
    assert "0.998" in capsys.readouterr().err


def test_spin_zero_leaves_the_namespace_as_it_was():
    for line in ([], ["--video", "--orbit", "--supersample", "2"], ["--disk_tilt", "20", "--anti_alias", "lod_radius", "--gpus", "2"]):
        plain, zero = vars(cli.parse_args(line)), vars(cli.parse_args(line + ["--spin", "0"]))
        assert plain == zero
        assert plain.pop("spin") == 0.0
    assert cli.spin_note(cli.parse_args([])) is None


def test_isco_note():
    # the disk's own sense: prograde for a positive spin, retrograde for a negative one
    assert cli.spin_note(cli.parse_args(["--spin", "0.9", "--ar1", "1.5"])) is None
    note = cli.spin_note(cli.parse_args(["--spin", "0.9", "--ar1", "1.1"]))
    assert note and "prograde" in note and "ISCO" in note
    note = cli.spin_note(cli.parse_args(["--spin", "-0.9", "--ar1", "3"]))
    assert note and "retrograde" in note
    assert kerr.r_isco(0.0, True) == pytest.approx(3.0) and kerr.r_isco(0.0, False) == pytest.approx(3.0)
    assert kerr.r_plus(0.0) == 1.0 and kerr.r_photon(0.0, True) == pytest.approx(1.5)
    info = kerr.kerr_info(0.9)
    assert info["r_isco_prograde"] < 3.0 < info["r_isco_retrograde"] and info["r_photon_pro"] < 1.5 < info["r_photon_retro"]
    assert info["a"] == pytest.approx(0.45)


@pytest.mark.parametrize("line", [["--spin", "0.998", "--pov", "1.08", "0", "0.05"], ["--spin", "0.998", "--pov", "0.7", "0", "0.02"],
                                  ["--redshift", "exact", "--pov", "0.9", "0", "0.1"], ["--spin", "0.5", "--video", "--orbit", "--pov", "0.95", "0", "0"]])
def test_a_camera_inside_the_static_limit_is_an_argparse_error(line, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(line)
    assert e.value.code == 2 and "static limit" in capsys.readouterr().err
    cli.parse_args([a for a in line if a not in ("--spin", "0.998", "0.5", "--redshift", "exact")])   # without the Kerr march it parses
    assert cli.parse_args(["--spin", "0.998", "--pov", "1.3", "0.2", "0.1"]).pov == [1.3, 0.2, 0.1]

