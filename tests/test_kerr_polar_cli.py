"""--spin_polarization on the command line and in the drivers' checks (no device): parsing, the companion flags it shares with
--polarization, every new refusal naming its flag, and that the default namespace and the lines --polarization and --spin_map
refuse keep their words."""
import numpy as np
import pytest

from bhr_amd import cli, drivers, polarization

SPIN = ["--spin", "0.6"]


def _error(capsys, argv):
    with pytest.raises(SystemExit):
        cli.parse_args(argv)
    return capsys.readouterr().err


def test_parsing_and_the_shared_companions():
    a = cli.parse_args(SPIN + ["--spin_polarization", "toroidal"])
    assert a.spin_polarization == ["toroidal"] and not hasattr(a, "polarization")
    assert cli.polarization_from_args(a) == {"kerr_polarization": dict(field=(0.0, 1.0, 0.0), fraction=0.7, cell=16)}
    a = cli.parse_args(SPIN + ["--redshift", "exact", "--spin_polarization", "0.3", "0.8", "0.5", "--polarization_fraction", "1", "--polarization_cell", "8",
                               "--stokes_output", "s.npz", "--polarization_ticks", "t.png", "--lens_flare", "--tonemap", "aces"])
    assert cli.polarization_from_args(a) == {"kerr_polarization": dict(field=(0.3, 0.8, 0.5), fraction=1.0, cell=8), "stokes_path": "s.npz",
                                             "ticks_path": "t.png"}
    # the exact redshift alone is the Kerr march too; a video takes --spin_map and the companions with it
    assert cli.parse_args(["--redshift", "exact", "--spin_polarization", "radial"]).spin_polarization == ["radial"]
    a = cli.parse_args(SPIN + ["--video", "--spin_map", "--spin_polarization", "vertical", "--stokes_output", "v.npz", "--polarization_cell", "32"])
    assert cli.polarization_from_args(a) == {"kerr_polarization": dict(field=(0.0, 0.0, 1.0), fraction=0.7, cell=32), "stokes_path": "v.npz"}
    # --polarization's own lines are what they were
    a = cli.parse_args(["--polarization", "toroidal", "--polarization_cell", "8"])
    assert cli.polarization_from_args(a) == {"polarization": dict(field=(0.0, 1.0, 0.0), fraction=0.7, cell=8)}


def test_the_default_namespace_is_what_it_was():
    a = vars(cli.parse_args([]))
    for key in ("spin_polarization", "polarization", "polarization_fraction", "polarization_cell", "stokes_output", "polarization_ticks", "spin_map"):
        assert key not in a
    assert cli.polarization_from_args(cli.parse_args([])) == {}


REFUSALS = [
    (["--spin_polarization", "toroidal"], "--spin_polarization needs --spin or --redshift exact"),
    (SPIN + ["--spin_polarization", "spiral"], "--spin_polarization: polarization field 'spiral'"),
    (SPIN + ["--spin_polarization", "1", "2"], "--spin_polarization: polarization field takes three numbers"),
    (SPIN + ["--spin_polarization", "toroidal", "--polarization_fraction", "1.5"], "--spin_polarization: polarization_fraction"),
    (SPIN + ["--spin_polarization", "toroidal", "--polarization_cell", "12"], "--spin_polarization: polarization_cell"),
    (SPIN + ["--spin_polarization", "toroidal", "--video"], "--spin_polarization with --video needs --spin_map"),
    (SPIN + ["--spin_polarization", "toroidal", "--video", "--spin_map", "--orbit"], "--spin_polarization does not combine with --orbit"),
    (SPIN + ["--spin_polarization", "toroidal", "--supersample", "2"], "--spin_polarization does not combine with --supersample other than 1"),
    (SPIN + ["--spin_polarization", "toroidal", "--video", "--spin_map", "--polarization_ticks", "t.png"], "--polarization_ticks is a still image's overlay"),
    (SPIN + ["--spin_polarization", "toroidal", "--stokes_output", "s.txt"], "--stokes_output writes a .npz file"),
    (SPIN + ["--spin_polarization", "toroidal", "--polarization_ticks", "t.jpg"], "--polarization_ticks writes a .png file"),
]


@pytest.mark.parametrize("argv, words", REFUSALS, ids=[" ".join(r[0][:6]) for r in REFUSALS])
def test_new_refusals_name_the_flag(capsys, argv, words):
    assert words in _error(capsys, argv)


# lines that were refused before keep their words, --spin_polarization or not
OLD_LINES = [
    (["--polarization_fraction", "0.5"], "--polarization_fraction needs --polarization: it belongs to the Stokes maps"),
    (["--stokes_output", "s.npz"], "--stokes_output needs --polarization: it belongs to the Stokes maps"),
    (SPIN + ["--polarization", "toroidal"], "--polarization does not combine with --spin: the transport rule is Schwarzschild's and a ray map holds Schwarzschild rays"),
    (["--redshift", "exact", "--polarization", "toroidal"], "--polarization does not combine with --redshift exact: that is the Kerr march's"),
    (["--polarization", "toroidal", "--video"], "--polarization with --video needs --ray_map"),
    (SPIN + ["--video", "--spin_map", "--polarization", "toroidal"], "--spin_map does not combine with --polarization: it is a Schwarzschild march's or the Schwarzschild ray map's"),
    (SPIN + ["--video", "--spin_map", "--polarization_cell", "8"], "--spin_map does not combine with --polarization: it is a Schwarzschild march's or the Schwarzschild ray map's"),
    (SPIN + ["--video", "--spin_map", "--shutter", "0.5"], "--spin_map does not combine with --shutter: shutter frames are marched"),
    (SPIN + ["--video", "--spin_map", "--supersample", "2"], "--spin_map does not combine with --supersample other than 1: a Kerr ray map holds one ray per pixel"),
    (SPIN + ["--video", "--spin_map", "--ray_map"], "--spin_map does not combine with --ray_map: that is a map of Schwarzschild rays"),
    (["--spin_map", "--video"], "--spin_map needs --spin or --redshift exact"),
]


@pytest.mark.parametrize("argv, words", OLD_LINES, ids=[" ".join(r[0][:5]) for r in OLD_LINES])
def test_existing_refusals_keep_their_words(capsys, argv, words):
    assert words in _error(capsys, argv)
    # ... and with --spin_polarization on the line what --spin_map refuses is still refused, in --spin_map's words
    if "--spin_map" in argv and "--polarization" not in argv and "--polarization_cell" not in argv and "--spin" in argv:
        assert words in _error(capsys, argv + ["--spin_polarization", "toroidal"])


def test_spin_polarization_and_polarization_together(capsys):
    err = _error(capsys, ["--polarization", "toroidal", "--spin_polarization", "toroidal"])
    assert "--spin_polarization needs --spin" in err or "--spin_polarization does not combine with --polarization" in err


def test_the_drivers_check():
    ok = drivers.check_kerr_polarization(dict(field="toroidal"), spin=0.6)
    assert ok == dict(field=(0.0, 1.0, 0.0), fraction=0.7, cell=16)
    assert drivers.check_kerr_polarization(None) is None
    assert drivers.check_kerr_polarization(dict(field=(1, 2, 3), fraction=1.0, cell=8), redshift="exact", video=True, spin_map=True)["cell"] == 8
    for kw, words in ((dict(), "needs --spin or --redshift exact"), (dict(spin=0.6, polarization=True), "does not combine with --polarization"),
                      (dict(spin=0.6, video=True), "with --video needs --spin_map"), (dict(spin=0.6, video=True, spin_map=True, orbit=True), "--orbit"),
                      (dict(spin=0.6, supersample=2), "--supersample other than 1"), (dict(spin=0.6, map_supersample=2), "--map_supersample"),
                      (dict(spin=0.6, gpus=2), "--gpus"), (dict(spin=0.6, world=2), "--gpus"), (dict(spin=0.6, shutter=0.5), "--shutter"),
                      (dict(spin=0.6, ray_map=True), "--ray_map"), (dict(spin=0.6, orbit_map=True), "--orbit_map"), (dict(spin=0.6, shutter_map=True), "--shutter_map"),
                      (dict(spin=0.6, passes=True), "--passes"), (dict(spin=0.6, observer=True), "--observer"), (dict(spin=0.6, projection=True), "--projection"),
                      (dict(spin=0.6, light_delay=True), "--light_delay"), (dict(spin=0.6, stars=True), "--stars point"),
                      (dict(spin=0.6, disk_model="v2"), "--disk_model"), (dict(spin=0.6, stokes_path="s.txt"), ".npz"),
                      (dict(spin=0.6, ticks_path="t.jpg"), ".png"), (dict(spin=0.6, video=True, spin_map=True, ticks_path="t.png"), "still image's overlay")):
        with pytest.raises(ValueError, match="spin_polarization|stokes_output|polarization_ticks") as e:
            drivers.check_kerr_polarization(dict(field="toroidal"), **kw)
        assert words in str(e.value), (kw, str(e.value))
    with pytest.raises(ValueError, match="takes field, fraction and cell"):
        drivers.check_kerr_polarization(dict(fraction=0.5), spin=0.6)
    with pytest.raises(ValueError):
        drivers.check_kerr_polarization(dict(field="toroidal", cell=12), spin=0.6)


def test_the_npz_names_the_hole(tmp_path):
    cells = np.zeros((2, 3, 3), dtype=np.float32)
    path = str(tmp_path / "s.npz")
    polarization.write_stokes(path, cells, 16, "toroidal", 0.7, camera=dict(cam_pos=[6, 0, 0.5], fov=90.0), hole=dict(spin=0.6, redshift="exact"))
    d = np.load(path)
    assert float(d["spin"]) == 0.6 and str(d["redshift"]) == "exact" and str(d["convention"]) == polarization.CONVENTION
    polarization.write_stokes(path, cells, 16, "toroidal", 0.7)
    assert "spin" not in np.load(path).files                      # --polarization's file is what it was
