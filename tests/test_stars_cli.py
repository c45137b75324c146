"""--stars point on the command line: it parses, the defaults change nothing, every refusal is an argparse error that names the
combination, and the drivers refuse the same combinations before any device is touched.  No GPU."""
import pytest

from bhr_amd import cli, drivers

NEW = {"stars": "texture", "star_gain": 2.0, "star_max_magnification": 32.0}


def test_stars_parse():
    a = cli.parse_args(["--stars", "point"])
    assert (a.stars, a.star_gain, a.star_max_magnification) == ("point", 2.0, 32.0)
    cli.validate_args(a)
    assert cli.stars_from_args(a) == {"gain": 2.0, "max_magnification": 32.0}
    assert cli.stars_from_args(cli.parse_args([])) is None
    a = cli.parse_args(["--stars", "point", "--star_gain", "3.5", "--star_max_magnification", "100", "--n_stars", "900"])
    assert cli.stars_from_args(a) == {"gain": 3.5, "max_magnification": 100.0} and a.n_stars == 900
    # a tilted disk, anti-aliasing, the lens flare, grading, an HDR still, passes and both map videos go with point stars
    cli.parse_args(["--stars", "point", "--disk_tilt", "20", "--anti_alias", "lod_radius", "--lens_flare", "--tonemap", "aces",
                    "--hdr_output", "x.pfm", "--passes", "x.npz", "--math", "fast"])
    cli.parse_args(["--stars", "point", "--video", "--ray_map"])
    cli.parse_args(["--stars", "point", "--video", "--orbit", "--orbit_map", "--video_hdr", "pq"])


def test_help_says_strict(capsys):
    with pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "--stars {texture,point}" in out and "strict arithmetic, whatever --math says" in out
    assert "--star_gain G" in out and "--star_max_magnification M" in out


def test_defaults_change_nothing():
    """Without the new flags a command line parses to what it parsed to before, plus the new keys at their defaults; --stars
    texture is the default spelled out."""
    for line in ([], ["--video", "--orbit", "--supersample", "2"], ["--disk_tilt", "20", "--anti_alias", "lod_radius", "--gpus", "2"],
                 ["--spin", "0.5"], ["--video", "--shutter", "0.5", "--shutter_map"], ["--observer", "circular"], ["--texture", "sky.png"],
                 ["--video", "--ray_map", "--map_supersample", "2"], ["--disk_model", "v2"]):
        ns = vars(cli.parse_args(line))
        assert {k: ns[k] for k in NEW} == NEW
        assert vars(cli.parse_args(line + ["--stars", "texture"])) == ns
    # the other two flags alone change those keys alone (they are read under --stars point only)
    ns, other = vars(cli.parse_args([])), vars(cli.parse_args(["--star_gain", "5", "--star_max_magnification", "8"]))
    assert {k: v for k, v in other.items() if k not in NEW} == {k: v for k, v in ns.items() if k not in NEW}


REFUSALS = [
    (["--texture", "sky.png"], ["--texture", "a sky image has no catalogue"]),
    (["--video"], ["--video", "--ray_map or --orbit_map"]),
    (["--video", "--orbit"], ["--video", "--ray_map or --orbit_map"]),
    (["--video", "--shutter", "0.5", "--shutter_map"], ["--shutter_map"]),
    (["--video", "--ray_map", "--map_supersample", "2"], ["--map_supersample"]),
    (["--video", "--orbit", "--orbit_map", "--map_supersample", "4"], ["--map_supersample"]),
    (["--supersample", "2"], ["--supersample"]),
    (["--gpus", "2"], ["--gpus"]),
    (["--disk_model", "v2"], ["--disk_model"]),
    (["--disk_model", "v2_volume"], ["--disk_model"]),
    (["--spin", "0.5"], ["--spin"]),
    (["--redshift", "exact"], ["--redshift exact"]),
    (["--observer", "circular"], ["--observer"]),
    (["--observer_velocity", "0.1", "0.2", "0.3"], ["--observer_velocity"]),
    (["--observer", "static", "--observer_sky", "plain"], ["--observer_sky"]),
    (["--observer", "infall", "--video", "--infall_to", "2"], ["--infall_to"]),
    (["--star_gain", "0"], ["--star_gain", "greater than 0"]),
    (["--star_gain", "-1"], ["--star_gain", "greater than 0"]),
    (["--star_gain", "nan"], ["--star_gain"]),
    (["--star_max_magnification", "0.5"], ["--star_max_magnification"]),
]


@pytest.mark.parametrize("extra, words", REFUSALS, ids=lambda v: "_".join(v) if isinstance(v, list) and v and v[0].startswith("--") else None)
def test_refusals_are_argparse_errors(extra, words, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--stars", "point"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    for w in words:
        assert w in err, (w, err)
    cli.parse_args(["--stars", "point"])                          # the flag alone parses


@pytest.mark.parametrize("line", [["--spin", "0.5", "--disk_tilt", "5"], ["--observer", "circular", "--gpus", "2"],
                                  ["--video", "--ray_map", "--orbit"], ["--map_supersample", "2"], ["--video", "--orbit_map"]])
def test_existing_refusals_keep_their_words(line, capsys):
    """A line that was refused before is refused with the same message with --stars point in front of it."""
    with pytest.raises(SystemExit):
        cli.parse_args(line)
    before = capsys.readouterr().err.splitlines()[-1]
    with pytest.raises(SystemExit):
        cli.parse_args(["--stars", "point"] + line)
    assert capsys.readouterr().err.splitlines()[-1] == before


def test_drivers_refuse_before_any_device_work():
    assert drivers.check_stars(None) is None
    assert drivers.check_stars({}) == {"gain": 2.0, "max_magnification": 32.0}
    assert drivers.check_stars({"gain": 3.0}) == {"gain": 3.0, "max_magnification": 32.0}
    for kw, word in ((dict(skybox_path="sky.png"), "sky texture"), (dict(supersample=2), "supersample"), (dict(gpus=2), "one GPU"),
                     (dict(disk_model="v2"), "disk_model"), (dict(spin=0.3), "spin"), (dict(redshift="exact"), "exact redshift"),
                     (dict(observer=(0.1, 0.0, 0.0)), "moving observer")):
        with pytest.raises(ValueError, match=word):
            drivers.check_stars({}, **kw)
    for bad in ({"gain": 0.0}, {"gain": float("nan")}, {"max_magnification": 0.5}, {"max_magnification": 2e6}, {"colour": 1}):
        with pytest.raises(ValueError):
            drivers.check_stars(bad)
    with pytest.raises(ValueError, match="one GPU"):
        drivers.render_image(64, 36, [6, 0, 0.5], 90.0, 0.1, gpus=2, stars={})
    # the progress record of a video names the stars, and only when there are any
    base = drivers.progress_params(4, 90.0, True, 0.1, 360.0, orbit_map=True)
    with_stars = drivers.progress_params(4, 90.0, True, 0.1, 360.0, orbit_map=True, stars={"gain": 2.0, "max_magnification": 32.0})
    assert "stars" not in base and with_stars == dict(base, stars={"gain": 2.0, "max_magnification": 32.0})
