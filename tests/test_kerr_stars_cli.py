"""--spin_stars and --spin_passes on the command line and in the drivers: the flags parse, they are absent from the default
namespace, a line refused without them is refused with the same last line with them, every new refusal is an argparse error that
names both flags and is raised before a renderer is made, and check_kerr_stars / check_kerr_passes raise the same.  No GPU."""
import pytest

from bhr_amd import cli, drivers

NEW = ("spin_stars", "spin_passes")
SPIN = ["--spin", "0.9"]


@pytest.fixture(autouse=True)
def no_renderer(monkeypatch):
    """Every refusal comes before the device: make_renderer and render_image must not be reached."""
    def touched(*a, **k):
        raise AssertionError("a renderer was asked for")
    monkeypatch.setattr(drivers, "make_renderer", touched)
    monkeypatch.setattr(drivers, "render_image", touched)
    monkeypatch.setattr(drivers, "render_video", touched)


def _error(line, capsys, run=False):
    with pytest.raises(SystemExit) as e:
        cli.main(line) if run else cli.parse_args(line)
    assert e.value.code == 2
    return capsys.readouterr().err.strip().splitlines()[-1]


def test_the_flags_parse():
    a = cli.parse_args(SPIN + ["--spin_stars", "point"])
    assert a.spin_stars == "point" and not hasattr(a, "spin_passes") and a.stars == "texture"
    assert cli.kerr_stars_from_args(a) == {"gain": 2.0, "max_magnification": 32.0}
    a = cli.parse_args(["--redshift", "exact", "--spin_stars", "point", "--star_gain", "30", "--star_max_magnification", "8"])
    assert cli.kerr_stars_from_args(a) == {"gain": 30.0, "max_magnification": 8.0}
    assert cli.kerr_stars_from_args(cli.parse_args(SPIN)) is None
    a = cli.parse_args(SPIN + ["--spin_passes", "p.npz"])
    assert a.spin_passes == "p.npz" and not hasattr(a, "spin_stars")
    # what works beside them: the exact redshift, the lens flare, the grade, any --math, a map video with or without an orbit, both
    for line in (SPIN + ["--spin_stars", "point", "--spin_passes", "p.npz", "--redshift", "exact", "--lens_flare", "--tonemap", "aces", "--math", "fast"],
                 SPIN + ["--spin_stars", "point", "--video", "--spin_map"], SPIN + ["--spin_stars", "point", "--video", "--spin_map", "--orbit"],
                 SPIN + ["--spin_stars", "point", "--video", "--spin_map", "--spin_map_supersample", "1"],
                 SPIN + ["--spin_passes", "P.NPZ", "--spin_polarization", "toroidal"]):
        cli.validate_args(cli.parse_args(line))
    with pytest.raises(SystemExit):
        cli.parse_args(SPIN + ["--spin_stars", "texture"])


def test_the_default_namespace_has_no_new_key():
    for line in ([], ["--video", "--orbit", "--supersample", "2"], SPIN, ["--stars", "point"], SPIN + ["--video", "--spin_map"],
                 SPIN + ["--spin_polarization", "toroidal"], ["--passes", "x.npz"]):
        assert not set(NEW) & set(vars(cli.parse_args(line)))
    plain = vars(cli.parse_args(SPIN + ["--video", "--spin_map"]))
    with_stars = vars(cli.parse_args(SPIN + ["--video", "--spin_map", "--spin_stars", "point"]))
    assert {k: v for k, v in with_stars.items() if k != "spin_stars"} == plain
    plain = vars(cli.parse_args(SPIN))
    with_passes = vars(cli.parse_args(SPIN + ["--spin_passes", "p.npz"]))
    assert {k: v for k, v in with_passes.items() if k != "spin_passes"} == plain


# lines the parser refused before these flags existed -- the refusals the issue lists among them -- keep their last line
REFUSED_BEFORE = (
    ["--stars", "point", "--spin", "0.9"], ["--stars", "point", "--redshift", "exact"], ["--spin", "0.9", "--video", "--spin_map", "--stars", "point"],
    ["--spin", "0.9", "--passes", "x.npz"], ["--spin", "1.5"], ["--spin", "0.5", "--disk_tilt", "10"], ["--spin", "0.5", "--video", "--ray_map"],
    ["--spin_map"], ["--spin", "0.9", "--spin_map"], ["--spin", "0.9", "--video", "--spin_map", "--shutter", "0.5"],
    ["--spin", "0.9", "--video", "--spin_map", "--supersample", "2"], ["--spin", "0.9", "--spin_map_supersample", "2"],
    ["--spin", "0.9", "--video", "--spin_shutter_map"], ["--spin", "0.9", "--video", "--shutter", "0.5", "--spin_shutter_map", "--spin_map"],
    ["--spin", "0.9", "--spin_observer", "zamo", "--passes", "x.npz"], ["--spin_observer", "zamo"],
    ["--spin", "0.9", "--video", "--spin_map", "--spin_observer", "zamo"], ["--spin", "0.9", "--spin_polarization", "toroidal", "--video"],
    ["--spin", "0.9", "--video", "--spin_map", "--spin_map_supersample", "2", "--spin_polarization", "toroidal"],
    ["--shutter", "0.5"], ["--passes", "x.npz", "--video"], ["--passes", "x.txt"], ["--stars", "point", "--texture", "sky.png"],
    ["--stars", "point", "--video"], ["--spin", "0.9", "--gpus", "2"], ["--spin", "0.9", "--disk_model", "v2"],
    ["--spin", "0.9", "--video", "--shutter", "0.5"],           # (a marched shutter under a spin: the spin's own refusal, so --spin_stars' --shutter one is the drivers')
)


@pytest.mark.parametrize("line", REFUSED_BEFORE, ids=lambda l: "_".join(l).replace("--", ""))
def test_old_refusals_keep_their_words(line, capsys):
    before = _error(line, capsys)
    assert "--spin_stars" not in before and "--spin_passes" not in before
    assert _error(["--spin_stars", "point"] + line, capsys) == before
    assert _error(line + ["--spin_passes", "p.npz"], capsys) == before
    assert _error(line + ["--spin_stars", "point", "--spin_passes", "p.npz"], capsys) == before


STARS_REFUSALS = [
    ([], "--spin"),                                                              # no spin
    (SPIN + ["--texture", "sky.png"], "--texture"),
    (SPIN + ["--supersample", "2"], "--supersample"),
    (SPIN + ["--video", "--spin_map", "--spin_map_supersample", "2"], "--spin_map_supersample"),
    (SPIN + ["--video", "--shutter", "0.5", "--spin_shutter_map"], "--spin_shutter_map"),
    (SPIN + ["--spin_observer", "zamo"], "--spin_observer"),
    (SPIN + ["--spin_observer_velocity", "0.1", "0", "0"], "--spin_observer"),
    (SPIN + ["--spin_projection", "equirect"], "--spin_projection"),
    (SPIN + ["--spin_projection", "fisheye", "--spin_projection_fov", "180"], "--spin_projection"),
    (SPIN + ["--spin_polarization", "toroidal"], "--spin_polarization"),
    (SPIN + ["--video"], "--spin_map"),
    (SPIN + ["--video", "--orbit"], "--spin_map"),
]


@pytest.mark.parametrize("extra, word", STARS_REFUSALS, ids=lambda v: "_".join(v).replace("--", "") if isinstance(v, list) else None)
def test_spin_stars_refusals_name_both_flags(extra, word, capsys):
    err = _error(extra + ["--spin_stars", "point"], capsys)
    assert "--spin_stars" in err and word in err
    cli.parse_args(extra)                                         # the same line without the flag parses


def test_stars_point_beside_spin_stars_is_refused_in_the_older_words(capsys):
    """--stars point stands ahead among the refusals and refuses a spin itself; at spin 0 --spin_stars' own no-spin refusal fires.
    check_kerr_stars names the pair."""
    assert _error(SPIN + ["--stars", "point", "--spin_stars", "point"], capsys) == _error(SPIN + ["--stars", "point"], capsys)
    err = _error(["--stars", "point", "--spin_stars", "point"], capsys)
    assert "--spin_stars" in err and "--spin" in err
    with pytest.raises(ValueError, match="--stars point") as e:
        drivers.check_kerr_stars({}, spin=0.9, stars=True)
    assert "--spin_stars" in str(e.value)


def test_several_gpus_and_ranks(capsys, monkeypatch):
    """--gpus > 1 is a spin's own older refusal on the command line; check_kerr_stars names it for the drivers, and several ranks of
    a video are refused by main() before a device is touched."""
    assert _error(SPIN + ["--gpus", "2", "--spin_stars", "point"], capsys) == _error(SPIN + ["--gpus", "2"], capsys)
    for kw in (dict(gpus=2), dict(world=2)):
        with pytest.raises(ValueError, match="--gpus") as e:
            drivers.check_kerr_stars({}, spin=0.9, **kw)
        assert "--spin_stars" in str(e.value)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    with pytest.raises(ValueError, match="--spin_stars") as e:
        cli.main(SPIN + ["--video", "--spin_map", "--spin_stars", "point", "--n_frames", "2"])
    assert "ranks" in str(e.value)


@pytest.mark.parametrize("line, word", [
    (SPIN + ["--spin_stars", "point", "--star_gain", "0"], "--star_gain"),
    (SPIN + ["--spin_stars", "point", "--star_gain", "nan"], "--star_gain"),
    (SPIN + ["--spin_stars", "point", "--star_max_magnification", "0.5"], "--star_max_magnification"),
    (SPIN + ["--spin_stars", "point", "--star_max_magnification", "1e7"], "--star_max_magnification"),
])
def test_value_errors_name_their_flag(line, word, capsys):
    err = _error(line, capsys)
    assert "--spin_stars" in err and word in err


PASSES_REFUSALS = [
    ([], "--spin"),
    (SPIN + ["--video"], "--video"),
    (SPIN + ["--video", "--spin_map"], "--video"),
    (SPIN + ["--supersample", "2"], "--supersample"),
    (SPIN + ["--spin_observer", "zamo"], "--spin_observer"),
    (SPIN + ["--spin_projection", "equirect"], "--spin_projection"),
]


@pytest.mark.parametrize("extra, word", PASSES_REFUSALS, ids=lambda v: "_".join(v).replace("--", "") if isinstance(v, list) else None)
def test_spin_passes_refusals_name_both_flags(extra, word, capsys):
    err = _error(extra + ["--spin_passes", "p.npz"], capsys)
    assert "--spin_passes" in err and word in err
    cli.parse_args(extra)


def test_spin_passes_takes_a_npz_path_and_passes_keeps_refusing_a_spin(capsys):
    err = _error(SPIN + ["--spin_passes", "p.txt"], capsys)
    assert "--spin_passes" in err and ".npz" in err
    assert _error(SPIN + ["--gpus", "2", "--spin_passes", "p.npz"], capsys) == _error(SPIN + ["--gpus", "2"], capsys)
    with pytest.raises(ValueError, match="--gpus") as e:
        drivers.check_kerr_passes("p.npz", spin=0.9, gpus=2)
    assert "--spin_passes" in str(e.value)
    # --passes itself: word for word what it was
    before = _error(SPIN + ["--passes", "x.npz"], capsys)
    assert "--passes" in before and _error(SPIN + ["--passes", "x.npz", "--spin_passes", "p.npz"], capsys) == before
    with pytest.raises(ValueError, match="a spin renders on one GPU with the texture disk source and writes no passes"):
        _render_image(spin=0.9, passes_path="x.npz", kerr_passes_path="p.npz")


def _render_image(**kw):
    """drivers.render_image itself (the fixture replaced the module's name): its refusals come before make_renderer."""
    return _RENDER_IMAGE(64, 36, [6.0, 0.0, 0.5], 90.0, 0.1, **kw)


_RENDER_IMAGE = drivers.render_image


def test_render_image_refuses_before_a_renderer_is_made():
    for kw, words in ((dict(kerr_stars={}), ("--spin_stars", "--spin")),
                      (dict(spin=0.9, kerr_stars={}, skybox_path="sky.png"), ("--spin_stars", "--texture")),
                      (dict(spin=0.9, kerr_stars={}, supersample=2), ("--spin_stars", "--supersample")),
                      (dict(spin=0.9, kerr_stars={}, kerr_view=dict(observer="zamo")), ("--spin_stars", "--spin_observer")),
                      (dict(spin=0.9, kerr_stars={}, kerr_view=dict(projection="equirect")), ("--spin_stars", "--spin_projection")),
                      (dict(spin=0.9, kerr_stars=dict(gain=-1.0)), ("--spin_stars", "--star_gain")),
                      (dict(spin=0.9, kerr_stars=dict(flux=1.0)), ("--spin_stars", "flux")),
                      (dict(kerr_passes_path="p.npz"), ("--spin_passes", "--spin")),
                      (dict(spin=0.9, kerr_passes_path="p.txt"), ("--spin_passes", ".npz")),
                      (dict(spin=0.9, kerr_passes_path="p.npz", supersample=4), ("--spin_passes", "--supersample")),
                      (dict(spin=0.9, kerr_passes_path="p.npz", kerr_view=dict(velocity=(0.1, 0.0, 0.0))), ("--spin_passes", "--spin_observer"))):
        with pytest.raises(ValueError) as e:
            _render_image(**kw)
        for w in words:
            assert w in str(e.value), (kw, str(e.value))
    # the older refusals stand ahead, word for word
    with pytest.raises(ValueError, match="point stars do not combine with a spin or the exact redshift"):
        _render_image(spin=0.9, stars={}, kerr_stars={})
    with pytest.raises(ValueError, match="a spin renders on one GPU"):
        _render_image(spin=0.9, gpus=2, kerr_stars={})


def test_check_functions_need_no_device():
    assert drivers.check_kerr_stars(None) is None
    assert drivers.check_kerr_stars(None, gpus=4, video=True, stars=True) is None                 # none set: nothing to check
    assert drivers.check_kerr_stars({}, spin=0.9) == {"gain": 2.0, "max_magnification": 32.0}
    assert drivers.check_kerr_stars(dict(gain=30.0), redshift="exact") == {"gain": 30.0, "max_magnification": 32.0}
    assert drivers.check_kerr_stars(dict(max_magnification=8.0), spin=-0.5, video=True, spin_map=True) == {"gain": 2.0, "max_magnification": 8.0}
    for kw, word in ((dict(spin=0.0), "--spin"), (dict(skybox_path="sky.png"), "--texture"), (dict(stars=True), "--stars point"),
                     (dict(supersample=2), "--supersample"), (dict(spin_map_supersample=2), "--spin_map_supersample"),
                     (dict(spin_shutter_map=True), "--spin_shutter_map"), (dict(shutter=0.5), "--shutter"), (dict(spin_observer=True), "--spin_observer"),
                     (dict(spin_projection=True), "--spin_projection"), (dict(gpus=2), "--gpus"), (dict(world=2), "ranks"), (dict(video=True), "--spin_map")):
        with pytest.raises(ValueError, match=word) as e:
            drivers.check_kerr_stars({}, **{"spin": 0.9, **kw})
        assert "--spin_stars" in str(e.value)
    assert drivers.check_kerr_passes(None, gpus=4, video=True) is None
    assert drivers.check_kerr_passes("p.npz", spin=0.9) is None and drivers.check_kerr_passes("p.npz", redshift="exact") is None
    for kw, word in ((dict(spin=0.0), "--spin"), (dict(video=True), "--video"), (dict(supersample=2), "--supersample"),
                     (dict(spin_observer=True), "--spin_observer"), (dict(spin_projection=True), "--spin_projection"), (dict(gpus=2), "--gpus")):
        with pytest.raises(ValueError, match=word) as e:
            drivers.check_kerr_passes("p.npz", **{"spin": 0.9, **kw})
        assert "--spin_passes" in str(e.value)
    # what existed keeps refusing what it refused, in its own words
    with pytest.raises(ValueError, match="point stars do not combine with a spin or the exact redshift"):
        drivers.check_stars({}, spin=0.9)
    with pytest.raises(ValueError, match="--spin_map does not combine with --stars point"):
        drivers.check_spin_map(True, spin=0.9, stars=True)


def test_progress_record_names_the_stars_only_when_there_are_any():
    base = drivers.progress_params(10, 90.0, True, 0.1, 360.0, spin_map=True)
    assert "kerr_stars" not in base and "stars" not in base
    st = drivers.check_kerr_stars(dict(gain=30.0), spin=0.9, video=True, spin_map=True)
    assert drivers.progress_params(10, 90.0, True, 0.1, 360.0, spin_map=True, kerr_stars=st) == dict(base, kerr_stars={"gain": 30.0, "max_magnification": 32.0})


def test_write_passes_takes_the_hole(tmp_path):
    import numpy as np
    from bhr_amd import output
    H, W, K = 3, 4, 2
    passes = dict(steps=np.ones((H, W), np.int32), status=np.ones((H, W), np.int32), escape_dir=np.zeros((H, W, 3), np.float32),
                  crossings=np.zeros((H, W), np.int32), hits=np.zeros((K, H, W, 5), np.float32))
    output.write_passes(str(tmp_path / "a.npz"), passes)
    assert set(np.load(tmp_path / "a.npz").files) == set(passes)                        # without a hole: the file it was
    output.write_passes(str(tmp_path / "b.npz"), passes, {"bg": np.zeros((H, W, 3), np.float32)}, hole=dict(spin=-0.9, redshift="exact"))
    z = np.load(tmp_path / "b.npz")
    assert set(z.files) == set(passes) | {"bg", "spin", "redshift"} and z["spin"] == np.float32(-0.9) and str(z["redshift"]) == "exact"
    for bad in (dict(spin=0.9), dict(spin=0.9, redshift="fast"), dict(spin=0.9, redshift="model", mass=1.0)):
        with pytest.raises(ValueError, match="hole"):
            output.write_passes(str(tmp_path / "c.npz"), passes, hole=bad)


def test_the_binding_declares_the_entry_points(hip_lib):
    from bhr_amd import _lib
    for name in ("bhr_set_kerr_stars", "bhr_get_kerr_stars_info", "bhr_kerr_stars_resources"):
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name)
    # null arguments are refused without a device
    assert hip_lib.bhr_set_kerr_stars(None, None, 0, None) == _lib.BHR_ERR_INVALID
    assert b"bhr_set_kerr_stars" in hip_lib.bhr_last_error()
    assert hip_lib.bhr_get_kerr_stars_info(None, None) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_kerr_stars_resources(0, 0, None) == _lib.BHR_ERR_INVALID
