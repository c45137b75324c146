"""--polarization on the command line and in the drivers: the flags parse, they are absent from the default namespace, a line
refused without them is refused with the same words with them, every new refusal names its flag, and check_polarization accepts
and rejects the right values before any device is touched.  No GPU."""
import pytest

from bhr_amd import cli, drivers

NEW = ("polarization", "polarization_fraction", "polarization_cell", "stokes_output", "polarization_ticks")


def test_the_flags_parse():
    a = cli.parse_args(["--polarization", "toroidal"])
    assert a.polarization == ["toroidal"]
    assert cli.polarization_from_args(a) == {"polarization": {"field": (0.0, 1.0, 0.0), "fraction": 0.7, "cell": 16}}
    a = cli.parse_args(["--polarization", "0.3", "0.8", "0.5", "--polarization_fraction", "1", "--polarization_cell", "8", "--stokes_output", "s.npz",
                        "--polarization_ticks", "t.png"])
    assert cli.polarization_from_args(a) == {"polarization": {"field": (0.3, 0.8, 0.5), "fraction": 1.0, "cell": 8}, "stokes_path": "s.npz",
                                             "ticks_path": "t.png"}
    assert cli.polarization_from_args(cli.parse_args(["--polarization", "-1", "0", "2.5"]))["polarization"]["field"] == (-1.0, 0.0, 2.5)
    assert cli.polarization_from_args(cli.parse_args([])) == {}
    # what works with it: a tilted disk with anti-aliasing, the lens flare, grading, point stars, any --math, a map video
    a = cli.parse_args(["--polarization", "vertical", "--disk_tilt", "25", "--anti_alias", "lod_radius", "--lens_flare", "--tonemap", "aces",
                        "--stars", "point", "--math", "fast"])
    cli.validate_args(a)
    a = cli.parse_args(["--polarization", "radial", "--video", "--ray_map", "--stokes_output", "v.npz"])
    cli.validate_args(a)
    assert cli.polarization_from_args(a) == {"polarization": {"field": (1.0, 0.0, 0.0), "fraction": 0.7, "cell": 16}, "stokes_path": "v.npz"}


def test_the_default_namespace_has_no_new_key():
    for line in ([], ["--video", "--orbit", "--supersample", "2"], ["--spin", "0.5"], ["--observer", "circular"], ["--light_delay"]):
        plain = vars(cli.parse_args(line))
        assert not set(NEW) & set(plain)
    plain = vars(cli.parse_args(["--video", "--ray_map"]))
    with_pol = vars(cli.parse_args(["--video", "--ray_map", "--polarization", "toroidal"]))
    assert {k: v for k, v in with_pol.items() if k != "polarization"} == plain


# lines the parser refused before this flag existed: the same words with --polarization toroidal in front
REFUSED_BEFORE = (
    ["--shutter", "0.5"], ["--spin", "1.5"], ["--spin", "0.5", "--disk_tilt", "10"], ["--spin", "0.5", "--video", "--ray_map"],
    ["--observer_sky", "shift"], ["--observer", "circular", "--spin", "0.3"], ["--map_supersample", "2"],
    ["--video", "--shutter_map"], ["--orbit_map"], ["--video", "--orbit", "--ray_map"], ["--ray_map"],
    ["--video", "--ray_map", "--supersample", "2"], ["--passes", "x.npz", "--video"], ["--stars", "point", "--texture", "sky.png"],
    ["--stars", "point", "--video"], ["--projection_fov", "100"], ["--projection", "fisheye", "--spin", "0.5"],
    ["--light_delay", "20"], ["--light_delay", "--spin", "0.5"], ["--light_delay", "--video", "--ray_map"],
)


def _error(line, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(line)
    assert e.value.code == 2
    return capsys.readouterr().err.strip().splitlines()[-1]


@pytest.mark.parametrize("line", REFUSED_BEFORE, ids=lambda l: "_".join(l).replace("--", ""))
def test_old_refusals_keep_their_words(line, capsys):
    before = _error(line, capsys)
    assert "polarization" not in before
    assert _error(["--polarization", "toroidal"] + line, capsys) == before
    assert _error(line + ["--polarization", "0.3", "0.8", "0.5", "--polarization_cell", "8"], capsys) == before


@pytest.mark.parametrize("extra, word", [
    (["--spin", "0.7"], "--spin"),
    (["--redshift", "exact"], "--redshift exact"),
    (["--observer", "circular"], "--observer"),
    (["--observer_velocity", "0.1", "0.2", "0.3"], "--observer_velocity"),
    (["--projection", "equirect"], "--projection equirect"),
    (["--projection", "fisheye"], "--projection fisheye"),
    (["--video", "--orbit", "--orbit_map"], "--orbit_map"),
    (["--video", "--shutter", "0.5", "--shutter_map"], "--shutter_map"),
    (["--video", "--shutter", "0.5"], "--shutter"),
    (["--video", "--ray_map", "--map_supersample", "2"], "--map_supersample"),
    (["--supersample", "2"], "--supersample"),
    (["--disk_model", "v2"], "--disk_model"),
    (["--disk_model", "v2_volume"], "--disk_model"),
    (["--gpus", "2"], "--gpus"),
    (["--video"], "--ray_map"),
    (["--video", "--orbit"], "--ray_map"),
])
def test_new_refusals_name_their_flag(extra, word, capsys):
    err = _error(extra + ["--polarization", "toroidal"], capsys)
    assert "--polarization" in err and word in err
    cli.parse_args(extra)                                         # the same line without the flag parses


def test_light_delay_with_polarization_is_refused_in_light_delays_words(capsys):
    """--light_delay stands ahead of --polarization among the refusals: it has none for it, so the polarisation's own fires."""
    err = _error(["--light_delay", "--polarization", "toroidal"], capsys)
    assert "--polarization" in err and "--light_delay" in err


@pytest.mark.parametrize("line, word", [
    (["--polarization", "spiral"], "spiral"), (["--polarization", "1", "2"], "three"), (["--polarization", "0", "0", "0"], "zero"),
    (["--polarization", "toroidal", "--polarization_fraction", "1.5"], "polarization_fraction"),
    (["--polarization", "toroidal", "--polarization_fraction", "nan"], "polarization_fraction"),
    (["--polarization", "toroidal", "--polarization_cell", "12"], "polarization_cell"),
    (["--polarization", "toroidal", "--stokes_output", "s.txt"], "--stokes_output"),
    (["--polarization", "toroidal", "--polarization_ticks", "t.jpg"], "--polarization_ticks"),
    (["--polarization", "toroidal", "--video", "--ray_map", "--polarization_ticks", "t.png"], "--polarization_ticks"),
    (["--polarization_fraction", "0.5"], "--polarization_fraction"), (["--polarization_cell", "8"], "--polarization_cell"),
    (["--stokes_output", "s.npz"], "--stokes_output"), (["--polarization_ticks", "t.png"], "--polarization_ticks"),
])
def test_value_errors_name_their_flag(line, word, capsys):
    err = _error(line, capsys)
    assert word in err and ("polarization" in err or "--stokes_output" in err)


def test_check_polarization_needs_no_device():
    assert drivers.check_polarization(None) is None
    assert drivers.check_polarization(None, spin=0.9, gpus=4, video=True) is None                 # none set: nothing to check
    assert drivers.check_polarization(dict(field="toroidal")) == {"field": (0.0, 1.0, 0.0), "fraction": 0.7, "cell": 16}
    assert drivers.check_polarization(dict(field=(0.3, 0.8, 0.5), fraction=1.0, cell=32), video=True, ray_map=True, stokes_path="a.npz") == \
        {"field": (0.3, 0.8, 0.5), "fraction": 1.0, "cell": 32}
    pol = dict(field="radial")
    for kw, word in ((dict(spin=0.5), "spin"), (dict(redshift="exact"), "exact redshift"), (dict(observer=True), "observer"),
                     (dict(projection=True), "projection"), (dict(light_delay=True), "light_delay"), (dict(orbit_map=True), "orbit_map"),
                     (dict(shutter_map=True), "shutter_map"), (dict(shutter=0.5), "shutter"), (dict(map_supersample=2), "map_supersample"),
                     (dict(supersample=2), "supersample"), (dict(disk_model="v2"), "disk_model"), (dict(disk_model="v2_volume"), "disk_model"),
                     (dict(gpus=2), "one GPU"), (dict(world=2), "one GPU"), (dict(video=True), "ray_map"),
                     (dict(video=True, ray_map=True, ticks_path="t.png"), "polarization_ticks"), (dict(stokes_path="s.txt"), "npz"),
                     (dict(ticks_path="t.jpg"), "png")):
        with pytest.raises(ValueError, match=word) as e:
            drivers.check_polarization(pol, **kw)
        assert "polarization" in str(e.value) or "stokes_output" in str(e.value)
    for bad in (dict(field="spiral"), dict(field="toroidal", fraction=-0.1), dict(field="toroidal", cell=4), dict(fraction=0.5),
                dict(field="toroidal", gain=2.0)):
        with pytest.raises(ValueError, match="polarization"):
            drivers.check_polarization(bad)
    for kw in (dict(stokes_path="s.npz"), dict(ticks_path="t.png")):
        with pytest.raises(ValueError, match="need a polarization"):
            drivers.check_polarization(None, **kw)


def test_progress_record_names_the_polarisation_only_when_set():
    base = drivers.progress_params(10, 90.0, False, 0.1, 360.0, ray_map=True)
    assert "polarization" not in base
    pol = drivers.check_polarization(dict(field="toroidal", cell=8))
    with_pol = drivers.progress_params(10, 90.0, False, 0.1, 360.0, ray_map=True, polarization=pol)
    assert with_pol == dict(base, polarization={"field": [0.0, 1.0, 0.0], "fraction": 0.7, "cell": 8})


def test_the_binding_declares_the_entry_points(hip_lib):
    import ctypes as C
    from bhr_amd import _lib
    for name in ("bhr_set_polarization", "bhr_read_stokes", "bhr_read_stokes_cells", "bhr_stokes_resources"):
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name)
    assert C.sizeof(_lib.Polarization) == 32
    # null arguments are refused without a device
    assert hip_lib.bhr_set_polarization(None, None) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_read_stokes(None, 0, None) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_read_stokes_cells(None, None, None) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_stokes_resources(0, None) == _lib.BHR_ERR_INVALID
