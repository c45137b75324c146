"""--spin_map_supersample on the command line and in the drivers' checks (no device): parsing beside what --spin_map takes,
the refusals naming both flags, a default namespace without the key, the progress record, and that the lines --spin_map refused
before keep their words."""
import pytest

from bhr_amd import cli, drivers

LINE = ["--spin", "0.6", "--video", "--spin_map"]


def _error(capsys, argv):
    with pytest.raises(SystemExit):
        cli.parse_args(argv)
    return capsys.readouterr().err


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_parsing(k):
    a = cli.parse_args(LINE + ["--spin_map_supersample", str(k)])
    assert a.spin_map_supersample == k and a.spin_map is True and a.supersample == 1 and a.map_supersample == 1


@pytest.mark.parametrize("extra", [["--orbit"], ["--redshift", "exact"], ["--lens_flare"], ["--tonemap", "aces", "--exposure", "1"],
                                   ["--orbit", "--redshift", "exact", "--lens_flare", "--tonemap", "reinhard"]], ids=lambda e: " ".join(e))
def test_parsing_beside_what_spin_map_takes(extra):
    a = cli.parse_args(LINE + ["--spin_map_supersample", "2"] + extra)
    assert a.spin_map_supersample == 2
    # the exact redshift alone is the Kerr march too
    assert cli.parse_args(["--redshift", "exact", "--video", "--spin_map", "--spin_map_supersample", "4"]).spin_map_supersample == 4


def test_a_line_without_the_flag_has_no_key():
    for argv in ([], LINE, ["--spin", "0.6"], ["--video", "--ray_map", "--map_supersample", "2"]):
        assert "spin_map_supersample" not in vars(cli.parse_args(argv))


REFUSALS = [
    # the factor without --spin_map: both flags by name
    (["--spin", "0.6", "--video", "--spin_map_supersample", "2"], ("--spin_map_supersample", "needs --spin_map")),
    (["--spin", "0.6", "--spin_map_supersample", "2"], ("--spin_map_supersample", "needs --spin_map")),
    (["--video", "--ray_map", "--spin_map_supersample", "2"], ("--spin_map_supersample", "needs --spin_map")),
    # ... with --spin_polarization
    (LINE + ["--spin_map_supersample", "2", "--spin_polarization", "toroidal"], ("--spin_map_supersample", "does not combine with --spin_polarization")),
    # no factor of three
    (LINE + ["--spin_map_supersample", "3"], ("--spin_map_supersample", "invalid choice")),
    # --spin_map's own restrictions hold with the factor
    (["--video", "--spin_map", "--spin_map_supersample", "2"], ("--spin_map needs --spin or --redshift exact",)),
    (["--spin", "0.6", "--spin_map", "--spin_map_supersample", "2"], ("--spin_map needs --video",)),
    (LINE + ["--spin_map_supersample", "2", "--shutter", "0.5"], ("--spin_map does not combine with --shutter",)),
    (LINE + ["--spin_map_supersample", "2", "--gpus", "2"], ("--spin_map does not combine with --gpus other than 1",)),
    (LINE + ["--spin_map_supersample", "2", "--ray_map"], ("--spin_map does not combine with --ray_map",)),
    # the lines --spin_map refused before read as before, with the factor and without it
    (LINE + ["--map_supersample", "2"], ("--spin_map does not combine with --map_supersample other than 1: a Kerr ray map has no supersampled form",)),
    (LINE + ["--supersample", "2"], ("--spin_map does not combine with --supersample other than 1: a Kerr ray map holds one ray per pixel",)),
    (LINE + ["--spin_map_supersample", "2", "--map_supersample", "2"],
     ("--spin_map does not combine with --map_supersample other than 1: a Kerr ray map has no supersampled form",)),
    (LINE + ["--spin_map_supersample", "2", "--supersample", "2"],
     ("--spin_map does not combine with --supersample other than 1: a Kerr ray map holds one ray per pixel",)),
]


@pytest.mark.parametrize("argv, words", REFUSALS, ids=[" ".join(r[0]) for r in REFUSALS])
def test_refusals(capsys, argv, words):
    err = _error(capsys, argv)
    for w in words:
        assert w in err, (w, err)


def test_the_drivers_check_makes_the_same_refusals():
    for k in (1, 2, 4, 8):
        assert drivers.check_spin_map_supersample(k, spin_map=True) is None
    assert drivers.check_spin_map_supersample(1) is None                       # the default without the map: nothing to refuse
    assert drivers.check_spin_map_supersample(1, spin_map=True, spin_polarization=True) is None
    for bad in (0, 3, 16, -2, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="spin_map_supersample must be 1, 2, 4 or 8"):
            drivers.check_spin_map_supersample(bad, spin_map=True)
    for k in (2, 4, 8):
        with pytest.raises(ValueError) as e:
            drivers.check_spin_map_supersample(k)
        assert "--spin_map_supersample" in str(e.value) and "needs --spin_map" in str(e.value)
        with pytest.raises(ValueError) as e:
            drivers.check_spin_map_supersample(k, spin_map=True, spin_polarization=True)
        assert "--spin_map_supersample" in str(e.value) and "--spin_polarization" in str(e.value)
    # the checks that refused a supersampled Kerr map under the old names still do, word for word
    with pytest.raises(ValueError, match="a Kerr ray map has no supersampled form: --spin_map does not combine with --map_supersample > 1"):
        drivers.check_spin_map(True, spin=0.6, map_supersample=2)
    with pytest.raises(ValueError, match="a Kerr ray map holds one ray per pixel: --spin_map does not combine with --supersample > 1"):
        drivers.check_spin_map(True, spin=0.6, supersample=2)


class _NoDevice:
    """A renderer that fails the test if render_video asks it for anything before the check refuses."""
    def __getattr__(self, name):
        raise AssertionError(f"render_video touched the renderer ({name}) before refusing")


@pytest.mark.parametrize("kw, words", [
    (dict(spin_map=True, spin_map_supersample=3), "spin_map_supersample must be 1, 2, 4 or 8"),
    (dict(spin_map_supersample=2), "needs --spin_map"),
    (dict(spin_map=True, spin_map_supersample=2, kerr_polarization=dict(field="toroidal")), "--spin_polarization"),
])
def test_render_video_refuses_before_any_device_work(tmp_path, kw, words):
    with pytest.raises(ValueError) as e:
        drivers.render_video(_NoDevice(), 16, 8, n_frames=2, fps=24, output_path=str(tmp_path / "v.mp4"), fov=90.0, static_cam_pos=[6, 0, 0.5], **kw)
    assert words in str(e.value)
    assert not (tmp_path / "v_frames").exists() and not list(tmp_path.iterdir())


def test_the_progress_record_carries_the_factor_only_above_one():
    base = (6, 90.0, False, 0.1, 360.0)
    old = drivers.progress_params(*base, spin_map=True)
    assert "spin_map_supersample" not in old and old["spin_map"] is True
    assert drivers.progress_params(*base, spin_map=True, spin_map_supersample=1) == old       # an old record still matches
    two = drivers.progress_params(*base, spin_map=True, spin_map_supersample=2)
    assert two == {**old, "spin_map_supersample": 2}
    assert drivers.progress_params(*base, spin_map=True, spin_map_supersample=4) != two       # a resume with another factor starts over
    assert "spin_map_supersample" not in drivers.progress_params(*base)
