"""The grading flags of the command line, the drivers' checks and the progress record.  CPU only: nothing renders."""
import pytest


def test_defaults_are_off():
    from bhr_amd import cli
    a = cli.parse_args([])
    assert a.tonemap is None and a.exposure is None and a.white is None and a.transfer is None and a.hdr_output is None
    assert cli.grade_from_args(a) is None
    cli.validate_args(a)


def test_flags_parse():
    from bhr_amd import cli
    a = cli.parse_args(["--tonemap", "aces", "--exposure", "1.5", "--transfer", "srgb"])
    cli.validate_args(a)
    assert cli.grade_from_args(a) == dict(tonemap="aces", exposure=1.5, white=2.5, transfer="srgb")
    a = cli.parse_args(["--tonemap", "reinhard", "--white", "4"])
    assert cli.grade_from_args(a) == dict(tonemap="reinhard", exposure=0.0, white=4.0, transfer="linear")
    a = cli.parse_args(["--tonemap", "clip", "--video", "--exposure", "-16"])
    cli.validate_args(a)
    assert cli.grade_from_args(a)["exposure"] == -16.0
    for bad in (["--tonemap", "filmic"], ["--transfer", "pq"], ["--exposure", "bright"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)


@pytest.mark.parametrize("argv", [["--exposure", "1"], ["--white", "3"], ["--transfer", "srgb"], ["--hdr_output", "o/m.pfm"]])
def test_grade_flags_imply_tonemap_clip(argv):
    from bhr_amd import cli
    a = cli.parse_args(argv)
    cli.validate_args(a)
    assert a.tonemap == "clip"
    g = cli.grade_from_args(a)
    assert g["tonemap"] == "clip" and set(g) == {"tonemap", "exposure", "white", "transfer"}


@pytest.mark.parametrize("argv,msg", [
    (["--exposure", "16.5"], "exposure"), (["--exposure", "-17"], "exposure"), (["--exposure", "nan"], "exposure"),
    (["--exposure", "inf"], "exposure"), (["--white", "0"], "white"), (["--white", "-1"], "white"), (["--white", "65505"], "white"),
    (["--white", "nan"], "white"), (["--white", "inf"], "white"),
    (["--tonemap", "aces", "--gpus", "2"], "one GPU"),
    (["--hdr_output", "m.pfm", "--video"], "hdr_output"), (["--hdr_output", "m.exr"], "hdr_output"),
    (["--hdr_output", "m.png"], "hdr_output"),
])
def test_refusals(argv, msg):
    from bhr_amd import cli
    with pytest.raises(ValueError, match=msg):
        cli.validate_args(cli.parse_args(argv))


def test_hdr_output_formats_pass():
    from bhr_amd import cli
    for name in ("m.pfm", "m.hdr", "dir/M.HDR"):
        cli.validate_args(cli.parse_args(["--hdr_output", name, "--tonemap", "aces"]))


def test_check_grade():
    from bhr_amd.renderer import check_grade
    assert check_grade(None) is None and check_grade({}) is None and check_grade(dict(tonemap=None)) is None
    assert check_grade(dict(tonemap="aces")) == dict(tonemap="aces", exposure=0.0, white=2.5, transfer="linear", keep_hdr=False)
    for bad in (dict(tonemap="filmic"), dict(tonemap="clip", transfer="pq"), dict(tonemap="clip", exposure=17),
                dict(tonemap="clip", exposure=float("nan")), dict(tonemap="reinhard", white=0.0),
                dict(tonemap="reinhard", white=float("inf")), dict(tonemap="clip", gamma=2.2), dict(exposure=1.0)):
        with pytest.raises(ValueError):
            check_grade(bad)


def test_render_image_refuses_before_it_builds_a_renderer():
    from bhr_amd import drivers
    common = dict(width=64, height=36, cam_pos=[6, 0, 0.5], fov=90.0, step_size=0.1)
    with pytest.raises(ValueError, match="one GPU"):
        drivers.render_image(gpus=2, grade=dict(tonemap="aces"), **common)
    with pytest.raises(ValueError, match="hdr_path needs a grade"):
        drivers.render_image(hdr_path="m.pfm", **common)
    with pytest.raises(ValueError, match=".pfm or .hdr"):
        drivers.render_image(hdr_path="m.exr", grade=dict(tonemap="clip"), **common)
    with pytest.raises(ValueError, match="tonemap"):
        drivers.render_image(grade=dict(tonemap="filmic"), **common)


def test_progress_params_carry_the_grade_only_when_set():
    from bhr_amd import cli, drivers
    base = drivers.progress_params(10, 90.0, True, 0.1, 360.0)
    assert set(base) == {"n_frames", "fov", "orbit", "disk_rotation_speed", "orbit_degrees"}
    assert drivers.progress_params(10, 90.0, True, 0.1, 360.0, grade=None) == base
    g = cli.grade_from_args(cli.parse_args(["--tonemap", "aces", "--exposure", "1", "--transfer", "srgb", "--video"]))
    with_grade = drivers.progress_params(10, 90.0, True, 0.1, 360.0, grade=g)
    assert {k: v for k, v in with_grade.items() if k not in base} == dict(tonemap="aces", exposure=1.0, white=2.5, transfer="srgb")
    assert all(with_grade[k] == base[k] for k in base)
    other = drivers.progress_params(10, 90.0, True, 0.1, 360.0, grade=dict(g, exposure=0.5))
    assert other != with_grade and other != base                    # a resume across grades, or on and off, starts over


def test_render_video_refuses_a_bad_grade_before_it_touches_the_renderer(tmp_path):
    from bhr_amd import drivers
    with pytest.raises(ValueError, match="exposure"):
        drivers.render_video(None, 64, 36, 2, 24, str(tmp_path / "v.mp4"), 90.0, [6, 0, 0.5], grade=dict(tonemap="aces", exposure=99))
