"""--light_delay on the command line, in the drivers and at the ABI's door: it parses bare and with a scale, it is absent from the
default namespace, its refusals fire before any device is touched, the keyword reaches the drivers and the progress record only
when it is set, and the two entry points refuse null arguments without a device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from bhr_amd import cli, drivers


# ---- parsing and defaults -----------------------------------------------------------------------------------------------------------
def test_light_delay_parses():
    assert cli.parse_args(["--light_delay"]).light_delay == 1.0                    # bare: the physical delay
    assert cli.parse_args(["--light_delay", "2.5"]).light_delay == 2.5
    assert cli.parse_args(["--light_delay", "0"]).light_delay == 0.0
    assert cli.parse_args(["--light_delay", "--video"]).light_delay == 1.0         # bare ahead of another flag
    assert cli.light_delay_from_args(cli.parse_args(["--light_delay", "16"])) == {"light_delay": 16.0}
    assert cli.light_delay_from_args(cli.parse_args([])) == {}
    # what works with it: plain supersampling, a tilted disk, the lens flare, grading, HDR, video, an orbit, any --math
    a = cli.parse_args(["--light_delay", "--supersample", "2", "--disk_tilt", "20", "--lens_flare", "--tonemap", "aces", "--video", "--orbit",
                        "--video_hdr", "pq", "--math", "fast"])
    cli.validate_args(a)
    cli.parse_args(["--light_delay", "3", "--video", "--video_codec", "mjpeg", "--bit_depth", "8", "--hdr_output", "x.pfm"])


def test_the_default_namespace_has_no_light_delay():
    assert "light_delay" not in vars(cli.parse_args([]))
    for line in (["--video", "--orbit", "--supersample", "2"], ["--spin", "0.5"], ["--observer", "circular"], ["--projection", "fisheye"]):
        plain = vars(cli.parse_args(line))
        assert "light_delay" not in plain
        if line[0] == "--video":
            with_delay = vars(cli.parse_args(line + ["--light_delay"]))
            assert {k: v for k, v in with_delay.items() if k != "light_delay"} == plain and with_delay["light_delay"] == 1.0


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
FLAGS = (["--light_delay"], ["--light_delay", "2.5"], ["--light_delay", "0"])


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "_".join(f).strip("-"))
@pytest.mark.parametrize("extra, word", [
    (["--anti_alias", "lod_radius"], "--anti_alias"),
    (["--disk_model", "v2"], "--disk_model"),
    (["--disk_model", "v2_volume"], "--disk_model"),
    (["--supersample", "2", "--supersample_threshold", "0.1"], "--supersample_threshold"),
    (["--gpus", "2"], "--gpus"),
    (["--spin", "0.7"], "--spin"),
    (["--redshift", "exact"], "--redshift exact"),
    (["--observer", "circular"], "--observer"),
    (["--observer_velocity", "0.1", "0.2", "0.3"], "--observer_velocity"),
    (["--observer", "infall", "--video", "--infall_to", "2"], "--infall_to"),
    (["--projection", "equirect"], "--projection equirect"),
    (["--projection", "fisheye", "--projection_fov", "200"], "--projection fisheye"),
    (["--passes", "x.npz"], "--passes"),
    (["--video", "--shutter", "0.5"], "--shutter"),
    (["--video", "--ray_map"], "--ray_map"),
    (["--video", "--orbit", "--orbit_map"], "--orbit_map"),
    (["--video", "--shutter", "0.5", "--shutter_map"], "--shutter"),
    (["--stars", "point"], "--stars point"),
])
def test_light_delay_refusals_are_argparse_errors(flags, extra, word, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(extra + flags)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--light_delay" in err and word in err
    cli.parse_args(extra)                                         # the same line without the flag parses
    cli.parse_args(flags)


@pytest.mark.parametrize("value", ("-0.5", "16.5", "nan", "inf", "wide"))
def test_light_delay_scale_errors(value, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--light_delay", value])
    assert e.value.code == 2
    assert "--light_delay" in capsys.readouterr().err


def test_driver_checks_need_no_device():
    assert drivers.check_light_delay(None, anti_alias="lod_radius", gpus=4, spin=0.9, observer=True) is None      # no delay: nothing to check
    assert drivers.check_light_delay(1) == 1.0 and drivers.check_light_delay(0.0) == 0.0 and drivers.check_light_delay(16.0) == 16.0
    for kw, word in ((dict(anti_alias="lod_radius"), "anti_alias"), (dict(disk_model="v2"), "disk_model"), (dict(disk_model="v2_volume"), "disk_model"),
                     (dict(supersample_threshold=0.1), "supersample_threshold"), (dict(gpus=2), "one GPU"), (dict(world=2), "one rank"),
                     (dict(spin=0.5), "spin"), (dict(redshift="exact"), "exact redshift"), (dict(observer=True), "observer"),
                     (dict(projection=True), "projection"), (dict(passes=True), "passes"), (dict(shutter=0.5), "shutter"),
                     (dict(maps=True), "ray_map"), (dict(stars=True), "point stars")):
        for scale in (0.0, 1.0, 2.5):
            with pytest.raises(ValueError, match="light_delay") as e:
                drivers.check_light_delay(scale, **kw)
            assert word in str(e.value)
    for scale in (-0.1, 16.1, float("nan"), float("inf"), "wide", (1.0, 2.0)):
        with pytest.raises(ValueError, match="light_delay"):
            drivers.check_light_delay(scale)
    with pytest.raises(ValueError, match="light_delay"):          # the drivers refuse before any device work
        drivers.render_image(64, 32, [6, 0, 0.5], 90.0, 0.1, light_delay=1.0, spin=0.5)
    with pytest.raises(ValueError, match="light_delay"):
        drivers.render_image(64, 32, [6, 0, 0.5], 90.0, 0.1, light_delay=1.0, gpus=2)
    with pytest.raises(ValueError, match="light_delay"):
        drivers.render_image(64, 32, [6, 0, 0.5], 90.0, 0.1, light_delay=1.0, observer=(0.1, 0.0, 0.0))
    with pytest.raises(ValueError, match="light_delay"):
        drivers.render_image(64, 32, [6, 0, 0.5], 90.0, 0.1, light_delay=1.0, projection="equirect")
    with pytest.raises(ValueError, match="light_delay"):
        drivers.render_image(64, 32, [6, 0, 0.5], 90.0, 0.1, light_delay=17.0)


# ---- the keyword reaches the drivers and the progress record only when it is set -------------------------------------------------------
def _run_main(monkeypatch, argv):
    seen = {}

    def render_image(**kw):
        seen["image"] = kw
        return np.zeros((2, 2, 3), dtype=np.float32)

    class Renderer:
        def close(self):
            pass

    def make_renderer(*a, **kw):
        seen["renderer"] = (a, kw)
        return Renderer(), None, None, None

    def render_video(renderer, width, height, **kw):
        seen["video"] = dict(kw, width=width, height=height)

    monkeypatch.setattr(drivers, "render_image", render_image)
    monkeypatch.setattr(drivers, "make_renderer", make_renderer)
    monkeypatch.setattr(drivers, "render_video", render_video)
    monkeypatch.setattr(drivers, "save_image", lambda *a, **kw: None)
    assert cli.main(argv) == 0
    return seen


def test_the_default_passes_no_keyword(monkeypatch):
    for argv in ([], ["--observer", "circular"], ["--supersample", "2"], ["--projection", "fisheye"]):
        assert "light_delay" not in _run_main(monkeypatch, argv)["image"], argv
        assert "light_delay" not in _run_main(monkeypatch, argv + ["--video"])["video"], argv


def test_the_light_delay_reaches_the_drivers(monkeypatch):
    kw = _run_main(monkeypatch, ["--light_delay"])["image"]
    assert kw["light_delay"] == 1.0 and "observer" not in kw and "projection" not in kw and (kw["width"], kw["height"]) == (1920, 1080)
    kw = _run_main(monkeypatch, ["--light_delay", "2.5", "-r", "hd", "--supersample", "2", "--math", "fast"])["image"]
    assert kw["light_delay"] == 2.5 and kw["supersample"] == 2 and kw["math"] == "fast"
    seen = _run_main(monkeypatch, ["--light_delay", "0", "-r", "sd", "--video", "--orbit"])
    assert seen["video"]["light_delay"] == 0.0 and seen["video"]["orbit"] is True and seen["renderer"][0][:2] == (640, 360)
    assert _run_main(monkeypatch, ["--light_delay", "--video"])["video"]["light_delay"] == 1.0


def test_several_ranks_are_refused_before_a_renderer_exists(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setattr(drivers, "make_renderer", lambda *a, **kw: pytest.fail("a renderer was made"))
    with pytest.raises(ValueError, match="light_delay.*one rank"):
        cli.main(["--light_delay", "--video"])


def test_progress_params_carry_the_light_delay_only_when_set():
    base = drivers.progress_params(4, 90.0, True, 0.1, 360.0)
    assert "light_delay" not in base
    p = drivers.progress_params(4, 90.0, True, 0.1, 360.0, light_delay=1.0)
    assert p == {**base, "light_delay": 1.0}
    assert drivers.progress_params(4, 90.0, True, 0.1, 360.0, light_delay=0.0) == {**base, "light_delay": 0.0}     # 0 is a setting too
    other = drivers.progress_params(4, 90.0, True, 0.1, 360.0, light_delay=2.5)
    assert other != p and other != base                           # a resume under another scale starts over


def test_the_renderer_refuses_what_the_delay_does_not_combine_with():
    """HipRenderer.render_async checks the keyword ahead of the camera and the library: no context is needed to see it."""
    from bhr_amd import HipRenderer
    r = object.__new__(HipRenderer)                               # no __init__: no device
    for kw in (dict(observer=(0.1, 0.0, 0.0)), dict(projection="equirect"), dict(math="strict"), dict(math="fast")):
        with pytest.raises(ValueError, match="light_delay"):
            HipRenderer.render_async(r, [6, 0, 0.5], 90.0, light_delay=1.0, **kw)
    for scale in (-1.0, 16.5, float("nan")):
        with pytest.raises(ValueError, match="light_delay"):
            HipRenderer.render_async(r, [6, 0, 0.5], 90.0, light_delay=scale)


# ---- the ABI without a device -------------------------------------------------------------------------------------------------------------
def test_null_arguments_are_refused_without_a_device(hip_lib):
    from bhr_amd import _lib
    assert {"bhr_render_delayed", "bhr_delayed_resources"} <= set(_lib.SYMBOLS)
    assert C.sizeof(_lib.LightDelay) == 8
    cam, d = _lib.Camera(), _lib.LightDelay(1.0, 0)
    assert hip_lib.bhr_render_delayed(None, C.byref(cam), C.byref(d), 0) == _lib.BHR_ERR_INVALID
    msg = hip_lib.bhr_last_error().decode()
    assert "bhr_render_delayed" in msg and "null" in msg
    assert hip_lib.bhr_render_delayed(None, None, None, 0) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_delayed_resources(0, None) == _lib.BHR_ERR_INVALID
    msg = hip_lib.bhr_last_error().decode()
    assert "bhr_delayed_resources" in msg and "null" in msg
    assert hip_lib.bhr_delayed_resources(1, None) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_abi_version() == 1
