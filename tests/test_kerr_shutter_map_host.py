"""--spin_shutter_map on the command line and in the drivers' checks (no device): parsing, the refusals naming both flags, a
default namespace without the key, render_video refusing before it touches the renderer, the progress record, and that the
lines refused before keep their words, with and without the new flag."""
import os

import pytest

from bhr_amd import cli, drivers

LINE = ["--spin", "0.9", "--video", "--shutter", "0.5", "--spin_shutter_map"]
FLAG = "--spin_shutter_map"


def _error(capsys, argv):
    with pytest.raises(SystemExit):
        cli.parse_args(argv)
    return capsys.readouterr().err


@pytest.mark.parametrize("extra", [[], ["--orbit"], ["--redshift", "exact"], ["--lens_flare"], ["--shutter_samples", "16"], ["--spin_map_supersample", "2"],
                                   ["--orbit", "--redshift", "exact", "--spin_map_supersample", "4", "--tonemap", "aces"]], ids=lambda e: " ".join(e))
def test_parsing(extra):
    a = cli.parse_args(LINE + extra)
    assert a.spin_shutter_map is True and a.shutter == 0.5 and a.supersample == 1 and a.map_supersample == 1
    assert "spin_map" not in vars(a) and a.shutter_map is False
    # the exact redshift alone is the Kerr march too
    assert cli.parse_args(["--redshift", "exact", "--video", "--shutter", "0.25", FLAG]).spin_shutter_map is True


def test_a_line_without_the_flag_has_no_key():
    for argv in ([], ["--spin", "0.9"], ["--spin", "0.9", "--video", "--spin_map"], ["--video", "--shutter", "0.5", "--shutter_map"]):
        assert "spin_shutter_map" not in vars(cli.parse_args(argv))


REFUSALS = [
    (["--video", "--shutter", "0.5", FLAG], ("needs --spin or --redshift exact", "--shutter_map")),
    (["--spin", "0.9", FLAG], ("needs --video",)),
    (["--spin", "0.9", "--video", FLAG], ("needs --shutter > 0", "--spin_map")),
    (LINE + ["--spin_map"], ("does not combine with --spin_map: that is the map of an instantaneous exposure",)),
    (LINE + ["--ray_map"], ("does not combine with --ray_map",)),
    (LINE + ["--orbit_map", "--orbit"], ("does not combine with --orbit_map",)),
    (LINE + ["--shutter_map"], ("does not combine with --shutter_map",)),
    (LINE + ["--supersample", "2"], ("--supersample",)),
    (LINE + ["--map_supersample", "2"], ("--map_supersample",)),
    (LINE + ["--spin_polarization", "toroidal"], ("does not combine with --spin_polarization",)),
    (LINE + ["--spin_observer", "zamo"], ("does not combine with --spin_observer",)),
    (LINE + ["--spin_projection", "equirect"], ("does not combine with --spin_projection",)),
    (LINE + ["--observer", "static"], ("does not combine with --observer",)),
    (LINE + ["--projection", "equirect"], ("does not combine with --projection",)),
    (LINE + ["--light_delay", "1"], ("does not combine with --light_delay",)),
    (LINE + ["--stars", "point"], ("does not combine with --stars point",)),
    (LINE + ["--polarization", "toroidal"], ("does not combine with --polarization",)),
    (LINE + ["--gpus", "2"], ("does not combine with --gpus > 1",)),
]


@pytest.mark.parametrize("argv, words", REFUSALS, ids=[" ".join(r[0][len(LINE) - 1:] if r[0][:len(LINE)] == LINE else r[0]) for r in REFUSALS])
def test_cli_refusals_name_both_flags(capsys, argv, words):
    err = _error(capsys, argv)
    assert FLAG in err, err
    for w in words:
        assert w in err, (w, err)


OK = dict(spin=0.9, shutter=0.5)
CHECK_REFUSALS = [
    (dict(shutter=0.5), ("needs --spin or --redshift exact",)),
    (dict(OK, video=False), ("needs --video",)),
    (dict(spin=0.9, shutter=0.0), ("needs --shutter > 0",)),
    (dict(OK, spin_map=True), ("--spin_map", "that is the map of an instantaneous exposure")),
    (dict(OK, ray_map=True), ("--ray_map",)),
    (dict(OK, orbit_map=True), ("--orbit_map",)),
    (dict(OK, shutter_map=True), ("--shutter_map",)),
    (dict(OK, supersample=2), ("--supersample",)),
    (dict(OK, supersample=None), ("--supersample",)),
    (dict(OK, map_supersample=2), ("--map_supersample",)),
    (dict(OK, spin_polarization=True), ("--spin_polarization",)),
    (dict(OK, spin_observer=True), ("--spin_observer",)),
    (dict(OK, spin_projection=True), ("--spin_projection",)),
    (dict(OK, observer=True), ("--observer",)),
    (dict(OK, projection=True), ("--projection",)),
    (dict(OK, light_delay=True), ("--light_delay",)),
    (dict(OK, stars=True), ("--stars point",)),
    (dict(OK, polarization=True), ("--polarization",)),
    (dict(OK, gpus=2), ("--gpus > 1",)),
    (dict(OK, world=2), ("several ranks",)),
]


@pytest.mark.parametrize("kw, words", CHECK_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in r[0].items()) for r in CHECK_REFUSALS])
def test_the_drivers_check_names_both_flags(kw, words):
    with pytest.raises(ValueError) as e:
        drivers.check_spin_shutter_map(True, **kw)
    assert FLAG in str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert drivers.check_spin_shutter_map(False, **kw) is None               # without the flag nothing is checked


def test_the_drivers_check_accepts_what_the_mode_takes():
    assert drivers.check_spin_shutter_map(True, **OK) is None
    assert drivers.check_spin_shutter_map(True, redshift="exact", shutter=1.0) is None           # the exact redshift at spin 0
    for k in (1, 2, 4, 8):
        assert drivers.check_spin_map_supersample(k, spin_shutter_map=True) is None
        assert drivers.check_spin_map_supersample(k, spin_map=True) is None


class _NoDevice:
    """A renderer that fails the test if render_video asks it for anything before the check refuses."""
    def __getattr__(self, name):
        raise AssertionError(f"render_video touched the renderer ({name}) before refusing")


@pytest.mark.parametrize("kw, words", [
    (dict(shutter=0.0), "needs --shutter > 0"),
    (dict(shutter=0.5, spin_map=True), "does not combine with --spin_map"),
    (dict(shutter=0.5, shutter_map=True), "does not combine with --shutter_map"),
    (dict(shutter=0.5, ray_map=True), "does not combine with --ray_map"),
    (dict(shutter=0.5, map_supersample=2), "--map_supersample"),
    (dict(shutter=0.5, supersample=2), "--supersample"),
    (dict(shutter=0.5, kerr_polarization=dict(field="toroidal")), "--spin_polarization"),
    (dict(shutter=0.5, kerr_view=dict(observer="zamo")), "--spin_observer"),
    (dict(shutter=0.5, kerr_view=dict(projection="equirect")), "--spin_projection"),
    (dict(shutter=0.5, observer="static"), "--observer"),
    (dict(shutter=0.5, light_delay=1.0), "--light_delay"),
    (dict(shutter=0.5, world=2, rank=1), "several ranks"),
    (dict(shutter=0.5, spin_map_supersample=3), "spin_map_supersample must be 1, 2, 4 or 8"),
])
def test_render_video_refuses_before_any_device_work(tmp_path, kw, words):
    with pytest.raises(ValueError) as e:
        drivers.render_video(_NoDevice(), 16, 8, n_frames=2, fps=24, output_path=str(tmp_path / "v.mp4"), fov=90.0, static_cam_pos=[6, 0, 0.5],
                             spin_shutter_map=True, **kw)
    assert words in str(e.value)
    if "spin_map_supersample must" not in words:
        assert FLAG in str(e.value)
    assert not list(tmp_path.iterdir())


def test_the_progress_record_carries_the_mode_only_when_set():
    base = (6, 90.0, False, 0.1, 360.0)
    old = drivers.progress_params(*base, shutter=0.5, shutter_samples=3)
    assert "spin_shutter_map" not in old
    assert drivers.progress_params(*base, shutter=0.5, shutter_samples=3, spin_shutter_map=False) == old
    new = drivers.progress_params(*base, shutter=0.5, shutter_samples=3, spin_shutter_map=True)
    assert new == {**old, "spin_shutter_map": True}
    assert drivers.progress_params(*base, shutter=0.5, shutter_samples=3, spin_shutter_map=True, spin_map_supersample=2) == {**new, "spin_map_supersample": 2}


PINNED = [
    # a spin with a shutter, without the new flag
    (["--spin", "0.9", "--video", "--shutter", "0.5"], "--spin does not combine with --shutter: shutter frames march Schwarzschild rays"),
    (["--redshift", "exact", "--video", "--shutter", "0.5"], "does not combine with --shutter: shutter frames march Schwarzschild rays"),
    # --spin_map with a shutter
    (["--spin", "0.9", "--video", "--spin_map", "--shutter", "0.5"], "--spin_map does not combine with --shutter: shutter frames are marched"),
    # a spin with the Schwarzschild shutter map, without the new flag
    (["--spin", "0.9", "--video", "--shutter", "0.5", "--shutter_map"],
     "--spin does not combine with --ray_map, --orbit_map, --shutter_map or --passes: a ray map holds Schwarzschild rays"),
    # the factor without either map
    (["--spin", "0.9", "--video", "--spin_map_supersample", "2"], "--spin_map_supersample needs --spin_map"),
    # a still image takes no shutter, whatever else is there
    (["--spin", "0.9", "--shutter", "0.5", FLAG], "--shutter needs --video"),
]


@pytest.mark.parametrize("argv, words", PINNED, ids=[" ".join(r[0]) for r in PINNED])
def test_lines_refused_before_keep_their_words(capsys, argv, words):
    assert words in _error(capsys, argv)


def test_checks_pinned_before_keep_their_words():
    with pytest.raises(ValueError, match="shutter frames are marched: --spin_map does not combine with --shutter"):
        drivers.check_spin_map(True, spin=0.9, shutter=0.5)
    with pytest.raises(ValueError, match="--spin_map needs --spin or --redshift exact: it is the ray map of the Kerr march; a hole that does not spin takes "
                                         "--ray_map or --orbit_map"):
        drivers.check_spin_map(True)
    with pytest.raises(ValueError, match="--shutter_map needs --shutter > 0: an instantaneous exposure takes --ray_map or --orbit_map"):
        drivers.check_shutter_map(True, shutter=0.0)
    with pytest.raises(ValueError) as e:
        drivers.check_spin_map_supersample(2)
    assert "needs --spin_map" in str(e.value)
    # render_video with spin_map and a shutter, without the new flag: --spin_map's own refusal
    class Spinning:
        spin, redshift, supersample = 0.9, "model", 1
    with pytest.raises(ValueError, match="shutter frames are marched: --spin_map does not combine with --shutter"):
        drivers.render_video(Spinning(), 16, 8, n_frames=2, fps=24, output_path="/nonexistent/v.mp4", fov=90.0, static_cam_pos=[6, 0, 0.5],
                             spin_map=True, shutter=0.5)


def test_binding_declares_the_entry_point(hip_lib):
    from bhr_amd import HipRenderer, _lib
    assert "bhr_kerr_raymap_render_shutter" in _lib.SYMBOLS and hasattr(hip_lib, "bhr_kerr_raymap_render_shutter")
    assert callable(HipRenderer.render_shutter_from_kerr_ray_map_async)
    # argument checks that need no device
    assert hip_lib.bhr_kerr_raymap_render_shutter(None, None, 2, 0) == _lib.BHR_ERR_INVALID
    assert b"bhr_kerr_raymap_render_shutter" in hip_lib.bhr_last_error()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bhr.h")).read()
    text = " ".join(header.replace(" * ", " ").split())
    assert "bhr_kerr_raymap_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags);" in text
    assert '"kerr_raymap_shutter_fused" BHR_KERR_RAYMAP_SHUTTER_FUSED' in text
    assert "Not available: shutter frames from this map" not in text
