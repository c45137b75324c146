"""The host side of the orbit map (--orbit_map, render_video(orbit_map=True)): the driver's and the command line's refusals,
the progress record, and the new entry point in the binding.  No device is touched."""
import contextlib
import io
import os

import pytest


def test_check_orbit_map_refuses_each_bad_combination():
    from bhr_amd import drivers
    # off: nothing to check
    drivers.check_orbit_map(False, video=False, orbit=False, ray_map=True, disk_tilt=20.0, shutter=0.5, supersample=4,
                            disk_model="v2", gpus=3, world=2)
    drivers.check_orbit_map(True)                             # the good one: --video --orbit, everything else at its default
    drivers.check_orbit_map(True, video=True, orbit=True, ray_map=False, disk_tilt=0.0, shutter=0.0, supersample=1,
                            disk_model="texture", gpus=1, world=1)
    drivers.check_orbit_map(True, supersample=None)           # as the renderer is set: render_video passes the renderer's factor
    for kw in (dict(video=False), dict(orbit=False), dict(ray_map=True), dict(disk_tilt=20.0), dict(disk_tilt=-0.5),
               dict(shutter=0.25), dict(supersample=2), dict(disk_model="v2"), dict(disk_model="v2_volume"), dict(gpus=2),
               dict(world=2)):
        with pytest.raises(ValueError, match="orbit_map"):
            drivers.check_orbit_map(True, **kw)
    # check_ray_map and its messages are as they were
    with pytest.raises(ValueError, match="a ray map is one view: --ray_map does not combine with --orbit"):
        drivers.check_ray_map(True, orbit=True)


def test_cli_accepts_orbit_map():
    from bhr_amd import cli
    a = cli.parse_args(["--video", "--orbit", "--orbit_map"])
    assert a.orbit_map is True and a.ray_map is False
    cli.validate_args(a)
    a = cli.parse_args(["--video", "--orbit", "--orbit_map", "--disk_tilt", "0", "--math", "fast", "--anti_alias", "lod_radius"])
    assert a.orbit_map is True
    cli.validate_args(a)
    assert cli.parse_args([]).orbit_map is False              # off by default
    assert cli.parse_args(["--video", "--orbit"]).orbit_map is False


@pytest.mark.parametrize("argv", [["--video", "--orbit_map"], ["--orbit", "--orbit_map"], ["--orbit_map"],
                                  ["--video", "--orbit", "--orbit_map", "--ray_map"],
                                  ["--video", "--orbit", "--orbit_map", "--disk_tilt", "20"],
                                  ["--video", "--orbit", "--orbit_map", "--shutter", "0.5"],
                                  ["--video", "--orbit", "--orbit_map", "--supersample", "2"],
                                  ["--video", "--orbit", "--orbit_map", "--disk_model", "v2"],
                                  ["--video", "--orbit", "--orbit_map", "--disk_model", "v2_volume"],
                                  ["--video", "--orbit", "--orbit_map", "--gpus", "2"]])
def test_cli_refuses_orbit_map_combinations_in_argument_parsing(argv, capsys):
    from bhr_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2
    assert "--orbit_map" in capsys.readouterr().err


def test_cli_still_refuses_ray_map_with_orbit(capsys):
    from bhr_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--video", "--ray_map", "--orbit"])
    assert e.value.code == 2
    assert "--ray_map does not combine with --orbit: a ray map is one view" in capsys.readouterr().err


def test_help_says_what_an_orbit_map_frame_is():
    from bhr_amd import cli
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = " ".join(buf.getvalue().split())
    assert "--orbit_map" in text
    assert "strict march of the symmetric rays, not byte-identical to the marched frame of that view" in text


def test_render_video_refuses_before_touching_the_renderer(tmp_path):
    from bhr_amd import drivers

    class NoDevice:                                           # anything but the settings the checks read is device work
        supersample = 1
        disk_tilt = 0.0
        _dv2 = None

        def __getattr__(self, name):
            raise RuntimeError(f"device work: {name}")

    class Tilted(NoDevice):
        disk_tilt = 20.0

    class Supersampled(NoDevice):
        supersample = 2

    class DiskV2(NoDevice):
        _dv2 = object()

    args = (48, 27, 6, 24, "never/v.mp4", 90, [6, 0, 0.5])
    for renderer, kw, word in ((NoDevice(), dict(orbit=False), "--orbit"), (NoDevice(), dict(orbit=True, ray_map=True), "--ray_map"),
                               (NoDevice(), dict(orbit=True, shutter=0.5), "--shutter"), (NoDevice(), dict(orbit=True, world=2), "ranks"),
                               (NoDevice(), dict(orbit=True, supersample=4), "--supersample"), (Tilted(), dict(orbit=True), "--disk_tilt"),
                               (Supersampled(), dict(orbit=True), "--supersample"), (DiskV2(), dict(orbit=True), "--disk_model")):
        with pytest.raises(ValueError, match="orbit_map") as e:
            drivers.render_video(renderer, *args, orbit_map=True, **kw)
        assert word in str(e.value), (kw, str(e.value))
    assert not os.path.exists("never")
    # the good combination passes the checks and reaches the renderer
    with pytest.raises(RuntimeError, match="device work"):
        drivers.render_video(NoDevice(), 48, 27, 6, 24, str(tmp_path / "v.mp4"), 90, [6, 0, 0.5], orbit=True, orbit_map=True)


def test_progress_params_carry_orbit_map():
    from bhr_amd.drivers import progress_params
    base = progress_params(6, 90, True, 0.1, 360.0)
    assert "orbit_map" not in base                            # a record written before the flag existed still matches a run without it
    assert progress_params(6, 90, True, 0.1, 360.0, orbit_map=False) == base
    assert progress_params(6, 90, True, 0.1, 360.0, orbit_map=True) == dict(base, orbit_map=True)
    assert progress_params(6, 90, True, 0.1, 360.0, ray_map=True) == dict(base, ray_map=True)


def test_binding_declares_the_entry_point(hip_lib):
    from bhr_amd import _lib
    assert "bhr_raymap_render_view" in _lib.SYMBOLS and hasattr(hip_lib, "bhr_raymap_render_view")
    # argument checks that need no device
    assert hip_lib.bhr_raymap_render_view(None, None, 0) == _lib.BHR_ERR_INVALID
    assert b"bhr_raymap_render_view" in hip_lib.bhr_last_error()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bhr.h")).read()
    text = " ".join(header.replace(" * ", " ").split())
    assert "bhr_raymap_render_view(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags);" in text
    assert "the strict march of the build view's rays, not bit-identical to bhr_render of `cam`" in text
