"""The host side of motion blur from the ray map (--shutter_map, render_video(shutter_map=True),
HipRenderer.render_shutter_from_ray_map_async): the driver's and the command line's refusals, the progress record, the argument
checks of the Python surface and the new entry point in the binding.  No device is touched."""
import contextlib
import io
import os

import pytest


def test_check_shutter_map_accepts_and_refuses_each_combination():
    from bhr_amd import drivers
    # off: nothing to check
    drivers.check_shutter_map(False, shutter=0.0, orbit=True, ray_map=True, orbit_map=True, disk_tilt=20.0, supersample=4,
                              disk_model="v2", gpus=3, world=2)
    drivers.check_shutter_map(True)                            # the good one: an open shutter, everything else at its default
    drivers.check_shutter_map(True, shutter=0.5, orbit=True, ray_map=False, orbit_map=False, disk_tilt=0.0, supersample=1,
                              disk_model="texture", gpus=1, world=1)
    drivers.check_shutter_map(True, shutter=1.0, orbit=False, disk_tilt=25.0)      # a camera that stands still takes any disk
    drivers.check_shutter_map(True, supersample=None)          # as the renderer is set: render_video passes the renderer's factor
    for kw in (dict(shutter=0.0), dict(shutter=0), dict(ray_map=True), dict(orbit_map=True), dict(orbit=True, orbit_map=True),
               dict(orbit=True, disk_tilt=20.0), dict(orbit=True, disk_tilt=-0.5), dict(supersample=2), dict(disk_model="v2"),
               dict(disk_model="v2_volume"), dict(gpus=2), dict(world=2)):
        with pytest.raises(ValueError, match="shutter_map"):
            drivers.check_shutter_map(True, **kw)
    # check_ray_map, check_orbit_map and their messages are as they were: the two maps of an instantaneous exposure refuse a shutter
    with pytest.raises(ValueError, match="shutter frames are marched: --ray_map does not combine with --shutter"):
        drivers.check_ray_map(True, shutter=0.5)
    with pytest.raises(ValueError, match="shutter frames are marched: --orbit_map does not combine with --shutter"):
        drivers.check_orbit_map(True, shutter=0.5)


def test_cli_accepts_shutter_map():
    from bhr_amd import cli
    a = cli.parse_args(["--video", "--shutter", "0.5", "--shutter_map"])
    assert a.shutter_map is True and a.ray_map is False and a.orbit_map is False
    cli.validate_args(a)
    a = cli.parse_args(["--video", "--orbit", "--shutter", "0.5", "--shutter_samples", "8", "--shutter_map", "--math", "fast"])
    assert a.shutter_map is True
    cli.validate_args(a)
    a = cli.parse_args(["--video", "--shutter", "1", "--shutter_map", "--disk_tilt", "25"])      # still camera, tilted disk
    assert a.shutter_map is True
    assert cli.parse_args([]).shutter_map is False             # off by default
    assert cli.parse_args(["--video", "--shutter", "0.5"]).shutter_map is False


@pytest.mark.parametrize("argv", [["--shutter_map"], ["--video", "--shutter_map"], ["--video", "--shutter", "0", "--shutter_map"],
                                  ["--video", "--shutter", "0.5", "--shutter_map", "--ray_map"],
                                  ["--video", "--orbit", "--shutter", "0.5", "--shutter_map", "--orbit_map"],
                                  ["--video", "--orbit", "--shutter", "0.5", "--shutter_map", "--disk_tilt", "20"],
                                  ["--video", "--shutter", "0.5", "--shutter_map", "--supersample", "2"],
                                  ["--video", "--shutter", "0.5", "--shutter_map", "--disk_model", "v2"],
                                  ["--video", "--shutter", "0.5", "--shutter_map", "--disk_model", "v2_volume"],
                                  ["--video", "--shutter", "0.5", "--shutter_map", "--gpus", "2"]])
def test_cli_refuses_shutter_map_combinations_in_argument_parsing(argv, capsys):
    from bhr_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2
    assert "--shutter_map" in capsys.readouterr().err


@pytest.mark.parametrize("flag", ["--ray_map", "--orbit_map"])
def test_cli_still_refuses_the_other_maps_with_a_shutter(flag, capsys):
    from bhr_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--video", "--orbit", flag, "--shutter", "0.5"] if flag == "--orbit_map" else ["--video", flag, "--shutter", "0.5"])
    assert e.value.code == 2
    assert f"{flag} does not combine with --shutter: shutter frames are marched" in capsys.readouterr().err


def test_help_says_what_a_shutter_map_frame_is():
    from bhr_amd import cli
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = " ".join(buf.getvalue().split())
    assert "--shutter_map" in text
    assert "no sample is marched" in text


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
    on = dict(shutter=0.5, shutter_samples=4)
    for renderer, kw, word in ((NoDevice(), dict(shutter=0.0), "--shutter > 0"), (NoDevice(), dict(on, ray_map=True), "--ray_map"),
                               (NoDevice(), dict(on, orbit=True, orbit_map=True), "--orbit_map"), (NoDevice(), dict(on, world=2), "ranks"),
                               (NoDevice(), dict(on, supersample=4), "--supersample"), (Tilted(), dict(on, orbit=True), "--disk_tilt"),
                               (Supersampled(), on, "--supersample"), (DiskV2(), on, "--disk_model")):
        with pytest.raises(ValueError, match="shutter_map") as e:
            drivers.render_video(renderer, *args, shutter_map=True, **kw)
        assert word in str(e.value), (kw, str(e.value))
    assert not os.path.exists("never")
    # the good combinations pass the checks and reach the renderer: an orbit, and a still camera over a tilted disk
    with pytest.raises(RuntimeError, match="device work"):
        drivers.render_video(NoDevice(), 48, 27, 6, 24, str(tmp_path / "v.mp4"), 90, [6, 0, 0.5], orbit=True, shutter_map=True, **on)
    with pytest.raises(RuntimeError, match="device work"):
        drivers.render_video(Tilted(), 48, 27, 6, 24, str(tmp_path / "w.mp4"), 90, [6, 0, 0.5], orbit=False, shutter_map=True, **on)


def test_progress_params_carry_shutter_map_only_when_set():
    from bhr_amd.drivers import progress_params
    base = progress_params(6, 90, True, 0.1, 360.0, shutter=0.5, shutter_samples=4)
    assert "shutter_map" not in base                          # a record written before the flag existed still matches a run without it
    assert progress_params(6, 90, True, 0.1, 360.0, shutter=0.5, shutter_samples=4, shutter_map=False) == base
    assert progress_params(6, 90, True, 0.1, 360.0, shutter=0.5, shutter_samples=4, shutter_map=True) == dict(base, shutter_map=True)
    assert progress_params(6, 90, True, 0.1, 360.0, shutter=0.5, shutter_samples=4, orbit_map=True) == dict(base, orbit_map=True)


def test_renderer_rejects_mismatched_lists_before_any_device_work():
    from bhr_amd import HipRenderer

    class NoDevice:
        lens_flare = False

        def __getattr__(self, name):
            raise RuntimeError(f"device work: {name}")

    call = HipRenderer.render_shutter_from_ray_map_async
    with pytest.raises(ValueError, match="2 camera positions for 3 t_offsets"):
        call(NoDevice(), [0.0, 0.1, 0.2], [[6, 0, 0.5], [6, 0.1, 0.5]], 90.0)
    with pytest.raises(ValueError, match="0 camera positions for 1 t_offsets"):
        call(NoDevice(), [0.0], [], 90.0)
    with pytest.raises(ValueError, match="needs fov"):
        call(NoDevice(), [0.0, 0.1], [[6, 0, 0.5], [6, 0.1, 0.5]])
    with pytest.raises(RuntimeError, match="device work"):     # matching lists pass the checks and reach the device
        call(NoDevice(), [0.0, 0.1], [[6, 0, 0.5], [6, 0.1, 0.5]], 90.0)


def test_binding_declares_the_entry_point(hip_lib):
    from bhr_amd import _lib
    assert "bhr_raymap_render_shutter" in _lib.SYMBOLS and hasattr(hip_lib, "bhr_raymap_render_shutter")
    # argument checks that need no device
    assert hip_lib.bhr_raymap_render_shutter(None, None, 2, 0) == _lib.BHR_ERR_INVALID
    assert b"bhr_raymap_render_shutter" in hip_lib.bhr_last_error()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bhr.h")).read()
    text = " ".join(header.replace(" * ", " ").split())
    assert "bhr_raymap_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags);" in text
    assert '"raymap_shutter_fused" BHR_RAYMAP_SHUTTER_FUSED' in text
