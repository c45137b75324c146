"""The host side of supersampled ray maps (option "raymap_supersample", --map_supersample): the command line, the drivers'
refusals before any device work, the progress record and the info struct.  No device is touched."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = (["--ray_map"], ["--orbit", "--orbit_map"], ["--shutter", "0.5", "--shutter_map"])


@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("mode", MAPS)
def test_cli_accepts_the_factor_with_each_map(mode, k):
    from bhr_amd import cli
    a = cli.parse_args(["--video"] + mode + ["--map_supersample", str(k)])
    assert a.map_supersample == k and a.supersample == 1
    cli.validate_args(a)


def test_cli_defaults_and_help(capsys):
    from bhr_amd import cli
    assert cli.parse_args([]).map_supersample == 1
    assert cli.parse_args(["--video", "--ray_map"]).map_supersample == 1
    assert cli.parse_args(["--map_supersample", "1"]).map_supersample == 1        # 1 is no factor: nothing to refuse
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = " ".join(buf.getvalue().split())
    assert "--map_supersample" in text
    assert text.count("a supersampled map takes --map_supersample") == 3           # the three map flags point to it


@pytest.mark.parametrize("argv", [["--map_supersample", "2"], ["--video", "--map_supersample", "4"],
                                  ["--video", "--orbit", "--map_supersample", "2"], ["--video", "--supersample", "2", "--map_supersample", "2"],
                                  ["--video", "--ray_map", "--map_supersample", "3"], ["--video", "--ray_map", "--map_supersample", "0"],
                                  ["--video", "--ray_map", "--map_supersample", "16"], ["--video", "--ray_map", "--map_supersample", "two"]])
def test_cli_refuses_in_argument_parsing(argv, capsys):
    from bhr_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2
    assert "--map_supersample" in capsys.readouterr().err


@pytest.mark.parametrize("mode,flag", [(MAPS[0], "--ray_map"), (MAPS[1], "--orbit_map"), (MAPS[2], "--shutter_map")])
def test_cli_still_refuses_supersample_with_a_map(mode, flag, capsys):
    from bhr_amd import cli
    for extra in ([], ["--map_supersample", "2"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["--video"] + mode + ["--supersample", "2"] + extra)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert flag in err and "a ray map holds one ray per pixel" in err          # the existing message


def test_check_map_supersample():
    from bhr_amd.drivers import check_map_supersample
    check_map_supersample(1)
    check_map_supersample(1, False, False, False)
    for k in (1, 2, 4, 8):
        check_map_supersample(k, ray_map=True)
        check_map_supersample(k, orbit_map=True)
        check_map_supersample(k, shutter_map=True)
    for k in (2, 4, 8):
        with pytest.raises(ValueError, match="map_supersample"):
            check_map_supersample(k)
    for k in (0, 3, 16, -2, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="map_supersample"):
            check_map_supersample(k, ray_map=True)


def test_render_video_refuses_before_any_device_work():
    from bhr_amd import drivers

    class NoDevice:                                       # render_video refuses before it touches the renderer's device side
        supersample = 1
        _dv2 = None
        disk_tilt = 0.0

        def __getattr__(self, name):
            raise RuntimeError(f"device work: {name}")
    args = (NoDevice(), 48, 27, 6, 24, "never/v.mp4", 90, [6, 0, 0.5])
    with pytest.raises(ValueError, match="map_supersample"):
        drivers.render_video(*args, map_supersample=2)                         # no map
    with pytest.raises(ValueError, match="map_supersample"):
        drivers.render_video(*args, ray_map=True, map_supersample=3)
    with pytest.raises(ValueError, match="map_supersample"):
        drivers.render_video(*args, orbit=True, orbit_map=True, map_supersample=16)
    with pytest.raises(ValueError, match="map_supersample"):
        drivers.render_video(*args, shutter=0.5, shutter_map=True, map_supersample=0)
    with pytest.raises(ValueError, match="one ray per pixel"):                 # the renderer's own factor stays refused
        drivers.render_video(*args, ray_map=True, supersample=2, map_supersample=2)
    assert not os.path.exists("never")


def test_progress_params_carry_the_factor():
    from bhr_amd.drivers import progress_params
    for kw in (dict(ray_map=True), dict(orbit_map=True), dict(shutter=0.5, shutter_map=True)):
        base = progress_params(6, 90, False, 0.1, 360.0, **kw)
        assert "map_supersample" not in base              # a record written before the factor existed still matches a run without it
        assert progress_params(6, 90, False, 0.1, 360.0, map_supersample=1, **kw) == base
        for k in (2, 4, 8):
            assert progress_params(6, 90, False, 0.1, 360.0, map_supersample=k, **kw) == dict(base, map_supersample=k)
    assert progress_params(6, 90, False, 0.1, 360.0, ray_map=True, map_supersample=2) != progress_params(6, 90, False, 0.1, 360.0, ray_map=True, map_supersample=4)


def test_info_struct_has_the_factor_where_reserved_was(hip_lib, tmp_path):
    from bhr_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bhr.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",'
                   'sizeof(bhr_raymap_info),offsetof(bhr_raymap_info,supersample),offsetof(bhr_raymap_info,rows),'
                   'offsetof(bhr_raymap_info,crossings_stored),sizeof(((bhr_raymap_info*)0)->supersample));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_ss, o_rows, o_cs, sz_ss = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    I = _lib.RayMapInfo
    assert (o_ss, sz_ss, o_rows, o_cs) == (20, 4, 16, 24)
    assert size == 120 == 24 + 4 * 8 + C.sizeof(_lib.Camera)     # what it was with `reserved`: six i32, four 64-bit words, the camera
    assert (C.sizeof(I), I.supersample.offset, I.supersample.size, I.rows.offset, I.crossings_stored.offset) == (size, 20, 4, 16, 24)
    # the option's refusals need a context; the entry point's own need none
    assert hip_lib.bhr_set_option(None, b"raymap_supersample", 2.0) == _lib.BHR_ERR_INVALID
