"""The host side of the ray map: the passes file, the derived hit radius / azimuth, the command line's refusals and the
progress record.  No device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _passes(h=5, w=7, k=2, nc=5, seed=0):
    rng = np.random.default_rng(seed)
    crossings = rng.integers(0, 4, (h, w)).astype(np.int32)
    hits = rng.normal(size=(k, h, w, nc)).astype(np.float32)
    hits[np.arange(k)[:, None, None] >= np.minimum(crossings, k)[None]] = 0
    return dict(steps=rng.integers(1, 900, (h, w)).astype(np.int32), status=rng.integers(0, 3, (h, w)).astype(np.int32),
                escape_dir=rng.normal(size=(h, w, 3)).astype(np.float32), crossings=crossings, hits=hits)


def test_hit_polar_on_hand_made_records():
    from bhr_amd.output import hit_polar
    hits = np.zeros((2, 1, 4, 5), dtype=np.float32)
    hits[0, 0, 0, :2] = (3.0, 4.0)
    hits[0, 0, 1, :2] = (0.0, -2.5)
    hits[0, 0, 2, :2] = (-7.0, 0.0)
    hits[1, 0, 2, :2] = (100.0, 100.0)                    # a second crossing: not the one the passes derive from
    crossings = np.array([[1, 1, 2, 0]], dtype=np.int32)
    r, phi = hit_polar(hits, crossings)
    assert r.dtype == phi.dtype == np.float32 and r.shape == phi.shape == (1, 4)
    np.testing.assert_array_equal(r[0, :3], np.float32([5.0, 2.5, 7.0]))
    np.testing.assert_array_equal(phi[0, :3], np.arctan2(np.float32([4.0, -2.5, 0.0]), np.float32([3.0, 0.0, -7.0])))
    np.testing.assert_allclose(phi[0, :3], [np.arctan2(4.0, 3.0), -np.pi / 2, np.pi], rtol=1e-6)
    assert np.isnan(r[0, 3]) and np.isnan(phi[0, 3])      # no crossing
    # float32 arithmetic in the march's order: two products, a sum, a root
    x, y = np.float32(2.7182817), np.float32(-3.1415927)
    hits[0, 0, 0, :2] = (x, y)
    assert hit_polar(hits, crossings)[0][0, 0] == np.sqrt(np.float32(x * x) + np.float32(y * y), dtype=np.float32)
    with pytest.raises(ValueError):
        hit_polar(hits[..., :4], crossings)
    with pytest.raises(ValueError):
        hit_polar(hits, crossings[:, :3])


@pytest.mark.parametrize("nc", [5, 9])
def test_write_passes_round_trip(nc, tmp_path):
    from bhr_amd.output import hit_polar, write_passes
    h, w, k = 40, 64, 4
    p = _passes(h, w, k, nc)
    p["hit_r"], p["hit_phi"] = hit_polar(p["hits"], p["crossings"])
    rng = np.random.default_rng(1)
    layers = {name: rng.random((h, w, 3), dtype=np.float32) for name in ("bg", "disk", "blur")}
    p["steps"] = p["steps"].astype(np.int64)              # stored as int32 whatever it came as
    path = str(tmp_path / "sub" / "passes.npz")
    write_passes(path, p, layers)
    z = np.load(path)
    assert sorted(z.files) == sorted(["steps", "status", "escape_dir", "crossings", "hits", "hit_r", "hit_phi", "bg", "disk", "blur"])
    for name in ("steps", "status", "crossings"):
        assert z[name].dtype == np.int32 and z[name].shape == (h, w)
        np.testing.assert_array_equal(z[name], p[name])
    for name, shape in (("escape_dir", (h, w, 3)), ("hits", (k, h, w, nc)), ("hit_r", (h, w)), ("hit_phi", (h, w)),
                        ("bg", (h, w, 3)), ("disk", (h, w, 3)), ("blur", (h, w, 3))):
        assert z[name].dtype == np.float32 and z[name].shape == shape
        np.testing.assert_array_equal(z[name], p[name] if name in p else layers[name])      # NaN compares equal here
    # compressed: the hit planes are mostly zeros
    raw = sum(z[name].nbytes for name in z.files)
    assert os.path.getsize(path) < raw
    import zipfile
    with zipfile.ZipFile(path) as zf:
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in zf.infolist())
    # without layers, and the refusals
    write_passes(str(tmp_path / "bare.npz"), _passes())
    assert "bg" not in np.load(str(tmp_path / "bare.npz")).files
    with pytest.raises(ValueError):
        write_passes(str(tmp_path / "passes.npy"), p)
    with pytest.raises(ValueError):
        write_passes(path, {k_: v for k_, v in p.items() if k_ != "hits"})
    with pytest.raises(ValueError):
        write_passes(path, p, {"final": layers["bg"]})
    with pytest.raises(ValueError):
        write_passes(path, p, {"bg": layers["bg"][:, :-1]})
    with pytest.raises(ValueError):
        write_passes(path, dict(p, status=p["status"][:-1]))


@pytest.mark.parametrize("extra", [["--orbit"], ["--shutter", "0.5"], ["--supersample", "2"], ["--disk_model", "v2"],
                                   ["--disk_model", "v2_volume"], ["--gpus", "2"]])
def test_cli_refuses_ray_map_combinations_in_argument_parsing(extra, capsys):
    from bhr_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--video", "--ray_map"] + extra)
    assert e.value.code == 2
    assert "--ray_map" in capsys.readouterr().err


def test_cli_ray_map_and_passes_flags(capsys):
    from bhr_amd import cli
    a = cli.parse_args(["--video", "--ray_map", "--math", "fast"])
    assert a.ray_map is True and a.passes is None
    cli.validate_args(a)
    a = cli.parse_args([])
    assert a.ray_map is False and a.passes is None        # off by default
    a = cli.parse_args(["--passes", "out/p.npz"])
    assert a.passes == "out/p.npz"
    cli.validate_args(a)
    for argv in (["--ray_map"], ["--passes", "p.npz", "--video"], ["--passes", "p.txt"], ["--passes", "p.npz", "--gpus", "2"],
                 ["--passes", "p.npz", "--supersample", "4"], ["--passes", "p.npz", "--disk_model", "v2"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2
    capsys.readouterr()
    import io
    import contextlib
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = " ".join(buf.getvalue().split())
    assert "--ray_map" in text and "--passes" in text and "strict arithmetic's whatever --math says" in text


def test_drivers_refuse_before_any_device_work():
    from bhr_amd import drivers
    drivers.check_ray_map(False, orbit=True, shutter=0.5, supersample=4, disk_model="v2", gpus=3)      # off: nothing to check
    drivers.check_ray_map(True)
    for kw in (dict(orbit=True), dict(shutter=0.25), dict(supersample=2), dict(disk_model="v2"), dict(disk_model="v2_volume"),
               dict(gpus=2), dict(world=2)):
        with pytest.raises(ValueError, match="ray_map"):
            drivers.check_ray_map(True, **kw)
    drivers.check_passes(None, gpus=4)
    drivers.check_passes("a/b.npz")
    for args in (("p.png",), ("p.npz", 2), ("p.npz", 1, 2), ("p.npz", 1, 1, "v2")):
        with pytest.raises(ValueError):
            drivers.check_passes(*args)

    class NoDevice:                                       # render_video refuses before it touches the renderer's device side
        supersample = 1
        _dv2 = None

        def __getattr__(self, name):
            raise RuntimeError(f"device work: {name}")
    with pytest.raises(ValueError, match="orbit"):
        drivers.render_video(NoDevice(), 48, 27, 6, 24, "never/v.mp4", 90, [6, 0, 0.5], orbit=True, ray_map=True)
    assert not os.path.exists("never")


def test_progress_params_carry_ray_map():
    from bhr_amd.drivers import progress_params
    base = progress_params(6, 90, False, 0.1, 360.0)
    assert "ray_map" not in base                          # a record written before the flag existed still matches a run without it
    assert progress_params(6, 90, False, 0.1, 360.0, ray_map=False) == base
    assert progress_params(6, 90, False, 0.1, 360.0, ray_map=True) == dict(base, ray_map=True)


def test_info_struct_matches_the_header(hip_lib, tmp_path):
    from bhr_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bhr.h"\nint main(void){printf("%zu %zu %zu %zu\\n",'
                   'sizeof(bhr_raymap_info),offsetof(bhr_raymap_info,crossings_stored),offsetof(bhr_raymap_info,ray_steps),'
                   'offsetof(bhr_raymap_info,cam));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_cs, o_rs, o_cam = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    I = _lib.RayMapInfo
    assert (C.sizeof(I), I.crossings_stored.offset, I.ray_steps.offset, I.cam.offset) == (size, o_cs, o_rs, o_cam)
    for name in ("bhr_raymap_build", "bhr_raymap_render", "bhr_raymap_read", "bhr_raymap_get_info", "bhr_raymap_free"):
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name)
    # argument checks that need no device
    assert hip_lib.bhr_raymap_render(None, 0.0, 0) == _lib.BHR_ERR_INVALID and b"bhr_raymap_render" in hip_lib.bhr_last_error()
    assert hip_lib.bhr_raymap_build(None, None, 0) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_raymap_free(None) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_raymap_get_info(None, None) == _lib.BHR_ERR_INVALID
