"""The 16-bit PNG paths on the device (csrc/png_device.hip), the sinks, and the command line end to end: every file is
read back with tests/quant_ref.py's reader (CRCs, Adler-32, filters at a stride of 6) and compared sample for sample."""
import json
import os
import sys

import numpy as np
import pytest

import quant_ref as Q
from bhr_amd import scenes
from test_gpu_quantisers import SHAPES, _renderer, frames_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matrix(hip_lib):
    from bhr_amd.output import dither_matrix
    return dither_matrix()


def _check_file(data, want, w, h, hip_lib, what):
    assert len(data) <= hip_lib.bhr_png16_device_bound(w, h), what
    img, info = Q.png_read(data)
    assert (info["width"], info["height"], info["bit_depth"], info["idat_chunks"]) == (w, h, 16, h), what
    np.testing.assert_array_equal(img, want, err_msg=what)
    return info


@pytest.mark.parametrize("size", SHAPES)
def test_device_png16_decodes_to_the_u16_rows(size, hip_lib):
    from bhr_amd import _lib
    from bhr_amd.output import png_encode_device
    w, h = size
    r, r2 = _renderer(w, h), _renderer(w, h)
    frames = frames_for(w, h)
    frames["all 65535"] = np.ones((h, w, 3), np.float32)
    seen = set()
    for name, frame in frames.items():
        r.write_layer(_lib.LAYER_FINAL, frame)
        data = png_encode_device(r, bit_depth=16)
        u16 = r.read_final_u16()
        np.testing.assert_array_equal(u16, Q.quantize16(frame), err_msg=name)
        seen |= set(_check_file(data, u16, w, h, hip_lib, f"{w}x{h} {name}")["filters"])
        assert png_encode_device(r, bit_depth=16) == data, f"{name}: a second encode differs"
        r2.write_layer(_lib.LAYER_FINAL, frame)
        assert png_encode_device(r2, bit_depth=16) == data, f"{name}: a second context encodes differently"
        # the 8-bit file of the same frame is untouched by the 16-bit tables living beside its own
        np.testing.assert_array_equal(Q.png_read(png_encode_device(r))[0], Q.quantize8(frame), err_msg=name)
    if w * h > 1000:
        assert len(seen) >= 2, seen                                        # the filter choice is alive
    with pytest.raises(ValueError):
        png_encode_device(r, bit_depth=12)
    r.close()
    r2.close()


def test_device_png16_width_limit(hip_lib):
    from bhr_amd import _lib
    from bhr_amd.output import FrameSink, DEVICE, png_encode_device
    wmax = hip_lib.bhr_png16_device_max_width()
    assert 7680 <= wmax < hip_lib.bhr_png_device_max_width()
    assert hip_lib.bhr_png16_device_bound(wmax + 1, 2) == 0 < hip_lib.bhr_png16_device_bound(wmax, 2)
    r = _renderer(wmax, 2)
    rng = np.random.default_rng(2)
    frame = rng.random((2, wmax, 3), dtype=np.float32)
    frame[:, ::2] *= np.float32(0.01)
    r.write_layer(_lib.LAYER_FINAL, frame)
    _check_file(png_encode_device(r, bit_depth=16), Q.quantize16(frame), wmax, 2, hip_lib, "maximum width")
    r.close()
    r = _renderer(wmax + 1, 2)
    r.write_layer(_lib.LAYER_FINAL, np.zeros((2, wmax + 1, 3), np.float32))
    out = np.empty(1 << 20, np.uint8)
    import ctypes as C
    n = C.c_int64(0)
    rc = hip_lib.bhr_png16_encode_device(r._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size, C.byref(n))
    assert rc == _lib.BHR_ERR_INVALID and b"host encoder" in hip_lib.bhr_last_error()
    with pytest.raises(ValueError, match="host encoder"):
        png_encode_device(r, bit_depth=16)
    with pytest.raises(ValueError, match="host encoder"):
        FrameSink(r, slots=2, workers=1, level=DEVICE, bit_depth=16)
    np.testing.assert_array_equal(r.read_final_u16(), 0)                       # the context is still usable
    np.testing.assert_array_equal(Q.png_read(png_encode_device(r))[0], 0)      # and the 8-bit encoder takes the width
    r.close()


CAMS = [([6, 0, 0.5], 90), ([5, 2, 1.0], 80), ([-7, 1, 0.3], 70), ([3.2, 0.5, 0.12], 100), ([5, 2, 1.0], 80)]


def _loop(tmp, slots, sink_kw, dither="none"):
    """Renders CAMS with a scene update between the frames (the disk texture alternates) through a sink; -> file bytes."""
    from bhr_amd import HipRenderer
    from bhr_amd.output import FrameSink
    tex = [scenes.noisy_disk(), scenes.noisy_disk()[::-1].copy()]
    r = HipRenderer(96, 54, scenes.analytic_skybox(), tex[0], math="hybrid", frame_slots=slots)
    r.set_dither(dither)
    os.makedirs(tmp, exist_ok=True)
    with FrameSink(r, slots=3, workers=2, **sink_kw) as sink:
        for k, (c, f) in enumerate(CAMS):
            r.update_disk_texture(tex[k & 1])
            r.render_async(c, f)
            sink.submit(os.path.join(tmp, f"f{k}.png"))
        frames, _ = sink.drain()
    assert frames == len(CAMS)
    last16, last8 = r.read_final_u16(), r.read_final_u8()
    r.close()
    return [open(os.path.join(tmp, f"f{k}.png"), "rb").read() for k in range(len(CAMS))], last16, last8


@pytest.mark.parametrize("level", [-1, 1])
def test_png16_sink_two_slots_write_what_one_slot_writes(level, tmp_path, hip_lib):
    one, u16, _ = _loop(str(tmp_path / "one"), 1, dict(level=level, bit_depth=16))
    two, u16_two, _ = _loop(str(tmp_path / "two"), 2, dict(level=level, bit_depth=16))
    assert one == two
    np.testing.assert_array_equal(u16, u16_two)
    imgs = [Q.png_read(d) for d in one]
    assert all(i[1]["bit_depth"] == 16 for i in imgs)
    np.testing.assert_array_equal(imgs[-1][0], u16)
    assert (imgs[0][0] != imgs[1][0]).any()                                # the view moved
    assert (imgs[1][0] != imgs[4][0]).any()                                # the same view again under the other disk texture
    assert imgs[0][0].max() > 20000
    assert not [f for f in os.listdir(tmp_path / "two") if f.endswith(".tmp")]


@pytest.mark.parametrize("level", [-1, 1])
def test_dithered_8bit_sink_two_slots_write_what_one_slot_writes(level, tmp_path, matrix, hip_lib):
    one, _, u8 = _loop(str(tmp_path / "one"), 1, dict(level=level), dither="blue")
    two, _, _ = _loop(str(tmp_path / "two"), 2, dict(level=level), dither="blue")
    plain, u16, u8_plain = _loop(str(tmp_path / "plain"), 2, dict(level=level))
    assert one == two
    np.testing.assert_array_equal(Q.png_read(one[-1])[0], u8)
    assert (u8 != u8_plain).any()
    # a dithered pixel is the truncated one or the level above it
    d = Q.png_read(one[-1])[0].astype(np.int32) - Q.png_read(plain[-1])[0].astype(np.int32)
    assert set(np.unique(d).tolist()) <= {0, 1} and d.any()


def _tiny_cli(monkeypatch):
    """The command line at 64x36: "-r sd" is pointed at a tiny frame for the test (the flags' own paths are untouched)."""
    from bhr_amd import cli
    monkeypatch.setitem(cli.RESOLUTIONS, "sd", (64, 36))
    return cli


def test_cli_stills(tmp_path, monkeypatch, matrix, hip_lib):
    from bhr_amd import drivers
    cli = _tiny_cli(monkeypatch)
    captured = []
    render_image = drivers.render_image
    monkeypatch.setattr(drivers, "render_image", lambda *a, **k: captured.append(render_image(*a, **k)) or captured[-1])
    common = ["-r", "sd", "--n_stars", "100"]
    assert cli.main(common + ["-o", str(tmp_path / "deep.png"), "--bit_depth", "16"]) == 0
    img, info = Q.png_read((tmp_path / "deep.png").read_bytes())
    assert (info["width"], info["height"], info["bit_depth"]) == (64, 36, 16)
    np.testing.assert_array_equal(img, Q.quantize16(captured[-1]))
    assert img.max() > 5000
    assert cli.main(common + ["-o", str(tmp_path / "blue.png"), "--dither", "blue"]) == 0
    img, info = Q.png_read((tmp_path / "blue.png").read_bytes())
    assert info["bit_depth"] == 8
    np.testing.assert_array_equal(img, Q.quantize8_dither(captured[-1], matrix))
    assert (img != Q.quantize8(captured[-1])).any()
    with pytest.raises(ValueError, match="dither"):
        cli.main(common + ["-o", str(tmp_path / "no.png"), "--bit_depth", "16", "--dither", "blue"])
    assert not os.path.exists(tmp_path / "no.png")


def test_cli_video_16bit(tmp_path, monkeypatch, hip_lib):
    from bhr_amd import drivers, mp4
    cli = _tiny_cli(monkeypatch)
    monkeypatch.setenv("PATH", str(tmp_path / "no_such_dir"))                # no ffmpeg ...
    monkeypatch.setitem(sys.modules, "imageio", None)                       # ... and no pyav: the frames themselves are muxed
    out = str(tmp_path / "vid" / "v.mp4")
    common = ["-r", "sd", "--n_stars", "100", "--video", "--orbit", "--n_frames", "6", "--orbit_degrees", "60", "--fps", "6",
              "-o", out]
    assert cli.main(common + ["--bit_depth", "16"]) == 0
    d = drivers._frames_dir(out)
    assert sorted(f for f in os.listdir(d) if f.startswith("frame_")) == [f"frame_{k:04d}.png" for k in range(6)]
    files = [open(os.path.join(d, f"frame_{k:04d}.png"), "rb").read() for k in range(6)]
    imgs = [Q.png_read(f) for f in files]
    assert all((i[1]["width"], i[1]["height"], i[1]["bit_depth"]) == (64, 36, 16) for i in imgs)
    assert imgs[0][0].max() > 5000 and (imgs[0][0] != imgs[5][0]).any()
    info = mp4.read_samples(out)
    assert (info["width"], info["height"], info["duration"], info["object_type"]) == (64, 36, 6, 0x6D)
    video = open(out, "rb").read()
    assert [video[o:o + s] for o, s in info["samples"]] == files
    prog = json.load(open(os.path.join(d, "progress.json")))
    assert prog["params"]["bit_depth"] == 16 and "dither" not in prog["params"] and prog["completed"] == list(range(6))
    # a resume with another depth does not take these frames over: it starts again and writes 8-bit files
    assert cli.main(common + ["--resume"]) == 0
    again = [Q.png_read(open(os.path.join(d, f"frame_{k:04d}.png"), "rb").read()) for k in range(6)]
    assert all(i[1]["bit_depth"] == 8 for i in again)
    assert "bit_depth" not in json.load(open(os.path.join(d, "progress.json")))["params"]
