"""bhr_read_final_u16 and the dithered u8 rows (bhr_set_dither) against their NumPy restatement (tests/quant_ref.py):
exact, for injected frames of every shape class, rendered frames, row blocks, and every consumer of the u8 rows."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_ref
import quant_ref as Q
from bhr_amd import scenes

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (71, 37), (128, 128), (300, 70)]


@pytest.fixture(scope="module")
def matrix(hip_lib):
    from bhr_amd.output import dither_matrix
    m = dither_matrix()
    m.setflags(write=False)
    return m


def _renderer(w, h, **kw):
    from bhr_amd import HipRenderer
    return HipRenderer(w, h, scenes.analytic_skybox(32, 64), scenes.noisy_disk(16, 64), **kw)


def frames_for(w, h):
    """The injected frames of the issue: flat values, a dark ramp 0 .. 12/255, noise, and one of -1, 2, +inf and NaN."""
    rng = np.random.default_rng(100 * w + h)
    out = {}
    for v in (0.0, 0.0031, 0.5, 1.0):
        out[f"flat {v}"] = np.full((h, w, 3), v, np.float32)
    ramp = np.linspace(0.0, 12.0 / 255.0, w * h, dtype=np.float32).reshape(h, w)
    out["dark ramp"] = np.stack([ramp, ramp[::-1], ramp.T.reshape(h, w) if w == h else ramp * np.float32(0.5)], axis=-1)
    out["noise"] = rng.random((h, w, 3), dtype=np.float32)
    odd = np.array([-1.0, 2.0, np.inf, np.nan, -np.inf, 0.25], np.float32)
    out["non-finite"] = odd[rng.integers(0, odd.size, (h, w, 3))]
    out["non-finite"].reshape(-1)[:min(6, 3 * w * h)] = odd[:min(6, 3 * w * h)]
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in out.items()}


@pytest.mark.parametrize("size", SHAPES)
def test_injected_frames_quantise_as_the_restatement(size, matrix, hip_lib):
    from bhr_amd import _lib
    w, h = size
    r = _renderer(w, h)
    for name, frame in frames_for(w, h).items():
        r.write_layer(_lib.LAYER_FINAL, frame)
        np.testing.assert_array_equal(r.read_final_u16(), Q.quantize16(frame), err_msg=f"u16 {name}")
        np.testing.assert_array_equal(r.read_final_u8(), Q.quantize8(frame), err_msg=f"u8 {name}")
        r.set_dither("blue")
        assert r.dither == "blue"
        np.testing.assert_array_equal(r.read_final_u8(), Q.quantize8_dither(frame, matrix), err_msg=f"dither {name}")
        np.testing.assert_array_equal(r.read_final_u16(), Q.quantize16(frame), err_msg=f"u16 under dither {name}")
        r.set_dither("none")
        np.testing.assert_array_equal(r.read_final_u8(), Q.quantize8(frame), err_msg=f"u8 after dither {name}")
    r.close()


@pytest.mark.parametrize("math", ["strict", "hybrid"])
@pytest.mark.parametrize("outputs", ["f32", "u8"])
def test_rendered_default_view(math, outputs, matrix, hip_lib):
    """The 64x36 default view: both quantisers are functions of the f32 frame, whatever the frame kept in memory."""
    from bhr_amd import HipRenderer
    s = scenes.SCENES["default"]
    r = HipRenderer(64, 36, scenes.analytic_skybox(), scenes.noisy_disk(), math=math, outputs=outputs, **s["kw"])
    r.render_async(s["cam_pos"], s["fov"])
    plain = r.read_final_u8()
    final = r.read_layer(0)
    assert final.max() > 0.2
    np.testing.assert_array_equal(plain, Q.quantize8(final))
    np.testing.assert_array_equal(r.read_final_u16(), Q.quantize16(final))
    r.set_dither(1)
    np.testing.assert_array_equal(r.read_final_u8(), Q.quantize8_dither(final, matrix))     # the frame in memory, re-quantised
    r.render_async(s["cam_pos"], s["fov"])                                                     # and a frame rendered under dither
    np.testing.assert_array_equal(r.read_final_u8(), Q.quantize8_dither(final, matrix))
    np.testing.assert_array_equal(r.read_layer(0), final)
    np.testing.assert_array_equal(r.read_final_u16(), Q.quantize16(final))
    r.set_dither(0)
    np.testing.assert_array_equal(r.read_final_u8(), plain)                                    # off: the undithered rows, bit for bit
    r.render_async(s["cam_pos"], s["fov"])
    np.testing.assert_array_equal(r.read_final_u8(), plain)
    with pytest.raises(ValueError):
        r.set_dither("white")
    with pytest.raises(ValueError):
        r.set_dither(2)
    r.close()


def test_row_blocks_quantise_as_the_whole_frame(matrix, hip_lib):
    from bhr_amd import _lib
    w, h = 64, 40
    frame = frames_for(w, h)["dark ramp"] + frames_for(w, h)["noise"] * np.float32(0.01)
    whole = _renderer(w, h)
    whole.write_layer(_lib.LAYER_FINAL, frame)
    whole.set_dither("blue")
    d8, d16 = whole.read_final_u8(), whole.read_final_u16()
    np.testing.assert_array_equal(d8, Q.quantize8_dither(frame, matrix))
    for r0, r1 in ((0, 16), (16, 40)):
        t = _renderer(w, h, rows=(r0, r1))
        t.write_layer(_lib.LAYER_FINAL, frame[r0:r1])
        t.set_dither("blue")
        np.testing.assert_array_equal(t.read_final_u8(), d8[r0:r1], err_msg=f"rows {r0}..{r1}")
        np.testing.assert_array_equal(t.read_final_u16(), d16[r0:r1], err_msg=f"rows {r0}..{r1}")
        t.close()
    whole.close()


def test_jpeg_and_y4m_take_the_dithered_rows(tmp_path, matrix, hip_lib):
    from bhr_amd import _lib
    from bhr_amd.output import Y4MStream, jpeg_encode_device, jpeg_restart_interval, png_encode_device, read_y4m, rgb_to_yuv420
    w, h = 64, 36
    frame = frames_for(w, h)["dark ramp"]
    r = _renderer(w, h)
    r.write_layer(_lib.LAYER_FINAL, frame)
    plain_jpeg = jpeg_encode_device(r, 90)
    r.set_dither("blue")
    rows = Q.quantize8_dither(frame, matrix)
    assert (rows != Q.quantize8(frame)).any()
    jpeg = jpeg_encode_device(r, 90)
    assert jpeg == jpeg_ref.encode(rows, 90, jpeg_restart_interval(w))
    assert jpeg != plain_jpeg
    np.testing.assert_array_equal(Q.png_read(png_encode_device(r))[0], rows)
    path = str(tmp_path / "d.y4m")
    with Y4MStream(r, path, fps=24, slots=2) as st:
        st.submit()
        r.set_dither("none")                   # drains: the stream's frame was converted under "blue"
        st.submit()
        st.drain()
    _, planes = read_y4m(path)
    for got, want in zip(planes[0], rgb_to_yuv420(rows)):
        np.testing.assert_array_equal(got, want)
    for got, want in zip(planes[1], rgb_to_yuv420(Q.quantize8(frame))):
        np.testing.assert_array_equal(got, want)
    assert jpeg_encode_device(r, 90) == plain_jpeg
    r.close()


def test_gathers_that_store_from_the_v_pass_refuse_dither(hip_lib):
    from bhr_amd import _lib
    s = scenes.SCENES["default"]
    r = _renderer(64, 36)
    r.render_async(s["cam_pos"], s["fov"])
    plain = r.read_final_u8()
    cam = r.camera_uniforms(s["cam_pos"], s["fov"])
    ctxs = (C.c_void_p * 1)(r._ctx)
    r.set_dither("blue")
    assert hip_lib.bhr_group_render(ctxs, 1, C.byref(cam), _lib.GATHER_U8, None) == _lib.BHR_ERR_INVALID
    assert b"dither" in hip_lib.bhr_last_error()
    assert hip_lib.bhr_tile_render(r._ctx, C.byref(cam), _lib.GATHER_U8) == _lib.BHR_ERR_INVALID
    assert b"dither" in hip_lib.bhr_last_error()
    assert hip_lib.bhr_set_dither(r._ctx, 2) == _lib.BHR_ERR_INVALID
    # the f32 gather goes on working, and its rows quantise dithered afterwards
    out = np.empty((36, 64, 3), np.float32)
    _lib.check(hip_lib.bhr_group_render(ctxs, 1, C.byref(cam), 0, _lib.fptr(out)))
    from bhr_amd.output import dither_matrix
    np.testing.assert_array_equal(r.read_final_u8(), Q.quantize8_dither(out, dither_matrix()))
    r.set_dither("none")
    _lib.check(hip_lib.bhr_group_render(ctxs, 1, C.byref(cam), _lib.GATHER_U8, None))
    gathered = np.empty((36, 64, 3), np.uint8)
    _lib.check(hip_lib.bhr_read_gathered_u8(r._ctx, gathered.ctypes.data_as(C.POINTER(C.c_uint8))))
    np.testing.assert_array_equal(gathered, plain)
    np.testing.assert_array_equal(r.read_final_u8(), plain)
    r.close()
