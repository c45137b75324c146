"""The device JPEG encoder (csrc/jpeg_device.hip) against its NumPy restatement (tests/jpeg_ref.py): byte for byte."""
import io
import os

import numpy as np
import pytest

import jpeg_ref
from bhr_amd import scenes


def _frame(w, h, **kw):
    from bhr_amd import HipRenderer
    r = HipRenderer(w, h, scenes.analytic_skybox(), scenes.noisy_disk(), **kw)
    r.render_async([6, 0, 0.5], 90)
    return r


def _first_difference(a, b):
    n = min(len(a), len(b))
    at = next((i for i in range(n) if a[i] != b[i]), n)
    return f"lengths {len(a)} / {len(b)}, first difference at byte {at}: {a[max(at - 4, 0):at + 8].hex()} / {b[max(at - 4, 0):at + 8].hex()}"


def _same(dev, ref):
    assert dev == ref, _first_difference(dev, ref)


def _decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(256, 144), (97, 33), (1, 1), (2, 5), (33, 17), (1920, 64), (3840, 16), (7680, 8), (64, 1080),
                                  (32, 2160), (16, 4320)])
def test_device_jpeg_is_the_restatement(size, hip_lib):
    from bhr_amd.output import jpeg_encode_device, jpeg_restart_interval
    w, h = size
    r = _frame(w, h)
    data = jpeg_encode_device(r, 90)
    u8 = r.read_final_u8()
    _same(data, jpeg_ref.encode(u8, 90, jpeg_restart_interval(w)))
    assert _decode(data).shape == (h, w, 3)
    assert len(data) <= hip_lib.bhr_jpeg_device_bound(w, h)
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("quality", [1, 50, 100])
def test_device_jpeg_is_the_restatement_at_other_qualities(quality, hip_lib):
    from bhr_amd.output import jpeg_encode_device, jpeg_restart_interval
    r = _frame(256, 144)
    _same(jpeg_encode_device(r, quality), jpeg_ref.encode(r.read_final_u8(), quality, jpeg_restart_interval(256)))
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("quality", [90, 100])
def test_device_jpeg_of_extreme_frames(quality, hip_lib):
    """Black, white, a ramp, noise and a 0/255 frame through write_layer: long 0xFF runs in the data (stuffing), zero runs
    above 15 (ZRL), the largest coefficients; every file is the restatement's and stays inside the bound."""
    from bhr_amd import _lib
    from bhr_amd.output import jpeg_encode_device, jpeg_restart_interval
    w, h = 320, 90
    r = _frame(w, h)
    rng = np.random.default_rng(11)
    sizes = {}
    for name, frame in (("black", np.zeros((h, w, 3), np.float32)), ("white", np.ones((h, w, 3), np.float32)),
                        ("ramp", np.broadcast_to(np.linspace(0, 1, w, dtype=np.float32)[None, :, None], (h, w, 3)).copy()),
                        ("noise", rng.random((h, w, 3), dtype=np.float32)),
                        ("bilevel", rng.integers(0, 2, (h, w, 3)).astype(np.float32))):
        r.write_layer(_lib.LAYER_FINAL, frame)
        data = jpeg_encode_device(r, quality)
        u8 = r.read_final_u8()
        np.testing.assert_array_equal(u8, (np.clip(frame, 0, 1) * 255).astype(np.uint8), err_msg=name)
        ref = jpeg_ref.encode(u8, quality, jpeg_restart_interval(w))
        assert data == ref, f"{name}: {_first_difference(data, ref)}"
        assert _decode(data).shape == (h, w, 3)
        assert len(data) <= hip_lib.bhr_jpeg_device_bound(w, h)
        sizes[name] = len(data)
    print(f"[jpeg] {w}x{h} q {quality}: {sizes}")
    assert sizes["black"] < w * h * 3 / 50 and sizes["white"] < w * h * 3 / 50
    r.close()


@pytest.mark.gpu
def test_whole_fhd_frame(hip_lib):
    """One fhd frame at quality 90: decodes with libjpeg to 1920x1080; no worse than libjpeg's own encoding of the same u8
    frame with the same tables (MSE at most 1.02 x); the same bytes on a second encode and from a second context."""
    from PIL import Image
    from bhr_amd.output import jpeg_encode_device
    r = _frame(1920, 1080)
    data = jpeg_encode_device(r, 90)
    u8 = r.read_final_u8()
    dec = _decode(data)
    assert dec.shape == (1080, 1920, 3)
    ql, qc = jpeg_ref.tables(90)
    b = io.BytesIO()
    Image.fromarray(u8).save(b, "JPEG", qtables=[ql, qc], subsampling=2, optimize=False)
    mse = float(np.mean((dec.astype(np.float64) - u8) ** 2))
    mse_pil = float(np.mean((_decode(b.getvalue()).astype(np.float64) - u8) ** 2))
    print(f"[jpeg] 1920x1080 q 90: {len(data)} B = {len(data) / (1920 * 1080):.4f} B/pixel (libjpeg, same tables: {len(b.getvalue())} B); "
          f"MSE {mse:.4f} against libjpeg's {mse_pil:.4f} (ratio {mse / mse_pil:.4f})")
    assert mse <= 1.02 * mse_pil
    assert jpeg_encode_device(r, 90) == data
    r2 = _frame(1920, 1080)
    assert jpeg_encode_device(r2, 90) == data
    r2.close()
    r.close()


@pytest.mark.gpu
def test_sink_with_jpeg_codec_writes_the_same_files(tmp_path, hip_lib):
    from bhr_amd.output import FrameSink, jpeg_encode_device
    r = _frame(256, 144)
    cams = [([6, 0, 0.5], 90), ([5, 2, 1.0], 80), ([-7, 1, 0.3], 70), ([3.2, 0.5, 0.12], 100)] * 3
    direct = []
    with FrameSink(r, slots=3, workers=2, codec="jpeg", quality=90) as sink:
        for k, (c, f) in enumerate(cams):
            r.render_async(c, f)
            sink.submit(str(tmp_path / f"f{k:02d}.jpg"))
            if k < 4:
                direct.append(jpeg_encode_device(r, 90))
        frames, nbytes = sink.drain()
    assert frames == len(cams)
    total = 0
    for k in range(len(cams)):
        p = tmp_path / f"f{k:02d}.jpg"
        total += os.path.getsize(p)
        _same(p.read_bytes(), direct[k % 4])
    assert total == nbytes
    assert len(set(direct)) == 4                                          # four views, four different files
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    r.close()


@pytest.mark.gpu
def test_row_block_and_supersampled_contexts(hip_lib):
    """A tile context (rows 40..104 of 144) encodes its own rows as a 64-row image; a supersampled context its output frame."""
    from bhr_amd import HipRenderer
    from bhr_amd.output import jpeg_encode_device, jpeg_restart_interval
    r = HipRenderer(256, 144, scenes.analytic_skybox(), scenes.noisy_disk(), rows=(40, 104))
    r.render_async([6, 0, 0.5], 90)
    data = jpeg_encode_device(r, 90)
    u8 = r.read_final_u8()
    assert u8.shape == (64, 256, 3) and _decode(data).shape == (64, 256, 3)
    _same(data, jpeg_ref.encode(u8, 90, jpeg_restart_interval(256)))
    r.close()
    r = HipRenderer(256, 144, scenes.analytic_skybox(), scenes.noisy_disk(), supersample=2)
    r.render_async([6, 0, 0.5], 90)
    data = jpeg_encode_device(r, 90)
    u8 = r.read_final_u8()
    assert u8.shape == (144, 256, 3)
    _same(data, jpeg_ref.encode(u8, 90, jpeg_restart_interval(256)))
    r.close()


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(hip_lib):
    from bhr_amd.output import FrameSink, jpeg_encode_device, png_encode_device
    r = _frame(256, 144)
    png = png_encode_device(r)
    for q in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            jpeg_encode_device(r, q)
        with pytest.raises(ValueError, match="quality"):
            FrameSink(r, slots=2, workers=1, codec="jpeg", quality=q)
    assert png_encode_device(r) == png
    assert jpeg_encode_device(r, 90) == jpeg_encode_device(r, 90)
    r.close()
