"""16-bit output and blue-noise dither, the parts that need no GPU: the rank matrix, the restated quantisers
(tests/quant_ref.py), the host 16-bit PNG encoder, the command line and the progress record."""
import importlib.util
import os

import numpy as np
import pytest

import quant_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def matrix(hip_lib):
    from bhr_amd.output import dither_matrix
    m = dither_matrix()
    m.setflags(write=False)
    return m


def _generator():
    spec = importlib.util.spec_from_file_location("make_blue_noise", os.path.join(ROOT, "tools", "make_blue_noise.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_matrix_is_a_permutation(matrix):
    assert matrix.shape == (64, 64) and matrix.dtype == np.uint16
    assert sorted(matrix.ravel().tolist()) == list(range(4096))


def test_matrix_is_what_the_generator_makes(matrix):
    gen = _generator()
    m = gen.generate()
    np.testing.assert_array_equal(m, matrix)
    with open(gen.HEADER) as fh:
        assert fh.read() == gen.header_text(m)              # the committed header is the generator's output


def _band_means(m):
    """Periodogram of (M + 0.5) / 4096 - 0.5 over its variance, averaged over radial frequency bands (DC excluded)."""
    x = (m.astype(np.float64) + 0.5) / 4096.0 - 0.5
    p = np.abs(np.fft.fft2(x)) ** 2 / x.size / x.var()
    f = np.fft.fftfreq(64)
    fr = np.hypot(f[:, None], f[None, :])
    band = lambda lo, hi: float(p[(fr > 0) & (fr >= lo) & (fr < hi)].mean())
    return band(0, 1 / 8), [band(0, 1 / 16), band(1 / 16, 1 / 8), band(1 / 8, 1 / 4), band(1 / 4, 1 / 2)]


def test_matrix_is_blue(matrix):
    low, bands = _band_means(matrix)
    white, _ = _band_means(np.random.default_rng(5).permutation(4096).reshape(64, 64))
    print(f"[blue noise] mean normalised power over 0 < f < 1/8: {low:.2e} (random permutation: {white:.2f}); bands {bands}")
    assert low < 0.05                                        # the issue's acceptance condition
    assert white > 0.5                                       # the measure tells the two apart
    assert bands[0] < bands[1] < bands[2] < bands[3]         # power rises with frequency


FLAT = [0.0, 0.0031, 0.02, 0.5, 0.9999, 1.0, 0.003, 1.0 / 255.0, 0.25, 0.043]


@pytest.mark.parametrize("v", FLAT)
def test_flat_value_rounds_up_in_its_share_of_the_pixels(v, matrix):
    """A flat value v rounds up in exactly as many pixels of a 64 x 64 block as there are ranks r with
    frac(255 v) + (r + 0.5) / 4096 >= 1 (exact arithmetic: every term is a dyadic rational that binary64 holds) -- in every
    channel, whatever its offset, and wherever the block lies in the image."""
    v255 = np.float32(v) * np.float32(255.0)
    base = int(np.floor(v255))
    frac = float(v255) - base
    predicted = sum(1 for r in range(4096) if frac + (2 * r + 1) / 8192.0 >= 1.0)
    q = Q.quantize8_dither(np.full((64 + 9, 64 + 5, 3), v, np.float32), matrix, row0=13)
    assert set(np.unique(q).tolist()) <= {base, min(base + 1, 255)}
    for c in range(3):
        for (y0, x0) in ((0, 0), (9, 5)):
            assert int((q[y0:y0 + 64, x0:x0 + 64, c] > base).sum()) == predicted, (c, y0, x0)
    if frac == 0.0:
        assert predicted == 0                                # 0, 1 and every exact level stay as they are


def test_restated_quantisers_edge_values(matrix):
    from bhr_amd import output as O
    x = np.array([[[-1.0, 2.0, np.inf], [np.nan, -np.inf, 0.5], [1.0, 0.0, 0.99999994]]], np.float32)
    np.testing.assert_array_equal(Q.quantize16(x), [[[0, 65535, 65535], [0, 0, 32767], [65535, 0, 65534]]])
    d = Q.quantize8_dither(x, matrix)
    assert d[0, 0].tolist() == [0, 255, 255] and d[0, 1, :2].tolist() == [0, 0] and d[0, 2, :2].tolist() == [255, 0]
    # the package's own host quantisers (drivers.save_image) are the same functions
    rng = np.random.default_rng(3)
    y = (rng.random((70, 130, 3), dtype=np.float32) * 1.2 - 0.1).astype(np.float32)
    np.testing.assert_array_equal(O.quantize16(y), Q.quantize16(y))
    np.testing.assert_array_equal(O.quantize(y, dither="blue", row0=7), Q.quantize8_dither(y, matrix, row0=7))
    np.testing.assert_array_equal(O.quantize(y), (np.clip(y, 0, 1) * 255).astype(np.uint8))      # the default is untouched
    np.testing.assert_array_equal(O.quantize(y, dither="none"), Q.quantize8(y))
    # a row block dithers as the whole frame does
    np.testing.assert_array_equal(Q.quantize8_dither(y[16:40], matrix, row0=16), Q.quantize8_dither(y, matrix)[16:40])
    with pytest.raises(ValueError):
        O.quantize(y, dither="white")


def _images16(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    ramp = (np.arange(h * w * 3, dtype=np.int64) * 65535 // max(h * w * 3 - 1, 1)).astype(np.uint16).reshape(h, w, 3)
    return {"zeros": np.zeros((h, w, 3), np.uint16), "full": np.full((h, w, 3), 65535, np.uint16), "ramp": ramp,
            "noise": rng.integers(0, 65536, (h, w, 3)).astype(np.uint16)}


@pytest.mark.parametrize("w", [1, 2, 3, 8, 71, 300])
@pytest.mark.parametrize("h", [1, 3, 37])
def test_host_png16_round_trips(w, h, hip_lib):
    from bhr_amd.output import png_encode
    for name, img in _images16(w, h).items():
        for level in (0, 1, 6):
            for threads in (1, 4):
                data = png_encode(img, level=level, threads=threads)
                assert len(data) <= hip_lib.bhr_png_bound16(w, h)
                back, info = Q.png_read(data)
                assert (info["width"], info["height"], info["bit_depth"]) == (w, h, 16), (name, level, threads)
                assert back.dtype == np.uint16
                np.testing.assert_array_equal(back, img, err_msg=f"{name} level {level} threads {threads}")


def test_host_png16_file_and_8bit_reader(tmp_path, hip_lib):
    from bhr_amd.output import png_encode, png_write
    img = _images16(71, 37)["noise"]
    png_write(str(tmp_path / "a.png"), img, level=1)
    back, info = Q.png_read((tmp_path / "a.png").read_bytes())
    np.testing.assert_array_equal(back, img)
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    np.testing.assert_array_equal(Q.png_read(png_encode(img.byteswap().view(img.dtype.newbyteorder()), level=1))[0], img)
    # the reader on the 8-bit encoder, whose files Pillow reads too: same pixels from both
    import io
    from PIL import Image
    img8 = (img >> 8).astype(np.uint8)
    data = png_encode(img8, level=6, threads=4)
    back8, info8 = Q.png_read(data)
    assert info8["bit_depth"] == 8
    np.testing.assert_array_equal(back8, img8)
    np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), img8)
    with pytest.raises(AssertionError, match="CRC"):
        Q.png_read(data[:40] + bytes([data[40] ^ 1]) + data[41:])
    with pytest.raises(ValueError):
        png_encode(img.astype(np.uint32))


def test_cli_flags_and_refusals():
    from bhr_amd import cli
    a = cli.parse_args([])
    assert (a.bit_depth, a.dither) == (8, "none")
    cli.validate_args(a)
    a = cli.parse_args(["--bit_depth", "16"])
    assert a.bit_depth == 16
    cli.validate_args(a)
    a = cli.parse_args(["--dither", "blue", "--video", "--video_codec", "mjpeg"])
    assert a.dither == "blue"
    cli.validate_args(a)
    with pytest.raises(ValueError, match="dither"):
        cli.validate_args(cli.parse_args(["--bit_depth", "16", "--dither", "blue"]))
    with pytest.raises(ValueError, match="mjpeg"):
        cli.validate_args(cli.parse_args(["--bit_depth", "16", "--video", "--video_codec", "mjpeg"]))
    with pytest.raises(ValueError, match="PNG"):
        cli.validate_args(cli.parse_args(["--bit_depth", "16", "-o", "out.jpg"]))
    for bad in (["--bit_depth", "12"], ["--dither", "white"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    # a Namespace from before the flags existed still validates
    old = cli.parse_args([])
    del old.bit_depth, old.dither
    cli.validate_args(old)


def test_drivers_refuse_the_same_combinations(tmp_path):
    from bhr_amd import drivers
    img = np.zeros((4, 4, 3), np.float32)
    with pytest.raises(ValueError, match="dither"):
        drivers.save_image(img, str(tmp_path / "a.png"), bit_depth=16, dither="blue")
    with pytest.raises(ValueError, match="bit_depth"):
        drivers.save_image(img, str(tmp_path / "a.png"), bit_depth=12)
    with pytest.raises(ValueError, match="PNG"):
        drivers.save_image(img, str(tmp_path / "a.jpg"), bit_depth=16)
    with pytest.raises(ValueError, match="mjpeg"):
        drivers.render_video(None, 64, 36, 2, 24, str(tmp_path / "v.mp4"), 90, [6, 0, 0.5], bit_depth=16, video_codec="mjpeg")
    with pytest.raises(ValueError, match="dither"):
        drivers.render_image(64, 36, [6, 0, 0.5], 90, 0.1, bit_depth=16, dither="blue")
    assert not os.listdir(tmp_path)


def test_save_image_writes_both(tmp_path, matrix):
    from bhr_amd import drivers
    rng = np.random.default_rng(8)
    img = (rng.random((37, 71, 3), dtype=np.float32) * 0.06).astype(np.float32)
    drivers.save_image(img, str(tmp_path / "deep.png"), bit_depth=16)
    back, info = Q.png_read((tmp_path / "deep.png").read_bytes())
    assert info["bit_depth"] == 16
    np.testing.assert_array_equal(back, Q.quantize16(img))
    drivers.save_image(img, str(tmp_path / "blue.png"), dither="blue")
    back, info = Q.png_read((tmp_path / "blue.png").read_bytes())
    assert info["bit_depth"] == 8
    np.testing.assert_array_equal(back, Q.quantize8_dither(img, matrix))
    drivers.save_image(img, str(tmp_path / "plain.png"))
    np.testing.assert_array_equal(Q.png_read((tmp_path / "plain.png").read_bytes())[0], (np.clip(img, 0, 1) * 255).astype(np.uint8))


def test_progress_params_carry_only_what_is_not_default():
    from bhr_amd.drivers import progress_params
    base = {"n_frames": 6, "fov": 90, "orbit": True, "disk_rotation_speed": 0.1, "orbit_degrees": 60.0}
    assert progress_params(6, 90, True, 0.1, 60.0) == base                       # a record of the parent commit still matches
    assert progress_params(6, 90, True, 0.1, 60.0, bit_depth=8, dither="none") == base
    assert progress_params(6, 90, True, 0.1, 60.0, bit_depth=16) == dict(base, bit_depth=16)
    assert progress_params(6, 90, True, 0.1, 60.0, dither="blue") == dict(base, dither="blue")
    assert progress_params(6, 90, True, 0.1, 60.0, "mjpeg", 75, 8, "blue") == dict(base, video_codec="mjpeg", video_quality=75,
                                                                                  dither="blue")
    # different values never compare equal: such a resume starts over
    assert progress_params(6, 90, True, 0.1, 60.0, bit_depth=16) != base != progress_params(6, 90, True, 0.1, 60.0, dither="blue")
