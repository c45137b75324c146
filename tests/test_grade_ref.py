"""The grade's NumPy restatement (tests/grade_ref.py) at its fixed points, and the two HDR file formats of drivers.save_hdr
through the restatement's decoders.  CPU only."""
import numpy as np
import pytest

import grade_ref as G

F32 = np.float32


def test_clip_at_zero_stops_linear_is_np_clip():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-1, 3, 4096), [0.0, 1.0, 2.5, 65504.0, 1e5]]).astype(F32)
    got = G.grade_hdr(G.clamp_hdr(x), "clip", 0.0, 2.5, "linear")
    np.testing.assert_array_equal(got, np.clip(x, 0, 1).astype(np.float64))
    zeros = np.zeros(8, F32)
    np.testing.assert_array_equal(G.grade(x[:8], zeros, zeros), np.clip(x[:8], 0, 1).astype(np.float64))


def test_hdr_plane_is_f32_in_the_combines_order():
    bg, disk, blur = F32(0.1), F32(0.2), F32(1e-9)
    h = G.hdr_plane(np.array([bg]), np.array([disk]), np.array([blur]))
    assert h.dtype == F32 and h[0] == (bg + disk) + blur
    odd = np.array([np.nan, np.inf, -np.inf, -1.0, 7e4], F32)
    zeros = np.zeros(5, F32)
    np.testing.assert_array_equal(G.hdr_plane(odd, zeros, zeros), np.array([0, 65504, 0, 0, 65504], F32))
    np.testing.assert_array_equal(G.hdr_plane(np.array([np.inf], F32), zeros[:1], np.array([-np.inf], F32)), [0])   # inf - inf
    np.testing.assert_array_equal(G.hdr_plane(odd, zeros), G.hdr_plane(odd, zeros, zeros))


@pytest.mark.parametrize("white", [0.5, 1.0, 2.5, 100.0])
def test_reinhard_maps_white_to_one(white):
    h = np.array([white], F32)
    assert abs(G.grade_hdr(h, "reinhard", 0.0, white)[0] - 1.0) < 1e-7       # iw2 is rounded to f32
    assert G.grade_hdr(h * F32(0.999), "reinhard", 0.0, white)[0] < 1.0
    assert G.grade_hdr(h * F32(4), "reinhard", 0.0, white)[0] == 1.0
    assert abs(G.grade_hdr(h * F32(0.25), "reinhard", 2.0, white)[0] - 1.0) < 1e-7   # two stops up


def test_aces_and_srgb_values():
    # the formula at 1 is 2.54 / 3.16 = 0.803797...; the figure quoted for it, 0.80383, holds to its four leading digits
    assert abs(G.tonemap(1.0, "aces") - 2.54 / 3.16) < 1e-15 and abs(G.tonemap(1.0, "aces") - 0.80383) < 5e-5
    assert G.tonemap(0.0, "aces") == 0.0 and G.tonemap(1e5, "aces") == 1.0
    assert abs(G.transfer_fn(0.5, "srgb") - 0.735357) < 5e-7
    assert G.transfer_fn(0.0, "srgb") == 0.0 and abs(G.transfer_fn(1.0, "srgb") - 1.0) < 1e-12
    lo, hi = G.transfer_fn(0.0031308, "srgb"), G.transfer_fn(np.nextafter(0.0031308, 1.0), "srgb")
    assert abs(hi - lo) < 1e-7                                     # the two branches meet
    assert G.gain_of(-3.5) == F32(2.0 ** -3.5) and G.gain_of(2.0) == 4.0 and G.iw2_of(2.5) == F32(0.16)


@pytest.mark.parametrize("op", G.OPS)
@pytest.mark.parametrize("transfer", G.TRANSFERS)
@pytest.mark.parametrize("stops", [-3.5, 0.0, 2.25])
def test_operators_are_monotone(op, transfer, stops):
    h = np.linspace(0.0, 8.0, 100_000).astype(F32)
    y = G.grade_hdr(h, op, stops, 2.5, transfer)
    assert y[0] == 0.0 and (y >= 0).all() and (y <= 1).all()
    assert (np.diff(y) >= 0).all()
    assert y[-1] > y[0]


def test_pfm_round_trip_is_exact(tmp_path):
    from bhr_amd.drivers import save_hdr
    rng = np.random.default_rng(2)
    img = rng.uniform(0, 3, (7, 5, 3)).astype(F32)
    img[0, 0] = [0.0, 65504.0, 1e-30]
    path = str(tmp_path / "a.pfm")
    save_hdr(img, path)
    data = open(path, "rb").read()
    assert data.startswith(b"PF\n5 7\n-1.0\n")
    back = G.pfm_read(data)
    assert back.dtype == F32
    np.testing.assert_array_equal(back.view(np.uint32), img.view(np.uint32))
    assert data[-12:] == img[0, -1].astype("<f4").tobytes()        # bottom-up: the file ends with the top row


def test_rgbe_round_trip(tmp_path):
    from bhr_amd.drivers import rgbe_encode, save_hdr
    rng = np.random.default_rng(3)
    img = (rng.uniform(0, 1, (9, 6, 3)) * 10.0 ** rng.uniform(-6, 4.5, (9, 6, 1))).astype(F32)
    img[0, 0] = 0.0
    img[0, 1] = [65504.0, 1.0, 0.0]
    img[0, 2] = [1.0, 1.0, 1.0]
    img[0, 3] = [0.0, 0.0, 2.5]
    path = str(tmp_path / "a.hdr")
    save_hdr(img, path)
    data = open(path, "rb").read()
    assert data.startswith(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 9 +X 6\n")
    assert len(data) == len(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 9 +X 6\n") + 9 * 6 * 4      # flat
    back = G.rgbe_read(data)
    bound = img.max(axis=-1, keepdims=True).astype(np.float64) / 128
    err = np.abs(back.astype(np.float64) - img)
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    assert (back <= img).all()                                     # truncated mantissas never exceed the value
    assert (back[0, 0] == 0).all() and back[0, 1, 2] == 0 and back[0, 3, 0] == 0 and back[0, 3, 2] == 2.5
    px = rgbe_encode(img)
    assert tuple(px[0, 2]) == (128, 128, 128, 129) and tuple(px[0, 0]) == (0, 0, 0, 0)
    m, e = np.frexp(img.max(axis=-1))
    np.testing.assert_array_equal(px[..., 3][img.max(axis=-1) > 0], (e + 128)[img.max(axis=-1) > 0])
    with pytest.raises(ValueError):
        save_hdr(img, str(tmp_path / "a.exr"))
    with pytest.raises(ValueError):
        save_hdr(img[..., 0], str(tmp_path / "b.pfm"))
