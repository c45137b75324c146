"""The JPEG format of include/bhr_output.h as restated by tests/jpeg_ref.py: decodes with libjpeg (Pillow), is as good
as libjpeg's own encoder with the same tables, stays inside int32, and uses the tables the library exports.  No GPU."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "e2e_ref.npz"))
    return (np.clip(z["final"], 0, 1) * 255).astype(np.uint8)


def _frames():
    rng = np.random.default_rng(5)
    return {"golden": _golden(), "noise": rng.integers(0, 256, (48, 80, 3), dtype=np.uint8),
            "bilevel": (rng.integers(0, 2, (48, 80, 3)) * 255).astype(np.uint8)}


@pytest.mark.parametrize("size", [(320, 180), (317, 179), (33, 17), (1, 1), (5, 2)])
def test_restatement_decodes_and_restart_intervals_do_not_change_pixels(size):
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    # smooth content with noise on top, so that both short and long coefficient runs occur
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), (x + y) % 256], axis=-1) + rng.integers(-20, 21, (h, w, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    plain = jpeg_ref.encode(img, 90, 0)
    want = _decode(plain)
    assert want.shape == (h, w, 3)
    from PIL import Image
    b = io.BytesIO()                                                         # the picture, not something else of that size
    Image.fromarray(img).save(b, "JPEG", qtables=list(jpeg_ref.tables(90)), subsampling=2, optimize=False)
    assert np.abs(want.astype(int) - img).mean() <= 1.25 * np.abs(_decode(b.getvalue()).astype(int) - img).mean() + 1
    for r in (1, 3, 7, jpeg_ref.restart_interval(w)):
        data = jpeg_ref.encode(img, 90, r)
        np.testing.assert_array_equal(_decode(data), want, err_msg=f"restart {r}")
        assert len(data) >= len(plain) + 6                                  # DRI, and the markers if there are any


@pytest.mark.parametrize("quality", [50, 75, 90, 100])
@pytest.mark.parametrize("name", ["golden", "noise", "bilevel"])
def test_quality_and_size_against_libjpeg(name, quality):
    """The bar is libjpeg itself: same tables, both files decoded by libjpeg.  MSE at most 1.02 x, size at most 1.06 x."""
    from PIL import Image
    img = _frames()[name]
    ql, qc = jpeg_ref.tables(quality)
    ours = jpeg_ref.encode(img, quality, 0)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", qtables=[ql, qc], subsampling=2, optimize=False)
    ref = b.getvalue()
    mse = np.mean((_decode(ours).astype(np.float64) - img) ** 2)
    mse_ref = np.mean((_decode(ref).astype(np.float64) - img) ** 2)
    print(f"[jpeg_ref] {name} q {quality}: MSE {mse:.4f} / libjpeg {mse_ref:.4f} = {mse / mse_ref:.4f}; "
          f"{len(ours)} B / {len(ref)} B = {len(ours) / len(ref):.4f}")
    assert mse <= 1.02 * mse_ref
    assert len(ours) <= 1.06 * len(ref)


def test_restart_overhead_is_small():
    """R = restart_interval(w) against R = 0 on the golden frame: a few bytes per interval."""
    img = _golden()
    r = jpeg_ref.restart_interval(img.shape[1])
    a, b = len(jpeg_ref.encode(img, 90, 0)), len(jpeg_ref.encode(img, 90, r))
    intervals = -(-(20 * 12) // r)
    print(f"[jpeg_ref] golden frame q 90: {a} B without restarts, {b} B with R = {r} ({(b - a) / intervals:.2f} B per interval)")
    assert 0 < b - a <= 6 + 8 * intervals


def _extreme_blocks():
    rng = np.random.default_rng(1)
    x = rng.integers(-128, 128, (20000 + 8, 8, 8))
    par = np.add.outer(np.arange(8), np.arange(8)) & 1
    x[0], x[1] = -128, 127
    x[2] = np.where(par == 0, -128, 127)
    x[3] = np.where(par == 0, 127, -128)
    # the sign patterns of the basis functions with the largest absolute sums: (0,4), (4,0), (4,4), and the one of (1,1)
    for k, (v, u) in enumerate([(0, 4), (4, 0), (4, 4), (1, 1)]):
        basis = np.outer(jpeg_ref.M[v], jpeg_ref.M[u])
        x[4 + k] = np.where(basis > 0, 127, -128)
    return x


def test_dct_stays_inside_int32_and_close_to_binary64():
    x = _extreme_blocks()
    f8 = jpeg_ref.fdct8(x, check=True)                                      # asserts the int32 bounds
    exact = np.einsum("vy,nyx,ux->nvu", jpeg_ref.M, x.astype(np.float64), jpeg_ref.M)
    err = np.abs(f8 / 8.0 - exact).max()
    print(f"[jpeg_ref] DCT: max |f8 / 8 - binary64| = {err:.6f}, max |f8| = {np.abs(f8).max()}")
    assert err <= 0.5
    # worst partial sums for ANY 8-bit block, not only these: |sum| <= sum |MI| * max |operand|
    row_worst = int(np.abs(jpeg_ref.MI).sum(axis=1).max()) * 128 + 1024
    t_worst = row_worst >> 11
    assert t_worst < 2 ** 15 and int(np.abs(jpeg_ref.MI).sum(axis=1).max()) * t_worst + 2048 < 2 ** 31
    # AC coefficients fit the 10 bits the Huffman tables provide, DC differences 11, at the finest quantiser (Q = 1)
    q = jpeg_ref.quant(f8, np.ones(64, np.int64))
    ac = q.reshape(-1, 64)[:, 1:]
    assert np.abs(ac).max() <= 1023 and np.abs(q[:, 0, 0]).max() <= 1024


def _lib_tables(hip_lib, quality):
    q, counts, vals = np.zeros((2, 64), np.uint8), np.zeros((4, 16), np.uint8), np.zeros((4, 162), np.uint8)
    p8 = C.POINTER(C.c_uint8)
    rc = hip_lib.bhr_jpeg_tables(quality, q.ctypes.data_as(p8), counts.ctypes.data_as(p8), vals.ctypes.data_as(p8))
    return rc, q, counts, vals


@pytest.mark.parametrize("quality", [1, 25, 50, 75, 90, 100])
def test_library_tables_are_the_restatements(quality, hip_lib):
    from bhr_amd.output import jpeg_tables
    rc, q, counts, vals = _lib_tables(hip_lib, quality)
    assert rc == 0
    ql, qc = jpeg_ref.tables(quality)
    assert q[0].tolist() == ql and q[1].tolist() == qc
    for k, (_, bits, huffval) in enumerate(jpeg_ref.HUFF):
        assert counts[k].tolist() == bits
        assert vals[k, :len(huffval)].tolist() == huffval and not vals[k, len(huffval):].any()
    assert jpeg_tables(quality) == ((ql, qc), [(bits, huffval) for _, bits, huffval in jpeg_ref.HUFF])


def test_tables_are_libjpegs(hip_lib):
    """The Huffman tables and the quality-50 quantisation tables are those in the DHT / DQT of a file Pillow writes."""
    dht, dqt = jpeg_ref.pillow_tables()
    rc, q, counts, vals = _lib_tables(hip_lib, 50)
    assert rc == 0
    assert q[0].tolist() == dqt[0] and q[1].tolist() == dqt[1]
    for k, (ident, bits, huffval) in enumerate(jpeg_ref.HUFF):
        assert dht[ident] == (bits, huffval)
        assert (counts[k].tolist(), vals[k, :sum(bits)].tolist()) == dht[ident]
    for quality in (1, 25, 75, 90, 100):                                    # libjpeg's scaling of them
        import io as _io
        from PIL import Image
        b = _io.BytesIO()
        Image.fromarray(np.zeros((16, 16, 3), "u1")).save(b, "JPEG", quality=quality, subsampling=2, optimize=False)
        got = {}
        for m, p in jpeg_ref.segments(b.getvalue()):
            at = 0
            while m == 0xDB and at < len(p):
                got[p[at] & 15] = list(p[at + 1:at + 65])
                at += 65
        assert (got[0], got[1]) == jpeg_ref.tables(quality)


def test_restart_interval_bound_and_refusals(hip_lib):
    from bhr_amd import _lib
    for w in (1, 2, 15, 16, 17, 320, 1920, 3840, 7680):
        r = hip_lib.bhr_jpeg_restart_interval(w)
        assert r == jpeg_ref.restart_interval(w) and 0 < r <= 65535
    assert all(hip_lib.bhr_jpeg_restart_interval(w) > 0 for w in range(1, 7681))
    for w, h in [(1, 1), (17, 33), (320, 180), (1920, 1080), (7680, 4320)]:
        mcus = -(-w // 16) * -(-h // 16)
        intervals = -(-mcus // hip_lib.bhr_jpeg_restart_interval(w))
        block_bits = 20 + 63 * 26
        mcu_bytes = -(-6 * block_bits // 8)
        assert mcu_bytes == 1244
        worst = 2 * mcus * mcu_bytes + 3 * intervals + len(jpeg_ref.header(w, h, 100, 10))
        assert hip_lib.bhr_jpeg_device_bound(w, h) >= worst
    for quality in (0, 101, -5):
        rc, *_ = _lib_tables(hip_lib, quality)
        assert rc == _lib.BHR_ERR_INVALID and b"quality" in hip_lib.bhr_last_error()
        with pytest.raises(ValueError):
            jpeg_ref.tables(quality)


def test_incompressible_frames_stay_inside_the_bound(hip_lib):
    """Noise and 0/255 frames at quality 100 (restatement; the device's files are the same bytes)."""
    rng = np.random.default_rng(3)
    w, h = 80, 48
    for img in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)):
        data = jpeg_ref.encode(img, 100, jpeg_ref.restart_interval(w))
        assert len(data) <= hip_lib.bhr_jpeg_device_bound(w, h)
