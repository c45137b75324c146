"""NumPy restatement of the device JPEG encoder (csrc/jpeg_device.hip; format in include/bhr_output.h).

Baseline sequential JFIF, 4:2:0, the four standard Huffman tables of ITU T.81 Annex K, integer colour conversion,
an int32 fixed-point DCT, restart intervals.  ``encode`` must reproduce the device's files byte for byte; every
arithmetic step below is repeated operation for operation by the kernel.  Not a test module.
"""
import struct

import numpy as np

# zig-zag position k -> natural index 8 v + u
ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
               28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
               47, 55, 62, 63])

# ITU T.81 Annex K.1: luminance and chrominance quantisation tables (quality 50), in zig-zag order as a DQT segment holds them
BASE_Q = (
    [16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60,
     57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112,
     100, 120, 92, 101, 103, 99],
    [17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66] + [99] * 50,
)

_AC_TAIL = [r * 16 + s for r in range(16) for s in range(1, 11)]          # every (run, size) symbol, in value order


def _ac_tail(skip):
    return [v for v in _AC_TAIL if v not in skip]


# ITU T.81 Annex K.3: (Tc << 4 | Th, BITS[16], HUFFVAL) in the order of the DHT segment: DC lum, AC lum, DC chroma, AC chroma
_AC_LUM_HEAD = [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21,
                82, 209, 240, 36, 51, 98, 114, 130]
_AC_CHR_HEAD = [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35,
                51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241]
HUFF = (
    (0x00, [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    (0x10, [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], _AC_LUM_HEAD + _ac_tail(set(_AC_LUM_HEAD))),
    (0x01, [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    (0x11, [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], _AC_CHR_HEAD + _ac_tail(set(_AC_CHR_HEAD))),
)

RESTART_INTERVAL = 10       # MCUs; bhr_jpeg_restart_interval(w) for every width (see include/bhr_output.h)


def restart_interval(width):
    return RESTART_INTERVAL


def scale_q(base, quality):
    """libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (force_baseline)."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * s + 50) // 100, 1), 255) for b in base]


def tables(quality):
    """-> (luma, chroma) quantisation tables in zig-zag order."""
    if not 1 <= quality <= 100:
        raise ValueError(f"quality {quality} outside 1..100")
    return scale_q(BASE_Q[0], quality), scale_q(BASE_Q[1], quality)


def codes(counts, vals):
    """symbol -> (code, length) of the canonical code (T.81 Annex C)."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


# the DCT matrix in 1.13 fixed point: MI[u][x] = round(8192 c(u) / 2 cos((2x + 1) u pi / 16)), c(0) = sqrt(1/2), c(u) = 1
M = np.array([[(0.5 * (np.sqrt(0.5) if u == 0 else 1.0)) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])
MI = np.round(M * 8192).astype(np.int64)


def fdct8(blocks, check=True):
    """(n, 8, 8) level-shifted samples [y][x] -> (n, 8, 8) [v][u] = EIGHT times the DCT coefficient.  Every intermediate
    fits int32 (asserted): rows t = (MI . p + 1024) >> 11 (four times the 1-D transform), columns (MI . t + 2048) >> 12."""
    blocks = np.asarray(blocks, np.int64)
    acc = np.einsum("ux,nyx->nyu", MI, blocks)
    t = (acc + (1 << 10)) >> 11
    acc2 = np.einsum("vy,nyu->nvu", MI, t)
    f8 = (acc2 + (1 << 11)) >> 12
    if check:
        # the partial sums of a dot product are bounded by the sum of absolute products
        worst1 = np.abs(MI).sum(axis=1).max() * 128 + (1 << 10)
        worst2 = np.abs(MI).sum(axis=1).max() * int(np.abs(t).max(initial=0)) + (1 << 11)
        assert worst1 < 2 ** 31 and worst2 < 2 ** 31 and np.abs(t).max(initial=0) < 2 ** 15
    return f8


def quant(f8, q_nat):
    """q = sign(f8) ((|f8| + 4 Q) // (8 Q)): round to nearest, halves away from zero.  q_nat: (64,) natural order."""
    q8 = 8 * np.asarray(q_nat, np.int64).reshape(8, 8)
    return np.sign(f8) * ((np.abs(f8) + q8 // 2) // q8)


def ycc(rgb):
    """(h, w, 3) u8 -> Y (H, W), Cb, Cr (H/2, W/2), the frame padded to multiples of 16 by repeating its last column / row."""
    h, w, _ = rgb.shape
    H, W = -(-h // 16) * 16, -(-w // 16) * 16
    p = np.pad(rgb.astype(np.int64), ((0, H - h), (0, W - w), (0, 0)), mode="edge")
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    c = (p.reshape(H // 2, 2, W // 2, 2, 3).sum(axis=(1, 3)) + 2) >> 2
    R, G, B = c[..., 0], c[..., 1], c[..., 2]
    Cb = np.clip((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16, 0, 255)
    Cr = np.clip((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16, 0, 255)
    return Y, Cb, Cr


def _blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128


def coefficients(rgb, quality):
    """Quantised coefficients in zig-zag order: Y (H/8, W/8, 64), Cb, Cr (H/16, W/16, 64)."""
    ql, qc = tables(quality)
    nat = np.argsort(ZZ)
    out = []
    for plane, q in zip(ycc(rgb), (ql, qc, qc)):
        b = _blocks(plane)
        z = quant(fdct8(b.reshape(-1, 8, 8)), np.array(q)[nat]).reshape(-1, 64)[:, ZZ]
        out.append(z.reshape(b.shape[0], b.shape[1], 64))
    return out


def header(w, h, quality, restart):
    ql, qc = tables(quality)
    out = bytearray(b"\xFF\xD8")
    out += b"\xFF\xE0" + struct.pack(">H5sHBHHBB", 16, b"JFIF\0", 0x0101, 0, 1, 1, 0, 0)
    out += b"\xFF\xDB" + struct.pack(">H", 2 + 65 * 2) + bytes([0]) + bytes(ql) + bytes([1]) + bytes(qc)
    out += b"\xFF\xC0" + struct.pack(">HBHHB", 17, 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    body = b"".join(bytes([k]) + bytes(counts) + bytes(vals) for k, counts, vals in HUFF)
    out += b"\xFF\xC4" + struct.pack(">H", 2 + len(body)) + body
    if restart:
        out += b"\xFF\xDD" + struct.pack(">HH", 4, restart)
    out += b"\xFF\xDA" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return bytes(out)


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, code, ln):
        self.acc = (self.acc << ln) | code
        self.n += ln
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _code_block(bw, z, pred, dc, ac):
    """z: 64 Python ints in zig-zag order."""
    d = z[0] - pred
    s = abs(d).bit_length()
    bw.put(*dc[s])
    if s:
        bw.put(d if d > 0 else d + (1 << s) - 1, s)
    last = 63
    while last > 0 and z[last] == 0:
        last -= 1
    run = 0
    for k in range(1, last + 1):
        v = z[k]
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        s = abs(v).bit_length()
        bw.put(*ac[(run << 4) | s])
        bw.put(v if v > 0 else v + (1 << s) - 1, s)
        run = 0
    if last < 63:
        bw.put(*ac[0])
    return z[0]


def encode(rgb_u8, quality=90, restart=0):
    """(h, w, 3) uint8 -> the bytes of the JFIF file.  restart: MCUs per restart interval, 0 = none."""
    rgb = np.ascontiguousarray(rgb_u8)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    h, w, _ = rgb.shape
    by, bb, br = (a.tolist() for a in coefficients(rgb, quality))
    dcl, acl, dcc, acc = (codes(counts, vals) for _, counts, vals in HUFF)
    bw = _Bits()
    pred = [0, 0, 0]
    n = rst = 0
    for my in range(len(bb)):
        for mx in range(len(bb[0])):
            if restart and n and n % restart == 0:
                bw.flush()
                bw.out += bytes([0xFF, 0xD0 + rst])
                rst = (rst + 1) & 7
                pred = [0, 0, 0]
            for dy in (0, 1):
                for dx in (0, 1):
                    pred[0] = _code_block(bw, by[2 * my + dy][2 * mx + dx], pred[0], dcl, acl)
            pred[1] = _code_block(bw, bb[my][mx], pred[1], dcc, acc)
            pred[2] = _code_block(bw, br[my][mx], pred[2], dcc, acc)
            n += 1
    bw.flush()
    return header(w, h, quality, restart) + bytes(bw.out) + b"\xFF\xD9"


def segments(buf):
    """(marker, payload) of every segment before SOS."""
    at = 2
    while at < len(buf):
        assert buf[at] == 0xFF
        m = buf[at + 1]
        if m == 0xDA:
            return
        n = struct.unpack_from(">H", buf, at + 2)[0]
        yield m, buf[at + 4:at + 2 + n]
        at += 2 + n


def pillow_tables():
    """The DHT and DQT of a file Pillow (libjpeg) writes at quality 50: {Tc<<4|Th: (counts, values)}, {Tq: 64 zig-zag}."""
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), "u1")).save(b, "JPEG", quality=50, subsampling=2, optimize=False)
    dht, dqt = {}, {}
    for m, p in segments(b.getvalue()):
        at = 0
        while m == 0xC4 and at < len(p):
            counts = list(p[at + 1:at + 17])
            n = sum(counts)
            dht[p[at]] = (counts, list(p[at + 17:at + 17 + n]))
            at += 17 + n
        while m == 0xDB and at < len(p):
            dqt[p[at] & 15] = list(p[at + 1:at + 65])
            at += 65
    return dht, dqt
