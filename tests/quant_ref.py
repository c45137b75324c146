"""NumPy restatement of the two quantisers that read the f32 FINAL frame (csrc/quantize.hip; include/bhr.h:
bhr_read_final_u16, bhr_set_dither), and a PNG reader built on Python's zlib alone.  Not a test module.

Every arithmetic step is the device's, operation for operation, in float32:
    q16 = (uint16)(int)(clip(x, 0, 1) * 65535.0f)
    q8  = (uint8)floorf(clip(x, 0, 1) * 255.0f + t(c, X, Y)),   t = (M[(Y + oy_c) & 63][(X + ox_c) & 63] + 0.5f) / 4096.0f
with NaN -> 0 (the device's fminf(fmaxf(x, 0), 1)), the product and the sum rounded once each.

The reader exists because Pillow hands 16-bit RGB back as 8 bits: it splits the chunks, checks every CRC-32 and the
Adler-32 of the zlib stream itself, inflates, and undoes the five filters at a stride of 3 or 6 bytes.
"""
import struct
import zlib

import numpy as np

OFFSETS = ((0, 0), (21, 37), (43, 11))       # (ox, oy) for R, G, B
F32 = np.float32


def clip01(x):
    x = np.asarray(x, dtype=F32)
    x = np.where(np.isnan(x), F32(0), x)
    return np.minimum(np.maximum(x, F32(0)), F32(1)).astype(F32)


def quantize8(x):
    """The undithered u8 rows: save_image's truncation."""
    return (clip01(x) * F32(255.0)).astype(np.int32).astype(np.uint8)


def quantize16(x):
    return (clip01(x) * F32(65535.0)).astype(np.int32).astype(np.uint16)


def thresholds(matrix, height, width, row0=0):
    """(height, width, 3) float32 thresholds of rows row0 .. row0 + height - 1 of the full image."""
    m = np.asarray(matrix).reshape(64, 64).astype(F32)
    ys, xs = np.arange(row0, row0 + height)[:, None], np.arange(width)[None, :]
    t = np.empty((height, width, 3), dtype=F32)
    for c, (ox, oy) in enumerate(OFFSETS):
        t[..., c] = (m[(ys + oy) & 63, (xs + ox) & 63] + F32(0.5)) / F32(4096.0)
    return t


def quantize8_dither(x, matrix, row0=0):
    v = clip01(x) * F32(255.0)
    assert v.dtype == F32
    s = v + thresholds(matrix, v.shape[0], v.shape[1], row0)
    assert s.dtype == F32
    return np.floor(s).astype(np.int32).astype(np.uint8)


# ---- PNG reader -------------------------------------------------------------------------------------------------------
PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def png_chunks(data):
    """[(type, payload)] of a PNG file; every chunk's CRC-32 is checked, and that nothing follows IEND."""
    assert data[:8] == PNG_MAGIC, "not a PNG file"
    at, out = 8, []
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert len(body) == n, "truncated chunk"
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == (zlib.crc32(kind + body) & 0xFFFFFFFF), f"CRC of chunk {kind!r} at byte {at}"
        out.append((kind, body))
        at += 12 + n
        if kind == b"IEND":
            break
    assert at == len(data) and out and out[-1][0] == b"IEND", "bytes after IEND, or no IEND"
    return out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def _unfilter(raw, h, nbytes, bpp):
    rows = np.zeros((h, nbytes), dtype=np.uint8)
    prev = bytes(nbytes)
    filters = []
    for j in range(h):
        line = raw[j * (nbytes + 1):(j + 1) * (nbytes + 1)]
        f, cur = line[0], bytearray(line[1:])
        filters.append(f)
        assert 0 <= f <= 4, f"filter type {f} in row {j}"
        if f == 1:
            for i in range(bpp, nbytes):
                cur[i] = (cur[i] + cur[i - bpp]) & 255
        elif f == 2:
            cur = bytearray(((np.frombuffer(bytes(cur), np.uint8).astype(np.int32) + np.frombuffer(prev, np.uint8)) & 255)
                            .astype(np.uint8).tobytes())
        elif f == 3:
            for i in range(nbytes):
                cur[i] = (cur[i] + (((cur[i - bpp] if i >= bpp else 0) + prev[i]) >> 1)) & 255
        elif f == 4:
            for i in range(nbytes):
                a = cur[i - bpp] if i >= bpp else 0
                c = prev[i - bpp] if i >= bpp else 0
                cur[i] = (cur[i] + _paeth(a, prev[i], c)) & 255
        prev = bytes(cur)
        rows[j] = np.frombuffer(prev, np.uint8)
    return rows, filters


def png_read(data):
    """-> (samples, info): (H, W, 3) uint8 or, at bit depth 16, uint16 (from the file's big-endian bytes); info = {width,
    height, bit_depth, idat_chunks, filters}.  Colour type 2, no interlace; everything else is refused."""
    chunks = png_chunks(data)
    assert chunks[0][0] == b"IHDR" and len(chunks[0][1]) == 13
    w, h, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (colour, comp, filt, interlace) == (2, 0, 0, 0) and depth in (8, 16), (depth, colour, comp, filt, interlace)
    z = b"".join(body for kind, body in chunks if kind == b"IDAT")
    assert len(z) >= 6 and (z[0] & 15) == 8 and ((z[0] << 8) | z[1]) % 31 == 0 and not (z[1] & 0x20), "zlib header"
    d = zlib.decompressobj(-15)
    raw = d.decompress(z[2:]) + d.flush()
    assert d.eof and len(d.unused_data) == 4, "the deflate stream does not end in front of a 4-byte trailer"
    assert struct.unpack(">I", d.unused_data)[0] == (zlib.adler32(raw) & 0xFFFFFFFF), "Adler-32"
    bpp = 3 * depth // 8
    nbytes = bpp * w
    assert len(raw) == h * (nbytes + 1), f"{len(raw)} filtered bytes for {w}x{h} at {depth} bits"
    rows, filters = _unfilter(raw, h, nbytes, bpp)
    if depth == 16:
        samples = rows.reshape(h, w, 3, 2).astype(np.uint16)
        img = (samples[..., 0] << 8) | samples[..., 1]
    else:
        img = rows.reshape(h, w, 3)
    return img, {"width": w, "height": h, "bit_depth": depth, "filters": filters,
                 "idat_chunks": sum(1 for kind, _ in chunks if kind == b"IDAT")}
