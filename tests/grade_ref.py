"""NumPy restatement of the grading stage (csrc/grade.hip; include/bhr.h: bhr_set_grade), and decoders of the two HDR file
formats drivers.save_hdr writes.  Not a test module.

hdr_plane() is the device's f32 arithmetic, operation for operation, and is compared bit for bit.  grade() evaluates the
operators and the transfer function in binary64, with their constants as written, from f32 inputs -- the plane h, and the two
factors the host derives and rounds to f32 (gain, iw2) -- and is what FINAL is compared against within TOL.

TOL = 1e-6 absolute: an f32 NumPy evaluation of every operator x transfer x exposure in {-3.5, 0, 2.25} stays within 2.8e-7
of this binary64 one over 4 M inputs ([0, 4] densely, 1e-8 .. 1e5 logarithmically, 0, 1, 0.0031308, 65504); the device gets
about four times that for its powf and its divide.
"""
import numpy as np

F32 = np.float32
TOL = 1e-6
OPS = ("clip", "reinhard", "aces")
TRANSFERS = ("linear", "srgb")
HDR_MAX = F32(65504.0)


def combine(bg, disk, blur=None):
    """s = (bg + disk) + blur in f32, the combine's own order; blur None: the sum of a BHR_SKIP_BLOOM frame."""
    s = np.asarray(bg, F32) + np.asarray(disk, F32)
    if blur is not None:
        s = s + np.asarray(blur, F32)
    assert s.dtype == F32
    return s


def clamp_hdr(x):
    """fminf(fmaxf(x, 0), 65504) with NaN -> 0."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        x = np.where(np.isnan(x), F32(0), x)
        return np.minimum(np.maximum(x, F32(0)), HDR_MAX).astype(F32)


def hdr_plane(bg, disk, blur=None):
    """The HDR plane h of a frame without flare, bit for bit."""
    with np.errstate(invalid="ignore"):                      # inf - inf in the injected layers: NaN -> 0
        return clamp_hdr(combine(bg, disk, blur))


def gain_of(stops):
    return F32(np.exp2(np.float64(F32(stops))))


def iw2_of(white):
    w = np.float64(F32(white))
    return F32(1.0 / (w * w))


def tonemap(v, op, iw2=None):
    """binary64; v >= 0."""
    v = np.asarray(v, np.float64)
    if op == "clip":
        return np.minimum(v, 1.0)
    if op == "reinhard":
        return np.minimum((v * (1.0 + v * np.float64(iw2))) / (1.0 + v), 1.0)
    if op == "aces":
        return np.clip((v * (2.51 * v + 0.03)) / (v * (2.43 * v + 0.59) + 0.14), 0.0, 1.0)
    raise ValueError(op)


def transfer_fn(y, transfer):
    y = np.asarray(y, np.float64)
    if transfer == "linear":
        return y
    if transfer == "srgb":
        return np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.power(np.maximum(y, 1e-300), 1.0 / 2.4) - 0.055)
    raise ValueError(transfer)


def grade_hdr(h, op="clip", stops=0.0, white=2.5, transfer="linear"):
    """FINAL of the plane h (f32), in binary64."""
    h = np.asarray(h)
    assert h.dtype == F32
    v = h.astype(np.float64) * np.float64(gain_of(stops))
    return transfer_fn(tonemap(v, op, iw2_of(white)), transfer)


def grade(bg, disk, blur=None, **kw):
    return grade_hdr(hdr_plane(bg, disk, blur), **kw)


# ---- HDR files ----------------------------------------------------------------------------------------------------------
def pfm_read(data):
    """(H, W, 3) float32 of a colour PFM file's bytes (rows are stored bottom-up)."""
    parts = data.split(b"\n", 3)
    assert parts[0] == b"PF", "not a colour PFM"
    w, h = (int(v) for v in parts[1].split())
    scale = float(parts[2])
    body = parts[3]
    assert len(body) == w * h * 12, f"{len(body)} bytes for {w}x{h}"
    img = np.frombuffer(body, dtype="<f4" if scale < 0 else ">f4").reshape(h, w, 3)
    return np.ascontiguousarray(img[::-1]).astype(F32)


def rgbe_read(data):
    """(H, W, 3) float32 of a flat (not run-length coded) Radiance file's bytes: mantissa * 2^(e - 136), e = 0 -> 0."""
    head, _, rest = data.partition(b"\n\n")
    lines = head.split(b"\n")
    assert lines[0] == b"#?RADIANCE" and b"FORMAT=32-bit_rle_rgbe" in lines, lines
    res, _, body = rest.partition(b"\n")
    tok = res.split()
    assert tok[0] == b"-Y" and tok[2] == b"+X", res
    h, w = int(tok[1]), int(tok[3])
    assert len(body) == w * h * 4, f"{len(body)} bytes for {w}x{h}"
    px = np.frombuffer(body, np.uint8).reshape(h, w, 4)
    e = px[..., 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(1.0, e - 136), 0.0)
    return (px[..., :3].astype(np.float64) * scale[..., None]).astype(F32)
