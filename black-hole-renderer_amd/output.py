"""Frame output: PNG files and the pipelined frame sink (include/bhr_output.h).

Counterpart of save_image (render.py:420-425) and of the PIL thread pool in render_video
(render.py:4412-4413, 4458-4467).  Decoded pixels are the reference's
``(np.clip(frame, 0, 1) * 255).astype(np.uint8)``; the compressed bytes are this encoder's own.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

DEFAULT_LEVEL = 6          # PIL's default zlib level for PNG
VIDEO_LEVEL = 1            # frames that are re-encoded into an MP4 anyway
DEVICE = -1                # BHR_PNG_DEVICE: filter + Huffman-code the frame on the GPU (csrc/png_device.hip)
JPEG_QUALITY = 90          # default quality of the device JPEG encoder (csrc/jpeg_device.hip)


def _u8(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"expected an (H, W, 3) uint8 image, got {a.dtype} {a.shape}")
    return a


def _u8_or_u16(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u" and a.dtype.itemsize == 2 and a.ndim == 3 and a.shape[2] == 3:
        return a.astype("=u2", copy=False)          # native endian: what the library reads
    return _u8(a)


def png_encode(rgb_u8: np.ndarray, level: int = DEFAULT_LEVEL, threads: int = 1) -> bytes:
    """(H, W, 3) uint8 -> PNG file bytes; an (H, W, 3) uint16 array -> a 16-bit PNG (bhr_png_encode16)."""
    a = _u8_or_u16(rgb_u8)
    h, w = a.shape[:2]
    lib = _lib.load()
    if a.dtype == np.uint16:
        cap = lib.bhr_png_bound16(w, h)
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_int64(0)
        _lib.check(lib.bhr_png_encode16(a.ctypes.data_as(C.POINTER(C.c_uint16)), w, h, level, threads,
                                        out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(n)))
        return out[:n.value].tobytes()
    cap = lib.bhr_png_bound(w, h)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_int64(0)
    p8 = C.POINTER(C.c_uint8)
    _lib.check(lib.bhr_png_encode(a.ctypes.data_as(p8), w, h, level, threads, out.ctypes.data_as(p8), cap, C.byref(n)))
    return out[:n.value].tobytes()


def png_write(path: str, rgb_u8: np.ndarray, level: int = DEFAULT_LEVEL, threads: int = 0) -> None:
    """Image.fromarray(rgb_u8).save(path) with row bands deflated on ``threads`` threads
    (0: one per 256 rows, at most the CPUs of this process).  A uint16 array is written as a 16-bit PNG."""
    a = _u8_or_u16(rgb_u8)
    h, w = a.shape[:2]
    if threads <= 0:
        threads = max(1, min(len(os.sched_getaffinity(0)), h // 256))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if a.dtype == np.uint16:
        _lib.check(_lib.load().bhr_png_write16(os.fsencode(path), a.ctypes.data_as(C.POINTER(C.c_uint16)), w, h, level, threads))
        return
    _lib.check(_lib.load().bhr_png_write(os.fsencode(path), a.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, level, threads))


def png_encode_device(renderer, bit_depth: int = 8) -> bytes:
    """PNG file bytes of the renderer's FINAL layer, filtered and entropy coded on the device (bhr_png_encode_device;
    ``bit_depth=16``: bhr_png16_encode_device, the samples of ``renderer.read_final_u16()``)."""
    if bit_depth not in (8, 16):
        raise ValueError(f"bit_depth must be 8 or 16, got {bit_depth!r}")
    lib = _lib.load()
    if bit_depth == 16 and renderer.width > lib.bhr_png16_device_max_width():
        raise ValueError(f"the 16-bit device PNG encoder takes frames up to {lib.bhr_png16_device_max_width()} pixels wide, "
                         f"this one has {renderer.width}; use the host encoder")
    bound, encode = ((lib.bhr_png16_device_bound, lib.bhr_png16_encode_device) if bit_depth == 16
                     else (lib.bhr_png_device_bound, lib.bhr_png_encode_device))
    cap = bound(renderer.width, renderer.rows)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_int64(0)
    _lib.check(encode(renderer._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(n)))
    return out[:n.value].tobytes()


def png_device_menu():
    """The encoder's code menu: list of (codes[257] uint32 = reversed code << 4 | length, header words, header bits)."""
    lib = _lib.load()
    n = C.c_int32(0)
    U32P = C.POINTER(C.c_uint32)
    out, k = [], 0
    while True:
        codes, hdr, bits = np.zeros(257, np.uint32), np.zeros(64, np.uint32), C.c_uint32(0)
        _lib.check(lib.bhr_png_device_menu(k, codes.ctypes.data_as(U32P), hdr.ctypes.data_as(U32P), C.byref(bits), C.byref(n)))
        out.append((codes, hdr, int(bits.value)))
        k += 1
        if k >= n.value:
            return out


def jpeg_encode_device(renderer, quality: int = JPEG_QUALITY) -> bytes:
    """JFIF file bytes (baseline, 4:2:0, standard Huffman tables) of the renderer's FINAL layer, colour-converted,
    transformed and entropy coded on the device (bhr_jpeg_encode_device; the format is fixed in include/bhr_output.h)."""
    lib = _lib.load()
    cap = lib.bhr_jpeg_device_bound(renderer.width, renderer.rows)
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_int64(0)
    _lib.check(lib.bhr_jpeg_encode_device(renderer._ctx, int(quality), out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(n)))
    return out[:n.value].tobytes()


def jpeg_tables(quality: int = JPEG_QUALITY):
    """The encoder's tables (host only): (luma, chroma) quantisation tables of ``quality``, 64 entries each in zig-zag
    order, and the four Huffman tables in DHT order (DC luma, AC luma, DC chroma, AC chroma) as (BITS[16], HUFFVAL)."""
    lib = _lib.load()
    q, counts, vals = np.zeros((2, 64), np.uint8), np.zeros((4, 16), np.uint8), np.zeros((4, 162), np.uint8)
    p8 = C.POINTER(C.c_uint8)
    _lib.check(lib.bhr_jpeg_tables(int(quality), q.ctypes.data_as(p8), counts.ctypes.data_as(p8), vals.ctypes.data_as(p8)))
    huff = [(counts[k].tolist(), vals[k, :int(counts[k].sum())].tolist()) for k in range(4)]
    return (q[0].tolist(), q[1].tolist()), huff


def jpeg_restart_interval(width: int) -> int:
    """MCUs per restart interval of a frame that wide (part of the file format; bhr_jpeg_restart_interval)."""
    return int(_lib.load().bhr_jpeg_restart_interval(int(width)))


DITHERS = ("none", "blue")
_DITHER_OFFSETS = ((0, 0), (21, 37), (43, 11))          # (ox, oy) of the R, G and B channels


def dither_matrix() -> np.ndarray:
    """The (64, 64) uint16 blue-noise rank matrix of the dithered quantiser (bhr_dither_matrix; host only)."""
    m = np.empty(4096, dtype=np.uint16)
    _lib.check(_lib.load().bhr_dither_matrix(m.ctypes.data_as(C.POINTER(C.c_uint16))))
    return m.reshape(64, 64)


def _clip01(image: np.ndarray) -> np.ndarray:
    """clip(x, 0, 1) in f32 with NaN -> 0, as the device's fminf(fmaxf(x, 0), 1)."""
    x = np.asarray(image, dtype=np.float32)
    return np.minimum(np.maximum(np.where(np.isnan(x), np.float32(0), x), np.float32(0)), np.float32(1))


def dither_thresholds(height: int, width: int, row0: int = 0) -> np.ndarray:
    """t(c, X, Y) = (M[(Y + oy_c) & 63][(X + ox_c) & 63] + 0.5) / 4096 for rows row0 .. row0 + height - 1 of the full image:
    (height, width, 3) float32 (exact: 13 significant bits)."""
    m = dither_matrix().astype(np.float32)
    ys, xs = np.arange(row0, row0 + height)[:, None], np.arange(width)[None, :]
    t = np.empty((height, width, 3), dtype=np.float32)
    for c, (ox, oy) in enumerate(_DITHER_OFFSETS):
        t[..., c] = (m[(ys + oy) & 63, (xs + ox) & 63] + np.float32(0.5)) / np.float32(4096.0)
    return t


def quantize(image: np.ndarray, dither: str = "none", row0: int = 0) -> np.ndarray:
    """save_image's 8-bit conversion: truncation, not rounding (render.py:423).  ``dither="blue"``: the device's dithered
    quantiser restated (bhr_set_dither): floor(clip(x, 0, 1) * 255 + t) in f32, the product and the sum rounded once each;
    ``row0``: the image's first row in the full frame (a row block dithers as the whole frame does)."""
    if dither not in DITHERS:
        raise ValueError(f"dither must be one of {DITHERS}, got {dither!r}")
    if dither == "none":
        return (np.clip(image, 0, 1) * 255).astype(np.uint8)
    x = _clip01(image)
    v = x * np.float32(255.0)
    return np.floor(v + dither_thresholds(x.shape[0], x.shape[1], row0)).astype(np.uint8)


def quantize16(image: np.ndarray) -> np.ndarray:
    """The 16-bit conversion of bhr_read_final_u16: (uint16)(clip(x, 0, 1) * 65535) in f32, truncated; NaN -> 0."""
    return (_clip01(image) * np.float32(65535.0)).astype(np.uint16)


class FrameSink:
    """Device frame -> PNG (or, with ``codec="jpeg"``, JPEG) file without stalling the render stream.

    ``submit(path)`` quantises the renderer's FINAL layer on the device, starts the copy into a pinned
    host slot and returns; worker threads encode and write.  ``drain()`` waits for the files.
    ``level=DEVICE`` encodes on the GPU as well: the workers only fetch the finished bytes and write them.
    ``codec="jpeg"``: baseline JPEG of ``quality`` 1..100, always coded on the GPU (``level`` is not used).
    ``bit_depth=16`` (PNG only): the files are 16-bit PNGs of the renderer's 16-bit rows (bhr_sink_create_png16)."""

    def __init__(self, renderer, slots: int = 0, workers: int = 0, level: int = VIDEO_LEVEL, codec: str = "png",
                 quality: int = JPEG_QUALITY, bit_depth: int = 8):
        if codec not in ("png", "jpeg"):
            raise ValueError(f"codec must be 'png' or 'jpeg', got {codec!r}")
        if bit_depth not in (8, 16) or (bit_depth == 16 and codec != "png"):
            raise ValueError(f"bit_depth must be 8, or 16 with codec 'png'; got {bit_depth!r} with {codec!r}")
        if workers <= 0:
            workers = max(1, min(16, len(os.sched_getaffinity(0)) - 1))
        if slots <= 0:
            slots = workers + 4        # every encoder busy plus a few frames of slack for the renderer
        self._lib = _lib.load()
        self._sink = C.c_void_p()
        self._renderer = renderer          # keeps the context alive
        if codec == "jpeg":
            _lib.check(self._lib.bhr_sink_create_jpeg(renderer._ctx, slots, workers, int(quality), C.byref(self._sink)))
        elif bit_depth == 16:
            _lib.check(self._lib.bhr_sink_create_png16(renderer._ctx, slots, workers, level, C.byref(self._sink)))
        else:
            _lib.check(self._lib.bhr_sink_create(renderer._ctx, slots, workers, level, C.byref(self._sink)))
        self.workers, self.slots, self.level, self.codec, self.quality = workers, slots, level, codec, quality
        self.bit_depth = bit_depth
        import weakref
        if not hasattr(renderer, "_sinks"):
            renderer._sinks = []
        renderer._sinks.append(weakref.ref(self))

    def submit(self, path: str) -> None:
        _lib.check(self._lib.bhr_sink_submit(self._sink, os.fsencode(path)))

    def drain(self):
        """-> (frames written, bytes written) since creation."""
        frames, nbytes = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.bhr_sink_drain(self._sink, C.byref(frames), C.byref(nbytes)))
        return frames.value, nbytes.value

    def close(self) -> None:
        if self._sink:
            self._lib.bhr_sink_destroy(self._sink)
            self._sink = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rgb_to_yuv420(rgb_u8: np.ndarray):
    """The stream's colour conversion on the host (checker for the device kernel; integer BT.601 limited range,
    chroma from the rounded mean of each 2x2 block): (H, W, 3) uint8 -> (Y (H, W), Cb (H/2, W/2), Cr (H/2, W/2))."""
    a = _u8(rgb_u8).astype(np.int32)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    h, w = r.shape
    m = (a.reshape(h // 2, 2, w // 2, 2, 3).sum(axis=(1, 3)) + 2) >> 2
    r, g, b = m[..., 0], m[..., 1], m[..., 2]
    cb = ((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128
    cr = ((112 * r - 94 * g - 18 * b + 128) >> 8) + 128
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def read_y4m(path: str):
    """Minimal YUV4MPEG2 reader (4:2:0): -> (header dict, list of (Y, Cb, Cr) uint8 planes).  A ``C420p10`` file (the HDR
    stream) gives uint16 planes, from little-endian samples."""
    with open(path, "rb") as f:
        head = f.readline().decode("ascii").split()
        assert head[0] == "YUV4MPEG2", head
        tags = {t[0]: t[1:] for t in head[1:]}
        w, h = int(tags["W"]), int(tags["H"])
        deep = tags.get("C") == "420p10"
        dtype, nbytes = (np.dtype("<u2"), w * h * 3) if deep else (np.dtype(np.uint8), w * h * 3 // 2)
        frames = []
        while True:
            line = f.readline()
            if not line:
                break
            assert line.startswith(b"FRAME"), line[:20]
            raw = f.read(nbytes)
            assert len(raw) == nbytes, "truncated frame"
            buf = np.frombuffer(raw, dtype=dtype)
            if deep:
                buf = buf.astype(np.uint16)
            frames.append((buf[:w * h].reshape(h, w), buf[w * h:w * h * 5 // 4].reshape(h // 2, w // 2),
                           buf[w * h * 5 // 4:].reshape(h // 2, w // 2)))
    return {"width": w, "height": h, "fps": tags["F"], "chroma": [t for t in head[1:] if t.startswith("C")][0],
            "tags": head[1:]}, frames


HDR_TRANSFERS = ("pq", "hlg")
HDR_WHITE_NITS = 203.0      # BT.2408's reference white: the display level of scene value 1.0 under PQ


def check_hdr(hdr):
    """The ``hdr`` of a Y4MStream -- None, or a dict with ``transfer`` ("pq" | "hlg") and any of ``exposure`` (stops, -16 .. 16)
    and ``white_nits`` (PQ: the display level of scene value 1.0, in (0, 10000]) -- checked and completed with the defaults:
    None or dict(transfer, exposure, white_nits).  Raises ValueError; needs no device."""
    if hdr is None:
        return None
    if not isinstance(hdr, dict):
        raise ValueError(f"hdr must be None or a dict, got {hdr!r}")
    unknown = set(hdr) - {"transfer", "exposure", "white_nits"}
    if unknown:
        raise ValueError(f"unknown hdr settings {sorted(unknown)}")
    transfer = hdr.get("transfer")
    if transfer not in HDR_TRANSFERS:
        raise ValueError(f"hdr transfer must be one of {HDR_TRANSFERS}, got {transfer!r}")
    exposure, white = hdr.get("exposure", 0.0), hdr.get("white_nits", HDR_WHITE_NITS)
    for name, v in (("exposure", exposure), ("white_nits", white)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"hdr {name} must be a number, got {v!r}")
    if not (np.isfinite(exposure) and -16.0 <= exposure <= 16.0):
        raise ValueError(f"hdr exposure must be between -16 and 16 stops, got {exposure!r}")
    if transfer == "pq" and not (np.isfinite(white) and 0.0 < white <= 10000.0):
        raise ValueError(f"hdr white_nits must be greater than 0 and at most 10000, got {white!r}")
    return dict(transfer=transfer, exposure=float(exposure), white_nits=float(white))


class Y4MStream:
    """Device frames -> one YUV4MPEG2 (yuv420p) stream, in submission order, without a PNG detour
    (replaces the PNG -> imread -> libx264 assembly of render.py:4497-4503; include/bhr_output.h).

    ``hdr`` = dict(transfer="pq" | "hlg", exposure=0.0, white_nits=203.0): the HDR stream instead (bhr_y4m_open_hdr): 10-bit
    BT.2020 frames (``C420p10``) made from the scene-linear HDR plane of every submitted frame, which must have kept it
    (set_grade(..., keep_hdr=True)); ``light_levels()`` gives its MaxCLL and MaxFALL."""

    def __init__(self, renderer, path: str, fps: int, slots: int = 8, hdr=None):
        self.hdr = check_hdr(hdr)
        self._lib = _lib.load()
        self._s = C.c_void_p()
        self._renderer = renderer
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        if self.hdr is None:
            _lib.check(self._lib.bhr_y4m_open(renderer._ctx, os.fsencode(path), int(fps), 1, slots, C.byref(self._s)))
        else:
            cfg = _lib.HdrStream(_lib.HDR_PQ if self.hdr["transfer"] == "pq" else _lib.HDR_HLG, self.hdr["exposure"],
                                 self.hdr["white_nits"], 0)
            _lib.check(self._lib.bhr_y4m_open_hdr(renderer._ctx, os.fsencode(path), int(fps), 1, slots, C.byref(cfg), C.byref(self._s)))
        import weakref
        if not hasattr(renderer, "_sinks"):
            renderer._sinks = []
        renderer._sinks.append(weakref.ref(self))

    def submit(self) -> None:
        _lib.check(self._lib.bhr_y4m_submit(self._s))

    def drain(self):
        frames, nbytes = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.bhr_y4m_drain(self._s, C.byref(frames), C.byref(nbytes)))
        return frames.value, nbytes.value

    def light_levels(self):
        """(MaxCLL, MaxFALL) in nits of the frames written so far (call it after drain()): the largest pixel and the largest
        frame mean of min(white_nits * max(R, G, B), 10000) over the linear BT.2020 values.  (0.0, 0.0) for an HLG stream,
        which carries no such metadata, and for an 8-bit stream."""
        out = (C.c_double * 2)()
        _lib.check(self._lib.bhr_y4m_light_levels(self._s, out))
        return float(out[0]), float(out[1])

    def close(self) -> None:
        if self._s:
            self._lib.bhr_y4m_close(self._s)
            self._s = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- geometry passes of a ray map (HipRenderer.ray_map_passes) -----------------------------------------------------------
PASS_DTYPES = {"steps": np.int32, "status": np.int32, "crossings": np.int32, "escape_dir": np.float32, "hits": np.float32,
               "hit_r": np.float32, "hit_phi": np.float32}
PASS_LAYERS = ("bg", "disk", "blur")


def hit_polar(hits: np.ndarray, crossings: np.ndarray):
    """Radius and azimuth of every pixel's FIRST disk crossing in the disk's own plane, from the map's records: with
    (hx, hy) = hits[0, ..., 0:2] in float32, ``hit_r = sqrt(hx * hx + hy * hy)`` (the march's annulus test, operation for
    operation) and ``hit_phi = arctan2(hy, hx)`` in (-pi, pi]; NaN where ``crossings == 0``.  Returns (hit_r, hit_phi), each
    (H, W) float32."""
    hits = np.asarray(hits, dtype=np.float32)
    crossings = np.asarray(crossings)
    if hits.ndim != 4 or hits.shape[3] not in (5, 9) or hits.shape[1:3] != crossings.shape:
        raise ValueError(f"hits must be (K, H, W, 5 | 9) and crossings (H, W), got {hits.shape} and {crossings.shape}")
    hx, hy = hits[0, ..., 0], hits[0, ..., 1]
    r = np.sqrt(hx * hx + hy * hy, dtype=np.float32)
    phi = np.arctan2(hy, hx, dtype=np.float32)
    none = crossings <= 0
    return np.where(none, np.float32(np.nan), r).astype(np.float32), np.where(none, np.float32(np.nan), phi).astype(np.float32)


def write_passes(path: str, passes: dict, layers: dict = None, hole: dict = None) -> None:
    """The geometry passes of a ray map (HipRenderer.ray_map_passes) and, with ``layers``, the frame's ``bg`` / ``disk`` /
    ``blur`` layers ((H, W, 3) float32 each) as one compressed ``.npz``: the integer passes as int32, everything else as
    float32, under the keys they came with.  ``hole``: dict(spin=, redshift=) of a Kerr ray map's passes
    (HipRenderer.kerr_ray_map_passes), stored as ``spin`` (float32) and ``redshift`` ("model" or "exact").  A host function; needs
    no device."""
    if not str(path).lower().endswith(".npz"):
        raise ValueError(f"the passes are written as a .npz file, got {path!r}")
    missing = [k for k in ("steps", "status", "escape_dir", "crossings", "hits") if k not in passes]
    if missing:
        raise ValueError(f"passes lack {missing}")
    unknown = sorted(set(passes) - set(PASS_DTYPES))
    if unknown:
        raise ValueError(f"unknown passes {unknown}")
    shape = np.asarray(passes["steps"]).shape
    if len(shape) != 2:
        raise ValueError(f"steps must be (H, W), got {shape}")
    out = {}
    for name, a in passes.items():
        a = np.ascontiguousarray(a, dtype=PASS_DTYPES[name])
        want = {"escape_dir": shape + (3,), "hits": a.shape[:1] + shape + a.shape[3:]}.get(name, shape)
        if a.shape != want or (name == "hits" and (a.ndim != 4 or a.shape[3] not in (5, 9))):
            raise ValueError(f"pass {name!r} has shape {a.shape} in a {shape} frame")
        out[name] = a
    for name, a in (layers or {}).items():
        if name not in PASS_LAYERS:
            raise ValueError(f"layers are {PASS_LAYERS}, got {name!r}")
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != shape + (3,):
            raise ValueError(f"layer {name!r} has shape {a.shape} in a {shape} frame")
        out[name] = a
    if hole is not None:
        if set(hole) != {"spin", "redshift"} or hole["redshift"] not in ("model", "exact"):
            raise ValueError(f"hole takes spin and redshift ('model' or 'exact'), got {hole!r}")
        out["spin"] = np.float32(hole["spin"])
        out["redshift"] = np.array(hole["redshift"])
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    np.savez_compressed(path, **out)
