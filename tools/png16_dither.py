#!/usr/bin/env python3
"""Measurements behind DESIGN section 5, "16-bit PNG and blue-noise dither" -> profiles/png16_dither.json.

    python tools/png16_dither.py measure --out profiles/png16_dither.json [--hist scanlines.npz]
        file sizes of the fhd bench frame (16-bit: device PNG with its own menu and with the 8-bit menu, host zlib 1 / 6, raw;
        8-bit device PNG, host zlib 6 and JPEG quality 90 with dither off and on) and the fhd video loop (default, 16-bit
        device frames, dithered 8-bit frames): a host clock around the frame loop, each leg twice, alternating.
        --hist: also the per-scanline histograms of the 16-bit file's filtered bytes (what a code menu is fitted to).
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/png16_dither.py kernels fhd|4k|8k
        the workload for the kernel times: quantize_u8 / quantize_u16 / quantize_u8_dither and the 8- and 16-bit PNG kernels,
        several times over one rendered frame of that size.
"""
import argparse
import json
import os
import shutil
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

SIZES = {"fhd": (1920, 1080), "4k": (3840, 2160), "8k": (7680, 4320)}


def bench_frame(w, h):
    """The default view of the bench (pov 6 0 0.5, fov 90, lifecycle texture at t = 0), rendered; -> renderer."""
    import bhr_amd  # noqa: F401
    from bhr_amd import drivers
    r, _, n_r, n_phi = drivers.make_renderer(w, h, [6, 0, 0.5], 90, n_stars=6000, math="hybrid")
    factories = drivers.init_lifecycle_system(r, n_r, n_phi, seed=42)
    drivers.advance_lifecycle_frame(r, factories, t=0.0, dt=0.0, recompute_stats=True)
    r.render_async([6, 0, 0.5], 90)
    return r


def filtered_scanlines(png, w, h, bpp):
    at, z = 8, b""
    while at < len(png):
        n = struct.unpack(">I", png[at:at + 4])[0]
        if png[at + 4:at + 8] == b"IDAT":
            z += png[at + 8:at + 8 + n]
        at += 12 + n
    return np.frombuffer(zlib.decompress(z), np.uint8).reshape(h, bpp * w + 1)


def sizes(hist_path=None):
    from bhr_amd import output as O
    w, h = SIZES["fhd"]
    r = bench_frame(w, h)
    u16, u8, final = r.read_final_u16(), r.read_final_u8(), r.read_layer(0)
    s = {"raw16": int(u16.nbytes), "raw8": int(u8.nbytes)}
    png16 = O.png_encode_device(r, bit_depth=16)
    s["png16_device"] = len(png16)
    raw = filtered_scanlines(png16, w, h, 6)
    s["png16_filters_used"] = np.bincount(raw[:, 0], minlength=5).tolist()
    if hist_path:
        np.savez_compressed(hist_path, filters=raw[:, 0].copy(),
                            hist=np.stack([np.bincount(row[1:], minlength=256) for row in raw]).astype(np.uint32),
                            hist_high_bytes=np.stack([np.bincount(row[1::2], minlength=256) for row in raw]).astype(np.uint32))
    r.set_option("png16_menu", 0)
    s["png16_device_with_8bit_menu"] = len(O.png_encode_device(r, bit_depth=16))
    r.set_option("png16_menu", 1)
    for level in (1, 6):
        t0 = time.perf_counter()
        s[f"png16_host_zlib{level}"] = len(O.png_encode(u16, level=level, threads=8))
        s[f"png16_host_zlib{level}_seconds_8_threads"] = time.perf_counter() - t0
    s["png8_device"] = len(O.png_encode_device(r))
    s["png8_host_zlib6"] = len(O.png_encode(u8, level=6, threads=8))
    s["jpeg_q90"] = len(O.jpeg_encode_device(r, 90))
    r.set_dither("blue")
    d8 = r.read_final_u8()
    s["png8_device_dither"] = len(O.png_encode_device(r))
    s["png8_host_zlib6_dither"] = len(O.png_encode(d8, level=6, threads=8))
    s["jpeg_q90_dither"] = len(O.jpeg_encode_device(r, 90))
    r.set_dither("none")
    s["u8_levels_in_use"] = int(np.unique(u8).size)
    s["share_of_pixels_below_level_12"] = float((final.max(axis=2) < 12 / 255).mean())
    s["share_of_samples_dither_moves"] = float((d8 != u8).mean())
    r.close()
    return s


def video_loop(kind, n_frames):
    from bhr_amd import drivers
    w, h = SIZES["fhd"]
    tmp = tempfile.mkdtemp(prefix="bhr_png16_dither_")
    try:
        r, _, _, _ = drivers.make_renderer(w, h, [6, 0, 0.5], 90, n_stars=6000, math="hybrid")
        st = {}
        kw = {"png16": dict(bit_depth=16), "dither": dict(dither="blue"), "default": {}}[kind]
        out = os.path.join(tmp, "v.mp4")
        drivers.render_video(r, w, h, n_frames=n_frames, fps=30, output_path=out, fov=90, static_cam_pos=[6, 0, 0.5], orbit=True,
                             assemble=False, video_stream="off", stats=st, **kw)
        d = drivers._frames_dir(out)
        files = [f for f in os.listdir(d) if f.endswith(".png")]
        size = sum(os.path.getsize(os.path.join(d, f)) for f in files)
        r.close()
        return {"leg": kind, "frames": n_frames, "loop_s": st["loop_s"], "fps": n_frames / st["loop_s"],
                "mb_per_frame": size / max(len(files), 1) / 1e6}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def kernels(name):
    from bhr_amd import _lib
    from bhr_amd.output import png_encode_device
    w, h = SIZES[name]
    r = bench_frame(w, h)
    final = r.read_layer(0)
    for _ in range({"fhd": 12, "4k": 8, "8k": 4}[name]):
        r.write_layer(_lib.LAYER_FINAL, final)        # the u8 / u16 rows follow the written frame: every pass quantises anew
        r.set_dither("none")
        a = png_encode_device(r)                      # quantize_u8_kernel + the 8-bit PNG kernels
        b = png_encode_device(r, bit_depth=16)        # quantize_u16_kernel + the 16-bit PNG kernels
        r.set_dither("blue")
        c = png_encode_device(r)                      # quantize_u8_dither_kernel + the 8-bit PNG kernels
    print(f"{name}: 8-bit {len(a)} B, 16-bit {len(b)} B, dithered 8-bit {len(c)} B")
    r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("measure")
    m.add_argument("--out", required=True)
    m.add_argument("--hist", default=None)
    m.add_argument("--frames", type=int, default=2400, help="frames of the 8-bit loops (the 16-bit loop takes a fifth)")
    k = sub.add_parser("kernels")
    k.add_argument("size", choices=sorted(SIZES))
    args = ap.parse_args()
    if args.cmd == "kernels":
        kernels(args.size)
        return 0
    out = {"what": "tools/png16_dither.py measure", "fhd_sizes_bytes": sizes(args.hist)}
    print(json.dumps(out["fhd_sizes_bytes"], indent=1), flush=True)
    legs = []
    for _ in range(2):
        for kind, n in (("default", args.frames), ("png16", max(args.frames // 5, 1)), ("dither", args.frames)):
            legs.append(video_loop(kind, n))
            print(json.dumps(legs[-1]), flush=True)
    out["fhd_video_loops"] = legs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
