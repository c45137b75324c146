"""Motion-JPEG video against the default (PNG) video loop on the GPU -> profiles/video_mjpeg.json.

    python tools/video_codec.py [--frames 300] [--repeats 2] [--parent-root DIR] [--kernel-stats CSV] [--out FILE]

Legs, each a fresh process, every leg `--repeats` times, alternating:
  * the configs[4] video loop (1920x1080, orbit, lifecycle ticking, frame files on disk; host clock around the frame
    loop, which ends in the sink's drain) with video_codec="auto" and "mjpeg" (quality 90) of this tree, and, with
    --parent-root (a checkout of the parent commit with its library built), the parent's default loop;
  * once each: the mjpeg loop at quality 75 and 95 (bytes per frame).
Then, in this process: one fhd frame's JPEG size against the restatement without restart intervals (the overhead of R),
and the synchronous encode calls at fhd / 4k / 8k.  Kernel times come from a separate run of

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/video_codec.py --kernels

whose *kernel_trace.csv is passed back with --kernel-stats (median duration per kernel and grid size).
"""
import argparse
import csv
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

WL = {"fhd": dict(width=1920, height=1080, cam_pos=[6, 0, 0.5], fov=90, step_size=0.1, disk_tilt=0.0, anti_alias="disabled"),
      "4k": dict(width=3840, height=2160, cam_pos=[6, 0, 0.5], fov=90, step_size=0.1, disk_tilt=25.0, anti_alias="lod_radius"),
      "8k": dict(width=7680, height=4320, cam_pos=[6, 0, 0.5], fov=90, step_size=0.05, disk_tilt=0.0, anti_alias="disabled")}


def leg(root, codec, quality, frames):
    """One video loop in this process, importing the package from `root`; prints one JSON line."""
    sys.path.insert(0, root)
    from bhr_amd import drivers
    tmp = tempfile.mkdtemp(prefix="bhr_video_codec_")
    try:
        r, _, _, _ = drivers.make_renderer(1920, 1080, [6, 0, 0.5], 90, n_stars=6000)
        kw = dict(video_codec=codec, video_quality=quality) if codec != "auto" else {}
        st = {}
        out = os.path.join(tmp, "v.mp4")
        drivers.render_video(r, 1920, 1080, n_frames=frames, fps=30, output_path=out, fov=90, static_cam_pos=[6, 0, 0.5],
                             orbit=True, assemble=False, video_stream="off", stats=st, **kw)
        d = drivers._frames_dir(out)
        files = [f for f in os.listdir(d) if f.startswith("frame_")]
        size = sum(os.path.getsize(os.path.join(d, f)) for f in files)
        r.close()
        print("LEG " + json.dumps({"codec": codec, "quality": quality if codec != "auto" else None, "frames": frames,
                                   "files": len(files), "ext": sorted({os.path.splitext(f)[1] for f in files}),
                                   "loop_s": st["loop_s"], "setup_s": st["setup_s"], "ms_per_frame": 1e3 * st["loop_s"] / frames,
                                   "fps": frames / st["loop_s"], "bytes_per_frame": size / max(len(files), 1)}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def kernels():
    """Encodes at the three sizes, for the profiler: 20 PNG and 20 JPEG encodes of one frame each."""
    sys.path.insert(0, ROOT)
    from bhr_amd import workloads
    from bhr_amd.output import jpeg_encode_device, png_encode_device
    for name, wl in WL.items():
        r, _, _, _ = workloads.make_scene(wl)
        r.render_async(wl["cam_pos"], wl["fov"])
        for _ in range(20):
            png_encode_device(r)
            jpeg_encode_device(r, 90)
        print(f"{name}: done", flush=True)
        r.close()


def kernel_stats(path):
    """Median duration (us) of the PNG and JPEG kernels per grid size, from a rocprofv3 kernel_trace.csv."""
    grids = {}
    for row in csv.DictReader(open(path)):
        name = row["Kernel_Name"]
        if "png_" not in name and "jpeg_" not in name:
            continue
        short = name.split("::")[-1].split("(")[0]
        grids.setdefault((short, int(row["Grid_Size_X"])), []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    out = {}
    for (short, grid), v in sorted(grids.items()):
        v.sort()
        out.setdefault(short, []).append({"grid_size_x": grid, "calls": len(v), "median_us": v[len(v) // 2] / 1e3})
    return out


def run_leg(root, codec, quality, frames):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", codec, "--leg-root", root, "--quality", str(quality), "--frames", str(frames)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    for line in p.stdout.splitlines():
        if line.startswith("LEG "):
            return json.loads(line[4:])
    raise RuntimeError(f"leg {codec} in {root} failed ({p.returncode}): {p.stderr[-1500:]}")


def stills(out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import jpeg_ref
    from bhr_amd import workloads
    from bhr_amd.output import jpeg_encode_device, jpeg_restart_interval, png_encode_device
    out["sync_encode_call"] = {}
    for name, wl in WL.items():
        r, _, _, _ = workloads.make_scene(wl)
        r.render_async(wl["cam_pos"], wl["fov"])
        res = {}
        for codec, fn in (("png", lambda: png_encode_device(r)), ("jpeg_q90", lambda: jpeg_encode_device(r, 90))):
            data = fn()
            t0 = time.perf_counter()
            for _ in range(30):
                data = fn()
            res[codec] = {"ms_per_call": (time.perf_counter() - t0) / 30 * 1e3, "bytes": len(data),
                          "bytes_per_pixel": len(data) / (wl["width"] * wl["height"])}
        out["sync_encode_call"][name] = res
        if name == "fhd":
            u8 = r.read_final_u8()
            R = jpeg_restart_interval(wl["width"])
            dev = jpeg_encode_device(r, 90)
            with_r, without = jpeg_ref.encode(u8, 90, R), jpeg_ref.encode(u8, 90, 0)
            intervals = -(-(120 * 68) // R)
            out["restart_overhead_fhd_q90"] = {"restart_interval": R, "intervals": intervals, "device_is_restatement": dev == with_r,
                                               "bytes_with": len(with_r), "bytes_without": len(without),
                                               "overhead_bytes_per_interval": (len(with_r) - len(without)) / intervals,
                                               "overhead_fraction": len(with_r) / len(without) - 1}
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--kernel-stats", default=None, help="kernel_trace.csv of a rocprofv3 run of --kernels")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_mjpeg.json"))
    ap.add_argument("--leg", default=None, choices=["auto", "mjpeg"])
    ap.add_argument("--leg-root", default=ROOT)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg_root, a.leg, a.quality, a.frames)
    if a.kernels:
        return kernels()
    out = {"what": "configs[4] video loop (1920x1080, orbit, lifecycle, frame files on disk): host clock around the frame loop "
                   "incl. the sink's drain; one process per leg, legs alternating", "frames_per_leg": a.frames, "legs": []}
    plan = ([("parent_auto", a.parent_root, "auto", None)] if a.parent_root else []) + \
        [("auto", ROOT, "auto", None), ("mjpeg_q90", ROOT, "mjpeg", 90)]
    for rep in range(a.repeats):
        for name, root, codec, q in plan:
            res = run_leg(root, codec, q or 90, a.frames)
            res.update(leg=name, repeat=rep)
            out["legs"].append(res)
            print(f"{name} #{rep}: {res['ms_per_frame']:.3f} ms/frame, {res['bytes_per_frame'] / 1e6:.3f} MB/frame", flush=True)
    for q in (75, 95):
        res = run_leg(ROOT, "mjpeg", q, a.frames)
        res.update(leg=f"mjpeg_q{q}", repeat=0)
        out["legs"].append(res)
        print(f"mjpeg_q{q}: {res['ms_per_frame']:.3f} ms/frame, {res['bytes_per_frame'] / 1e6:.3f} MB/frame", flush=True)
    summary = {}
    for res in out["legs"]:
        s = summary.setdefault(res["leg"], {"ms_per_frame": [], "bytes_per_frame": res["bytes_per_frame"]})
        s["ms_per_frame"].append(round(res["ms_per_frame"], 4))
    out["summary"] = summary
    stills(out)
    out["kernels_us"] = kernel_stats(a.kernel_stats) if a.kernel_stats else "not measured"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("summary", "sync_encode_call", "restart_overhead_fhd_q90", "kernels_us")}, indent=1))


if __name__ == "__main__":
    main()
