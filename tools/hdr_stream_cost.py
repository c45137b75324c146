#!/usr/bin/env python
"""HDR video stream: what it costs the video loop ("HDR video stream").

drivers.render_video at fhd as bench.py's video leg runs it (orbit camera, populations ticking, texture regenerated every frame,
PNG frames encoded on the device and written to a temporary directory), in three configurations: no stream
(video_stream="off"), the 8-bit yuv420p stream into a .y4m file, and the HDR stream (video_hdr="pq") into a .y4m file.  One
renderer, the configurations interleaved, --reps passes over all of them, --frames frames each; the figure is frames over the
loop's own time (render_video's stats: the one-off set-up apart), ending in the drain of the sink and the stream.  The files go
to --tmp (default: /dev/shm where it exists, so that a disk is not what is measured; a frame of the HDR stream is 12.4 MB).

A tree without the HDR stream (the parent commit) runs the first two configurations: --root selects the tree.
With BHR_HDR_TIMING=1 in the environment the library also prints the conversion kernel's own time from HIP events when the HDR
stream closes.

usage: python tools/hdr_stream_cost.py [--frames 120] [--reps 3] [--root DIR] [--out profiles/hdr_stream.json]
"""
import argparse
import inspect
import json
import os
import shutil
import sys
import tempfile
import time


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from bhr_amd import drivers
    legs = [("no stream", dict(video_stream="off")), ("y4m 8-bit", dict(video_stream="y4m"))]
    if "video_hdr" in inspect.signature(drivers.render_video).parameters:
        legs.append(("hdr pq", dict(video_stream="y4m", video_hdr="pq")))
    res = {"method": f"render_video at 1920x1080, {args.frames} frames per run, {args.reps} interleaved passes, fps over the frame loop "
                     "(set-up apart, drains included), files in " + (args.tmp or "the default temporary directory"),
           "root": os.path.abspath(args.root), "legs": {name: {"fps": []} for name, _ in legs}}
    r, _, _, _ = drivers.make_renderer(1920, 1080, [6, 0, 0.5], 90, n_stars=6000)
    try:
        for rep in range(args.reps + 1):                         # pass 0 warms up (clocks, allocations, page cache) and is dropped
            for name, kw in legs:
                tmp = tempfile.mkdtemp(prefix="bhr_hdr_cost_", dir=args.tmp)
                try:
                    st = {}
                    t0 = time.perf_counter()
                    drivers.render_video(r, 1920, 1080, n_frames=args.frames if rep else 16, fps=30, output_path=os.path.join(tmp, "v.mp4"),
                                         fov=90, static_cam_pos=[6, 0, 0.5], orbit=True, assemble=False, stats=st, **kw)
                    if rep:
                        res["legs"][name]["fps"].append(st["frames"] / st["loop_s"])
                        res["legs"][name]["wall_s"] = time.perf_counter() - t0
                finally:
                    shutil.rmtree(tmp, ignore_errors=True)
    finally:
        r.close()
    for name, leg in res["legs"].items():
        f = sorted(leg["fps"])
        leg["median_fps"], leg["spread"] = f[len(f) // 2], (f[-1] - f[0]) / f[len(f) // 2]
        print(f"{name:10s} fps " + " ".join(f"{x:7.1f}" for x in leg["fps"]) + f"   median {leg['median_fps']:7.1f}  spread {100 * leg['spread']:.1f} %",
              flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
