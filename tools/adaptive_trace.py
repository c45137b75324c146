#!/usr/bin/env python
"""Frames for a kernel trace of adaptive supersampling: the bench scene, hybrid, ONE frame at a time (a kernel's duration
is its own), `--frames` adaptive frames at factor k and threshold T.  Run under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/adaptive_trace.py --workload fhd -k 4 -T 0.0314
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="fhd")
    ap.add_argument("-k", type=int, default=4)
    ap.add_argument("-T", type=float, default=8 / 255)
    ap.add_argument("--frames", type=int, default=200)
    args = ap.parse_args()
    import bench
    from bhr_amd import workloads
    wl = bench.WORKLOADS[args.workload]
    r, _, _, _ = workloads.make_scene(wl, math="hybrid", frame_slots=1)
    r.set_supersample(args.k, args.T)
    for _ in range(args.frames):
        r.render_async(wl["cam_pos"], wl["fov"])
    r.sync()
    print(r.adaptive_info())
    r.close()


if __name__ == "__main__":
    main()
