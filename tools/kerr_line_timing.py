#!/usr/bin/env python
"""The Kerr line profile: what the line pass adds to a frame from the Kerr ray map ("Kerr line profile").

The bench scene seen from its pov around a hole of spin --spin, at fhd and at 3840 x 2160 (the fhd workload's view at that size), once
per redshift mode.  One Kerr map per context; the legs alternate in one process, --reps rounds to show the spread:
  none              bhr_kerr_raymap_render without a line: the frame from the map as the parent commit renders it
  powerlaw_first    the line set: power-law emissivity, first crossing, 256 bins over [0, 2)
  texture_all       texture emissivity, every crossing with the transmittance, 256 bins
  texture_all_4096  the same with 4096 bins (32 KiB of LDS cells per workgroup)
  one_bin           texture_all with 4 bins over [0, 8): every sample lands in one cell -- the contention case
Each leg renders --frames skip-bloom frames after a warm-up, the line's row alternating between 0 and 1 with the frame slots.  Per leg
and round, from the timing ring: frame_ms = span / frames (with two frames in flight they overlap) and the host clock ending in a
sync.  With --slots 1 the frames are serial on one stream, and a leg's frame_ms minus `none`'s is the isolated cost of the pass (its
memset, the kernel and the event behind it); with --slots 2 (the default of every context) it is what a video pays.

usage: python tools/kerr_line_timing.py [--frames 200] [--reps 3] [--spin 0.9] [--sizes fhd,4k] [--slots 2,1] [--out profiles/kerr_line_timing.json]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP = 8
LEGS = {
    "none": None,
    "powerlaw_first": dict(emissivity="powerlaw", orders="first"),
    "texture_all": dict(emissivity="texture", orders="all"),
    "texture_all_4096": dict(emissivity="texture", orders="all", n_bins=4096),
    "one_bin": dict(emissivity="texture", orders="all", n_bins=4, g_range=(0.0, 8.0)),
}
SIZES = {"fhd": (1920, 1080), "4k": (3840, 2160)}


def time_leg(r, line, frames):
    r.set_kerr_line(None) if line is None else r.set_kerr_line(**line)

    def frame(i):
        if line is not None:
            r.set_kerr_line_row(i & 1)
        r.render_from_kerr_ray_map_async(t_offset=0.1 * i, skip_bloom=True)
    for i in range(WARMUP):
        frame(i)
    r.sync()
    r.timing_reset()
    t0 = time.perf_counter()
    for i in range(frames):
        frame(WARMUP + i)
    r.sync()
    host_ms = (time.perf_counter() - t0) / frames * 1e3
    c = r.counters()
    out = {"frame_ms": c["span_ms"] / frames, "host_ms": host_ms, "march_ms": c["march_ms_sum"] / max(int(c["frames_timed"]), 1)}
    if line is not None:
        out["samples"] = r.kerr_line_info(0)["samples"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spin", type=float, default=0.9)
    ap.add_argument("--sizes", default="fhd,4k")
    ap.add_argument("--slots", default="2,1")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "kerr_line_timing.json"))
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import bench
    from bhr_amd import workloads
    res = {"method": f"one context per size, redshift mode and slot count; legs {tuple(LEGS)} alternating in one process, {args.frames} skip-bloom frames "
                     f"each after {WARMUP} warm-up frames, {args.reps} rounds; frame_ms = timing-ring span / frames", "spin": args.spin, "runs": {}}
    for size in args.sizes.split(","):
        wl = dict(bench.WORKLOADS["fhd"], width=SIZES[size][0], height=SIZES[size][1])
        for slots in (int(s) for s in args.slots.split(",")):
            for mode in ("model", "exact"):
                r, _, _, _ = workloads.make_scene(wl, math="hybrid", frame_slots=slots)
                try:
                    r.set_spin(args.spin)
                    r.set_redshift(mode)
                    r.build_kerr_ray_map(wl["cam_pos"], wl["fov"])
                    info = r.kerr_ray_map_info()
                    legs = {leg: [] for leg in LEGS}
                    for _ in range(args.reps):
                        for leg, line in LEGS.items():
                            legs[leg].append(time_leg(r, line, args.frames))
                    mean = {leg: sum(x["frame_ms"] for x in rows) / len(rows) for leg, rows in legs.items()}
                    run = {"legs": legs, "mean_frame_ms": mean, "added_ms": {leg: mean[leg] - mean["none"] for leg in LEGS if leg != "none"},
                           "crossings_stored": info["crossings_stored"], "overflow_pixels": info["overflow_pixels"],
                           "resources": {em: r.kerr_line_resources(mode, em) for em in ("powerlaw", "texture")}}
                    res["runs"][f"{size}/{mode}/slots{slots}"] = run
                    print(f"{size} {mode} slots {slots}: " + ", ".join(f"{leg} {ms:.3f}" for leg, ms in mean.items()) + " ms / frame", flush=True)
                finally:
                    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
