#!/usr/bin/env python
"""Supersampled Kerr ray maps: what a frame from a Kerr map of factor k costs against the marched supersampled Kerr frame
("Supersampled Kerr ray maps").

The fhd bench scene at pov (6, 0, 0.5) around the hole of --spin (default 0.9), per redshift mode and factor k, in ONE process:
a context with two frames in flight that holds the map (option "kerr_raymap_supersample" = k; its own supersampling stays 1),
and a second context of the same configuration with set_supersample(k) for the marched frames.  The build is timed by the host
clock around bhr_kerr_raymap_build, which synchronises (the first build allocates, the later ones reuse).  Then two legs --
frames from the map, marched Kerr frames -- alternating, --frames frames each after a warm-up, the round of two legs repeated
--reps times to show the spread.  Per leg and round, from the timing ring of those frames: the mean march bracket (for a map
frame: shade + the re-march of the overflow groups), the mean post-pass bracket, and the frame time as the span from the first
frame's start to the last frame's end over the number of frames, beside the host clock ending in a sync.

The one bar: at every setting the map frame is faster than the marched frame of the same k in every round (exit status 1
otherwise; the file is written either way).

usage: python tools/kerr_map_supersample_timing.py [--frames 200] [--reps 3] [--spin 0.9] [--factors 2,4]
                                                    [--out profiles/kerr_map_supersample_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("map", "marched")


def frame(r_map, r_ss, wl, leg):
    if leg == "map":
        r_map.render_from_kerr_ray_map_async(t_offset=0.0)
    else:
        r_ss.render_async(wl["cam_pos"], wl["fov"])


def time_leg(r_map, r_ss, wl, leg, frames, warm):
    r = r_map if leg == "map" else r_ss
    for _ in range(warm):
        frame(r_map, r_ss, wl, leg)
    r.sync()
    r.timing_reset()
    t0 = time.perf_counter()
    for _ in range(frames):
        frame(r_map, r_ss, wl, leg)
    r.sync()
    host_ms = (time.perf_counter() - t0) / frames * 1e3
    c = r.counters()
    n = int(c["frames_timed"])
    return {"frames": n, "march_ms": c["march_ms_sum"] / n, "post_ms": c["bloom_ms_sum"] / n, "frame_ms": c["span_ms"] / n,
            "host_ms": host_ms, "ray_steps_per_frame": int(c["ray_steps_sum"]) // n}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--spin", type=float, default=0.9)
    ap.add_argument("--factors", default="2,4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kerr_map_supersample_timing.json"))
    args = ap.parse_args()
    if not (1 <= args.frames <= 500):
        ap.error("--frames: 1 .. 500 (the timing ring holds 510 frames)")
    factors = [int(k) for k in args.factors.split(",")]
    if any(k not in (1, 2, 4, 8) for k in factors):
        ap.error("--factors: 1, 2, 4 or 8")
    import bench
    from bhr_amd import workloads
    wl = bench.WORKLOADS["fhd"]
    res = {"method": f"per redshift mode and factor: a hybrid two-slot context with the Kerr map (kerr_raymap_supersample = k) and a second one with "
                     f"set_supersample(k) (the post-pass follows the mode; the Kerr march has one arithmetic); legs {LEGS} alternating in one process, "
                     f"{args.frames} frames each after {args.warm} warm-up frames, {args.reps} rounds; brackets from the timing ring, "
                     f"frame_ms = span / frames",
           "spin": args.spin, "width": wl["width"], "height": wl["height"], "cam_pos": wl["cam_pos"], "fov": wl["fov"], "modes": {}}
    slower = []
    for mode in ("model", "exact"):
        res["modes"][mode] = {"factors": {}}
        for k in factors:
            r_map, _, _, note = workloads.make_scene(wl, math="hybrid", frame_slots=2)
            r_ss, _, _, _ = workloads.make_scene(wl, math="hybrid", frame_slots=2)
            entry = {"legs": {leg: [] for leg in LEGS}}
            try:
                res["modes"][mode]["scene"] = note
                for r in (r_map, r_ss):
                    r.set_spin(args.spin)
                    r.set_redshift(mode)
                r_ss.set_supersample(k)
                t_spin = time.perf_counter()                      # clocks up, slot streams calibrated
                while time.perf_counter() - t_spin < 0.5:
                    for _ in range(8):
                        r_map.render_async(wl["cam_pos"], wl["fov"])
                    r_map.sync()
                builds = []
                for _ in range(3):                                # the first build allocates, the later ones reuse
                    t0 = time.perf_counter()
                    r_map.build_kerr_ray_map(wl["cam_pos"], wl["fov"], supersample=k)
                    builds.append((time.perf_counter() - t0) * 1e3)
                info = r_map.kerr_ray_map_info()
                px = k * k * wl["width"] * wl["height"]
                entry.update(build_ms=builds, supersample=info["supersample"], slots=info["slots"], device_bytes=info["device_bytes"],
                             build_ray_steps=info["ray_steps"], overflow_pixels=info["overflow_pixels"], overflow_share=info["overflow_pixels"] / px,
                             crossings_stored_per_ray=info["crossings_stored"] / px)
                for _ in range(args.reps):
                    for leg in LEGS:
                        entry["legs"][leg].append(time_leg(r_map, r_ss, wl, leg, args.frames, args.warm))
            finally:
                r_map.close()
                r_ss.close()
            rounds = list(zip(entry["legs"]["map"], entry["legs"]["marched"]))
            entry["marched_over_map"] = [b["frame_ms"] / a["frame_ms"] for a, b in rounds]
            entry["map_faster_in_every_round"] = all(a["frame_ms"] < b["frame_ms"] for a, b in rounds)
            if not entry["map_faster_in_every_round"]:
                slower.append((mode, k))
            res["modes"][mode]["factors"][str(k)] = entry
            print(f"{mode} k={k}: build {min(entry['build_ms']):.3f} ms, K={entry['slots']}, overflow {entry['overflow_pixels']} fine px "
                  f"({100 * entry['overflow_share']:.4f} %), {entry['device_bytes'] / 1e6:.0f} MB; marched / map "
                  + " ".join(f"{x:.2f}" for x in entry["marched_over_map"]), flush=True)
            for leg in LEGS:
                rows = entry["legs"][leg]
                print(f"  {leg:7s} march ms " + " ".join(f"{x['march_ms']:8.3f}" for x in rows) + "   frame ms " +
                      " ".join(f"{x['frame_ms']:8.3f}" for x in rows) + "   host ms " + " ".join(f"{x['host_ms']:8.3f}" for x in rows), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:                        # after every factor: a long run leaves what it has
                json.dump(res, f, indent=1)
    if slower:
        print(f"the map frame is NOT faster than the marched frame in every round at {slower}", flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
