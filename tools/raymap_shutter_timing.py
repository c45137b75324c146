#!/usr/bin/env python
"""Motion blur from the ray map: what a shutter frame shaded from ONE map costs against a marched one ("Shutter frames
from the map").

Two views: the fhd bench scene, and the 4k anti-aliased one with the lens flare over a disk that is NOT tilted (an orbit needs
one), each on ONE hybrid context with two frames in flight.  The exposures are an orbit's: shutter 0.5 of a frame time, n samples
at drivers.shutter_times, the camera stepping round the orbit of the video driver (camera.orbit_position over --orbit_frames
positions); the map is built once for position 0.  Per view and n in --samples, five legs alternate in this process, --frames
frames each after a warm-up, the round of five repeated --reps times to show the spread:
  fused      bhr_raymap_render_shutter, option "raymap_shutter_fused" 1: one launch shades all samples
  unfused    bhr_raymap_render_shutter, option 0: per sample a shade launch, the fix launch and an accumulation launch
  hybrid     bhr_render_shutter, hybrid arithmetic     } the behaviour of the commit before this one:
  strict     bhr_render_shutter, strict arithmetic     } the baseline
  map_frame  single map frames of the orbit (bhr_raymap_render_view), for scale
Per leg and round, from the timing ring of those frames: the mean march bracket, the mean post-pass bracket, and the frame time
as the span from the first frame's start to the last frame's end over the number of frames (two frames in flight overlap), beside
the host clock ending in a sync.  A map with overflow pixels takes the unfused route whatever the option says: the JSON records
the count, and then "fused" is not the fused route.

The summary per view and n: fused as a ratio to hybrid and to strict, and whether fused beats unfused by more than the spread of
the rounds of either leg (max - min of frame_ms) -- the rule by which the fused route stays the default, taken at fhd n = 8.

usage: python tools/raymap_shutter_timing.py [--frames 200] [--reps 3] [--views fhd,4k] [--samples 4,8,16]
                                             [--orbit_frames 3600] [--out profiles/raymap_shutter_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("fused", "unfused", "hybrid", "strict", "map_frame")
SHUTTER = 0.5
WARMUP = 8


def make_frames(wl, n, n_orbit, count):
    """Per frame f: the positions and t_offsets render_video's shutter loop makes for it, and the frame's own camera."""
    from bhr_amd import drivers
    from bhr_amd.camera import orbit_position
    out = []
    for f in range(count):
        u = drivers.shutter_times(f, SHUTTER, n)
        out.append(([[float(v) for v in orbit_position(wl["cam_pos"], t, n_orbit)] for t in u], [(t - f) * 0.1 for t in u],
                    [float(v) for v in orbit_position(wl["cam_pos"], f, n_orbit)]))
    return out


def frame(r, wl, leg, fr):
    flare = bool(wl.get("lens_flare", False))
    pos, toff, cam = fr
    if leg in ("fused", "unfused"):
        r.render_shutter_from_ray_map_async(toff, pos, wl["fov"], lens_flare=flare)
    elif leg == "map_frame":
        r.render_from_ray_map_async(t_offset=0.0, lens_flare=flare, cam_pos=cam, fov=wl["fov"])
    else:
        r.render_shutter_async(pos, wl["fov"], toff, math=leg, lens_flare=flare)


def time_leg(r, wl, leg, frames_of, start, frames):
    if leg in ("fused", "unfused"):
        r.set_option("raymap_shutter_fused", 1 if leg == "fused" else 0)
    for i in range(WARMUP):
        frame(r, wl, leg, frames_of[start + i])
    r.sync()
    r.timing_reset()
    t0 = time.perf_counter()
    for i in range(frames):
        frame(r, wl, leg, frames_of[start + WARMUP + i])
    r.sync()
    host_ms = (time.perf_counter() - t0) / frames * 1e3
    c = r.counters()
    k = int(c["frames_timed"])
    return {"frames": k, "march_ms": c["march_ms_sum"] / k, "post_ms": c["bloom_ms_sum"] / k, "frame_ms": c["span_ms"] / k,
            "host_ms": host_ms, "ray_steps_per_frame": int(c["ray_steps_sum"]) // k}


def summarize(legs):
    ms = {leg: [x["frame_ms"] for x in rows] for leg, rows in legs.items()}
    mean = {leg: sum(v) / len(v) for leg, v in ms.items()}
    spread = {leg: max(v) - min(v) for leg, v in ms.items()}
    margin = max(spread["fused"], spread["unfused"])
    return {"mean_frame_ms": mean, "spread_frame_ms": spread, "fused_over_hybrid": mean["fused"] / mean["hybrid"],
            "fused_over_strict": mean["fused"] / mean["strict"], "fused_over_unfused": mean["fused"] / mean["unfused"],
            "fused_over_map_frame": mean["fused"] / mean["map_frame"],
            "fused_faster_than_unfused_beyond_spread": bool(mean["unfused"] - mean["fused"] > margin)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--views", default="fhd,4k")
    ap.add_argument("--samples", default="4,8,16")
    ap.add_argument("--orbit_frames", type=int, default=3600, help="positions on the full circle (BASELINE configs[4]: 3600)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raymap_shutter_timing.json"))
    args = ap.parse_args()
    if not (1 <= args.frames <= 500):
        ap.error("--frames: 1 .. 500 (the timing ring holds 510 frames)")
    samples = [int(s) for s in args.samples.split(",")]
    if not all(1 <= n <= 64 for n in samples):
        ap.error("--samples: 1 .. 64 each")
    import bench
    from bhr_amd import workloads
    res = {"method": f"one hybrid context per view, two frames in flight; legs {LEGS} alternating in one process, {args.frames} frames each "
                     f"after {WARMUP} warm-up frames, {args.reps} rounds; orbit exposures of shutter {SHUTTER} round a "
                     f"{args.orbit_frames}-position orbit; brackets from the timing ring, frame_ms = span / frames",
           "views": {}}
    default_rule = None
    for name in args.views.split(","):
        wl = dict(bench.WORKLOADS[name], disk_tilt=0.0)           # an orbit needs a disk that is not tilted
        r, _, _, note = workloads.make_scene(wl, math="hybrid", frame_slots=2)
        view = {"scene": note, "width": wl["width"], "height": wl["height"], "anti_alias": wl["anti_alias"], "disk_tilt": wl["disk_tilt"],
                "lens_flare": bool(wl.get("lens_flare", False)), "samples": {}}
        try:
            t_spin = time.perf_counter()                          # clocks up, slot streams calibrated
            while time.perf_counter() - t_spin < 0.5:
                for _ in range(8):
                    r.render_async(wl["cam_pos"], wl["fov"])
                r.sync()
            per_round = args.frames + WARMUP
            for n in samples:
                frames_of = make_frames(wl, n, args.orbit_frames, per_round * args.reps)
                r.build_ray_map(frames_of[0][2], wl["fov"])
                info = r.ray_map_info()
                legs = {leg: [] for leg in LEGS}
                for rep in range(args.reps):                      # every round a fresh stretch of the orbit, the same for its five legs
                    for leg in LEGS:
                        legs[leg].append(time_leg(r, wl, leg, frames_of, rep * per_round, args.frames))
                entry = {"slots": info["slots"], "diff": info["diff"], "overflow_pixels": info["overflow_pixels"],
                         "fused_route_taken": info["overflow_pixels"] == 0, "legs": legs}
                entry.update(summarize(legs))
                view["samples"][str(n)] = entry
                print(f"{name} n={n}: overflow {info['overflow_pixels']} px", flush=True)
                for leg in LEGS:
                    rows = legs[leg]
                    print(f"  {leg:9s} march ms " + " ".join(f"{x['march_ms']:8.3f}" for x in rows) + "   frame ms " +
                          " ".join(f"{x['frame_ms']:8.3f}" for x in rows) + "   host ms " + " ".join(f"{x['host_ms']:8.3f}" for x in rows), flush=True)
                print(f"  fused / hybrid {entry['fused_over_hybrid']:.3f}, / strict {entry['fused_over_strict']:.3f}, / unfused "
                      f"{entry['fused_over_unfused']:.3f}, / one map frame {entry['fused_over_map_frame']:.2f}; faster than unfused beyond "
                      f"the rounds' spread: {entry['fused_faster_than_unfused_beyond_spread']}", flush=True)
                if name == "fhd" and n == 8:
                    default_rule = entry["fused_faster_than_unfused_beyond_spread"] and entry["fused_route_taken"]
        finally:
            r.close()
        res["views"][name] = view
    res["fused_stays_default"] = default_rule                     # None: fhd n = 8 was not among the runs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
