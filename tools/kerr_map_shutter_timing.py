#!/usr/bin/env python
"""Motion blur from the Kerr ray map: what a shutter frame shaded from ONE Kerr map costs against what the commit before it could
do for the same exposure ("Kerr shutter frames from the map").

The fhd bench scene seen from its pov around a hole of spin --spin, once per redshift mode, on ONE hybrid context with two frames
in flight.  The exposures are an orbit's: shutter 0.5 of a frame time, n samples at drivers.shutter_times, the camera stepping
round the orbit of the video driver (camera.orbit_position over --orbit_frames positions); the Kerr map is built once for
position 0.  Per mode and n in --samples the legs alternate in this process, the round repeated --reps times to show the spread:
  fused       bhr_kerr_raymap_render_shutter, option "kerr_raymap_shutter_fused" 1: one launch shades all samples
  unfused     bhr_kerr_raymap_render_shutter, option 0: per sample a shade launch, the fix launch and an accumulation launch
  map_frames  the exposure's n single Kerr map frames (skip-bloom bhr_kerr_raymap_render_view calls), as they are: no mean, no
              post-pass                                                           } what the commit before this one can do:
  marched     the exposure's n marched Kerr frames (skip-bloom bhr_render calls)  } the baseline
--frames exposures per leg and round after a warm-up; the two baseline legs make n ring entries per exposure and take as many
exposures as the timing ring holds (500 // n at most).  Per leg and round, from the timing ring: the time per EXPOSURE as the span
from the first frame's start to the last frame's end over the number of exposures (two frames in flight overlap), the mean march
and post-pass brackets per ring entry, and the host clock ending in a sync.

--legs map_frames,marched with --root <tree of the commit before this one> times the baseline from that commit's own build (the
two legs use nothing this tool's commit adds); --baseline <its JSON> then puts those rows beside this build's under "parent" and
the summary compares against them.  The summary per mode and n: fused over the (parent's) map_frames and marched legs, whether
fused is below the parent's map_frames in every round, and whether fused beats unfused by more than the spread of the rounds of
either leg (max - min) -- the rule by which the fused route stays the default: at every mode and n measured.

usage: python tools/kerr_map_shutter_timing.py [--frames 200] [--reps 3] [--samples 4,8,16] [--spin 0.9] [--orbit_frames 3600]
           [--legs fused,unfused,map_frames,marched] [--root TREE] [--baseline JSON] [--out profiles/kerr_map_shutter_timing.json]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("fused", "unfused", "map_frames", "marched")
SHUTTER = 0.5
WARMUP = 8
RING = 500


def make_frames(wl, n, n_orbit, count):
    """Per exposure f: the positions and t_offsets render_video's shutter loop makes for it."""
    from bhr_amd import drivers
    from bhr_amd.camera import orbit_position
    out = []
    for f in range(count):
        u = drivers.shutter_times(f, SHUTTER, n)
        out.append(([[float(v) for v in orbit_position(wl["cam_pos"], t, n_orbit)] for t in u], [(t - f) * 0.1 for t in u]))
    return out


def exposure(r, wl, leg, fr):
    pos, toff = fr
    if leg in ("fused", "unfused"):
        r.render_shutter_from_kerr_ray_map_async(toff, pos)
    elif leg == "map_frames":
        for p, t in zip(pos, toff):
            r.render_from_kerr_ray_map_async(t_offset=t, cam_pos=p, skip_bloom=True)
    else:
        for p in pos:
            r.render_async(p, wl["fov"], skip_bloom=True)


def time_leg(r, wl, leg, frames_of, start, frames, n):
    if leg in ("fused", "unfused"):
        r.set_option("kerr_raymap_shutter_fused", 1 if leg == "fused" else 0)
    else:
        frames = max(1, min(frames, RING // n))                   # n ring entries per exposure
    for i in range(WARMUP):
        exposure(r, wl, leg, frames_of[start + i])
    r.sync()
    r.timing_reset()
    t0 = time.perf_counter()
    for i in range(frames):
        exposure(r, wl, leg, frames_of[start + WARMUP + i])
    r.sync()
    host_ms = (time.perf_counter() - t0) / frames * 1e3
    c = r.counters()
    k = int(c["frames_timed"])
    return {"exposures": frames, "ring_entries": k, "march_ms": c["march_ms_sum"] / k, "post_ms": c["bloom_ms_sum"] / k,
            "frame_ms": c["span_ms"] / frames, "host_ms": host_ms, "ray_steps_per_exposure": int(c["ray_steps_sum"]) // frames}


def summarize(legs, parent):
    ms = {leg: [x["frame_ms"] for x in rows] for leg, rows in legs.items()}
    base = {leg: [x["frame_ms"] for x in rows] for leg, rows in (parent or {}).items()}
    mean = lambda v: sum(v) / len(v)
    out = {"mean_frame_ms": {leg: mean(v) for leg, v in ms.items()}, "spread_frame_ms": {leg: max(v) - min(v) for leg, v in ms.items()}}
    if base:
        out["parent_mean_frame_ms"] = {leg: mean(v) for leg, v in base.items()}
    if "fused" in ms:
        for leg in ("map_frames", "marched"):
            ref = base.get(leg) or ms.get(leg)
            if ref:
                out[f"fused_over_{leg}"] = mean(ms["fused"]) / mean(ref)
        ref = base.get("map_frames") or ms.get("map_frames")
        if ref:
            out["fused_below_map_frames_in_every_round"] = bool(max(ms["fused"]) < min(ref))
        if "unfused" in ms:
            margin = max(out["spread_frame_ms"]["fused"], out["spread_frame_ms"]["unfused"])
            out["fused_over_unfused"] = mean(ms["fused"]) / mean(ms["unfused"])
            out["fused_faster_than_unfused_beyond_spread"] = bool(mean(ms["unfused"]) - mean(ms["fused"]) > margin)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", default="4,8,16")
    ap.add_argument("--spin", type=float, default=0.9)
    ap.add_argument("--orbit_frames", type=int, default=3600, help="positions on the full circle (BASELINE configs[4]: 3600)")
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--root", default=HERE, help="the tree whose build is timed (default: this one)")
    ap.add_argument("--baseline", default=None, help="JSON of a --legs map_frames,marched run of the commit before this one")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "kerr_map_shutter_timing.json"))
    args = ap.parse_args()
    if not (1 <= args.frames <= RING):
        ap.error(f"--frames: 1 .. {RING} (the timing ring holds 510 frames)")
    samples = [int(s) for s in args.samples.split(",")]
    if not all(1 <= n <= 64 for n in samples):
        ap.error("--samples: 1 .. 64 each")
    legs_run = [leg for leg in LEGS if leg in args.legs.split(",")]
    if not legs_run or set(args.legs.split(",")) - set(LEGS):
        ap.error(f"--legs: of {LEGS}")
    sys.path.insert(0, os.path.abspath(args.root))
    import bench
    from bhr_amd import workloads
    from bhr_amd.camera import orbit_position
    parent = None
    if args.baseline:
        with open(args.baseline) as f:
            parent = json.load(f)
    wl = bench.WORKLOADS["fhd"]
    res = {"method": f"per redshift mode one hybrid context, two frames in flight; legs {tuple(legs_run)} alternating in one process, {args.frames} "
                     f"exposures each (the baseline legs min({args.frames}, {RING} // n)) after {WARMUP} warm-up exposures, {args.reps} rounds; orbit "
                     f"exposures of shutter {SHUTTER} round a {args.orbit_frames}-position orbit; brackets from the timing ring, "
                     f"frame_ms = span / exposures",
           "spin": args.spin, "width": wl["width"], "height": wl["height"], "cam_pos": wl["cam_pos"], "fov": wl["fov"], "modes": {}}
    rule = []
    for mode in ("model", "exact"):
        r, _, _, note = workloads.make_scene(wl, math="hybrid", frame_slots=2)
        entry_mode = {"scene": note, "samples": {}}
        try:
            r.set_spin(args.spin)
            r.set_redshift(mode)
            t_spin = time.perf_counter()                          # clocks up, slot streams calibrated
            while time.perf_counter() - t_spin < 0.5:
                for _ in range(8):
                    r.render_async(wl["cam_pos"], wl["fov"])
                r.sync()
            per_round = args.frames + WARMUP
            for n in samples:
                frames_of = make_frames(wl, n, args.orbit_frames, per_round * args.reps)
                r.build_kerr_ray_map([float(v) for v in orbit_position(wl["cam_pos"], 0, args.orbit_frames)], wl["fov"])
                info = r.kerr_ray_map_info()
                legs = {leg: [] for leg in legs_run}
                for rep in range(args.reps):                      # every round a fresh stretch of the orbit, the same for its legs
                    for leg in legs_run:
                        legs[leg].append(time_leg(r, wl, leg, frames_of, rep * per_round, args.frames, n))
                base = None if parent is None else parent["modes"][mode]["samples"][str(n)]["legs"]
                entry = {"slots": info["slots"], "overflow_pixels": info["overflow_pixels"], "fused_route_taken": info["overflow_pixels"] == 0,
                         "legs": legs}
                if base is not None:
                    entry["parent"] = base
                entry.update(summarize(legs, base))
                entry_mode["samples"][str(n)] = entry
                print(f"{mode} n={n}: overflow {info['overflow_pixels']} px", flush=True)
                for leg in legs_run:
                    rows = legs[leg]
                    print(f"  {leg:10s} march ms " + " ".join(f"{x['march_ms']:8.3f}" for x in rows) + "   exposure ms " +
                          " ".join(f"{x['frame_ms']:8.3f}" for x in rows) + "   host ms " + " ".join(f"{x['host_ms']:8.3f}" for x in rows), flush=True)
                for leg, rows in (base or {}).items():
                    print(f"  parent {leg:10s} exposure ms " + " ".join(f"{x['frame_ms']:8.3f}" for x in rows), flush=True)
                print("  " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in entry.items() if k.startswith("fused_")), flush=True)
                if "fused_faster_than_unfused_beyond_spread" in entry:
                    rule.append(entry["fused_faster_than_unfused_beyond_spread"] and entry["fused_route_taken"])
        finally:
            r.close()
        res["modes"][mode] = entry_mode
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        res["fused_stays_default"] = bool(rule) and all(rule) if rule else None
        with open(args.out, "w") as f:                            # after every mode: a long run leaves what it has
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
