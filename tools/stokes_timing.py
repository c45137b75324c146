#!/usr/bin/env python
"""Polarisation: what the Stokes pass costs a frame from the ray map ("Polarisation").

Two scenes -- the fhd bench scene (bench.WORKLOADS["fhd"]) and the 4k one (3840 x 2160, disk tilted by 25 degrees, anti-aliased: a
map with differentials; no lens flare here) -- each on one hybrid context per number of frame slots (1: every kernel alone on its
stream, so the brackets are kernel times; 2: frames overlap, what a video pays).  Legs alternate in one process, --frames frames
each after a warm-up, the round repeated --reps times:
  off   frames from the map, no polarisation: the kernels of the commit before it, byte for byte (profiles/stokes_code_objects.txt)
  on    the same frames with a toroidal field set: the Stokes kernel and the cell reduction behind the shade launch
The timing ring brackets a frame as march (the shade launch and the fix launch over the overflow list: the yardstick) and post
(march end to frame end: bloom H, V + combine -- and, with a polarisation set, the Stokes pass, which is launched behind the
march bracket).  stokes_ms = post_ms(on) - post_ms(off) of the means with one frame slot; stokes_over_shade = stokes_ms / march_ms.

usage: python tools/stokes_timing.py [--frames 200] [--reps 3] [--sizes fhd,4k] [--out profiles/stokes_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_leg(r, frames):
    for _ in range(16):
        r.render_from_ray_map_async(t_offset=0.0)
    r.sync()
    r.timing_reset()
    t0 = time.perf_counter()
    for _ in range(frames):
        r.render_from_ray_map_async(t_offset=0.0)
    r.sync()
    host_ms = (time.perf_counter() - t0) / frames * 1e3
    c = r.counters()
    n = int(c["frames_timed"])
    return {"frames": n, "march_ms": c["march_ms_sum"] / n, "post_ms": c["bloom_ms_sum"] / n, "frame_ms": c["span_ms"] / n, "host_ms": host_ms}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="fhd,4k")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stokes_timing.json"))
    args = ap.parse_args()
    if not (1 <= args.frames <= 500):
        ap.error("--frames: 1 .. 500 (the timing ring holds 510 frames)")
    import bench
    from bhr_amd import workloads
    scenes = {"fhd": dict(bench.WORKLOADS["fhd"]), "4k": dict(bench.WORKLOADS["4k"], lens_flare=False)}
    sizes = args.sizes.split(",")
    if any(s not in scenes for s in sizes):
        ap.error(f"--sizes: a comma-separated list of {sorted(scenes)}")
    res = {"method": f"per scene and number of frame slots one hybrid context; legs off / on alternating in one process, {args.frames} frames each "
                     f"after 16 warm-up frames, {args.reps} rounds; march_ms = the shade + fix bracket, post_ms = march end to frame end (holds "
                     f"the Stokes pass), frame_ms = span of the timing ring / frames; stokes_ms = post_ms(on) - post_ms(off), one frame slot",
           "scenes": {}}
    for size in sizes:
        wl = scenes[size]
        out = {"width": wl["width"], "height": wl["height"], "disk_tilt": wl["disk_tilt"], "anti_alias": wl["anti_alias"], "slots": {}}
        for slots in (1, 2):
            r, _, _, note = workloads.make_scene(wl, math="hybrid", frame_slots=slots)
            legs = {"off": [], "on": []}
            try:
                t_spin = time.perf_counter()                          # clocks up, slot streams calibrated
                while time.perf_counter() - t_spin < 0.5:
                    for _ in range(8):
                        r.render_async(wl["cam_pos"], wl["fov"])
                    r.sync()
                r.build_ray_map(wl["cam_pos"], wl["fov"])
                info = r.ray_map_info()
                out.update(scene=note, diff=info["diff"], map_slots=info["slots"], overflow_pixels=info["overflow_pixels"],
                           resources=r.stokes_resources(bool(info["diff"])))
                for _ in range(args.reps):
                    for leg in legs:
                        r.set_polarization("toroidal" if leg == "on" else None)
                        legs[leg].append(time_leg(r, args.frames))
                r.set_polarization(None)
            finally:
                r.close()
            mean = {leg: {k: sum(x[k] for x in rows) / len(rows) for k in ("march_ms", "post_ms", "frame_ms", "host_ms")} for leg, rows in legs.items()}
            out["slots"][str(slots)] = {"legs": legs, "mean": mean}
            print(f"{size}, {slots} frame slot(s): Stokes kernel {out['resources']}, overflow {out['overflow_pixels']} px", flush=True)
            for leg, rows in legs.items():
                print(f"  {leg:4s} march ms " + " ".join(f"{x['march_ms']:7.4f}" for x in rows) + "   post ms " + " ".join(f"{x['post_ms']:7.4f}" for x in rows) +
                      "   frame ms " + " ".join(f"{x['frame_ms']:7.4f}" for x in rows), flush=True)
        one = out["slots"]["1"]["mean"]
        out["stokes_ms"] = one["on"]["post_ms"] - one["off"]["post_ms"]
        out["shade_ms"] = one["off"]["march_ms"]
        out["stokes_over_shade"] = out["stokes_ms"] / out["shade_ms"]
        two = out["slots"]["2"]["mean"]
        out["frame_ms_two_slots"] = {"off": two["off"]["frame_ms"], "on": two["on"]["frame_ms"]}
        print(f"  Stokes pass {out['stokes_ms']:.4f} ms, shade bracket {out['shade_ms']:.4f} ms: {out['stokes_over_shade']:.2f} of it", flush=True)
        res["scenes"][size] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
