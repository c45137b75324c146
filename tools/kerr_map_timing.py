#!/usr/bin/env python
"""Kerr ray map: what a frame shaded from the map costs against a marched Kerr frame ("Kerr ray map").

The fhd bench scene at pov (6, 0, 0.5) around the hole of --spin (default 0.9), once per redshift mode, each on ONE context
with two frames in flight.  Per mode: the build (host clock around bhr_kerr_raymap_build, which synchronises), then two legs --
frames from the Kerr map, marched Kerr frames -- alternating in this process, --frames frames each after a warm-up, the round of
two legs repeated --reps times to show the spread.  Per leg and round, from the timing ring of those frames: the mean march
bracket (for a map frame: shade + overflow re-march), the mean post-pass bracket, and the frame time as the span from the first
frame's start to the last frame's end over the number of frames (two frames in flight overlap), beside the host clock ending
in a sync.  Also: overflow pixels and crossings per pixel at the default slot count.

usage: python tools/kerr_map_timing.py [--frames 200] [--reps 3] [--spin 0.9] [--out profiles/kerr_map_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("map", "marched")


def frame(r, wl, leg):
    if leg == "map":
        r.render_from_kerr_ray_map_async(t_offset=0.0)
    else:
        r.render_async(wl["cam_pos"], wl["fov"])


def time_leg(r, wl, leg, frames):
    for _ in range(16):
        frame(r, wl, leg)
    r.sync()
    r.timing_reset()
    t0 = time.perf_counter()
    for _ in range(frames):
        frame(r, wl, leg)
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
    ap.add_argument("--spin", type=float, default=0.9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kerr_map_timing.json"))
    args = ap.parse_args()
    if not (1 <= args.frames <= 500):
        ap.error("--frames: 1 .. 500 (the timing ring holds 510 frames)")
    import bench
    from bhr_amd import workloads
    wl = bench.WORKLOADS["fhd"]
    res = {"method": f"one hybrid context per redshift mode (the post-pass follows it; the Kerr march has one arithmetic), two frames in flight; legs {LEGS} alternating in one process, {args.frames} frames each "
                     f"after 16 warm-up frames, {args.reps} rounds; brackets from the timing ring, frame_ms = span / frames",
           "spin": args.spin, "width": wl["width"], "height": wl["height"], "cam_pos": wl["cam_pos"], "fov": wl["fov"], "modes": {}}
    for mode in ("model", "exact"):
        r, _, _, note = workloads.make_scene(wl, math="hybrid", frame_slots=2)
        r.set_spin(args.spin)
        r.set_redshift(mode)
        out = {"scene": note, "legs": {leg: [] for leg in LEGS}}
        try:
            t_spin = time.perf_counter()                          # clocks up, slot streams calibrated
            while time.perf_counter() - t_spin < 0.5:
                for _ in range(8):
                    r.render_async(wl["cam_pos"], wl["fov"])
                r.sync()
            builds = []
            for _ in range(3):                                    # the first build allocates, the later ones reuse
                t0 = time.perf_counter()
                r.build_kerr_ray_map(wl["cam_pos"], wl["fov"])
                builds.append((time.perf_counter() - t0) * 1e3)
            info = r.kerr_ray_map_info()
            cr = r.kerr_ray_map_passes()["crossings"]
            out.update(build_ms=builds, slots=info["slots"], device_bytes=info["device_bytes"], build_ray_steps=info["ray_steps"],
                       overflow_pixels=info["overflow_pixels"], crossings_per_pixel=float(cr.mean()), max_crossings=int(cr.max()),
                       resources={"march": r.kerr_resources(redshift=mode)})
            for _ in range(args.reps):
                for leg in LEGS:
                    out["legs"][leg].append(time_leg(r, wl, leg, args.frames))
        finally:
            r.close()
        best = {leg: min(x["frame_ms"] for x in out["legs"][leg]) for leg in LEGS}
        out["frame_ms_best"] = best
        out["marched_over_map"] = best["marched"] / best["map"]
        res["modes"][mode] = out
        print(f"{mode}: build {min(out['build_ms']):.3f} ms, K={out['slots']}, overflow {out['overflow_pixels']} px, "
              f"{out['crossings_per_pixel']:.3f} crossings / pixel, {out['device_bytes'] / 1e6:.0f} MB; marched / map {out['marched_over_map']:.2f}", flush=True)
        for leg in LEGS:
            rows = out["legs"][leg]
            print(f"  {leg:7s} march ms " + " ".join(f"{x['march_ms']:7.3f}" for x in rows) + "   frame ms " +
                  " ".join(f"{x['frame_ms']:7.3f}" for x in rows) + "   host ms " + " ".join(f"{x['host_ms']:7.3f}" for x in rows), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
