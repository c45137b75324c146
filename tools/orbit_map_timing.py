#!/usr/bin/env python
"""Orbit map: what an orbit frame shaded from ONE turned ray map costs against a marched orbit frame ("Orbit map").

The fhd bench scene (bench.WORKLOADS["fhd"], disk not tilted) on ONE hybrid context with two frames in flight.  The camera goes
round the orbit of the video driver (camera.orbit_position over --orbit_frames positions); the map is built once for position 0.
Four legs alternate in this process, --frames frames each after a warm-up, the round of four repeated --reps times to show the
spread:
  orbit_map   orbit frames from the map turned to the frame's camera (bhr_raymap_render_view)
  static_map  frames from the map at the build camera (bhr_raymap_render)
  hybrid      bhr_render orbit frames, hybrid arithmetic      } the code of the commit before the orbit map:
  strict      bhr_render orbit frames, strict arithmetic      } the baseline
Per leg and round, from the timing ring of those frames: the mean march bracket (for a map frame: shade + overflow re-march), the
mean post-pass bracket, and the frame time as the span from the first frame's start to the last frame's end over the number of
frames (two frames in flight overlap), beside the host clock ending in a sync.

usage: python tools/orbit_map_timing.py [--frames 200] [--reps 3] [--orbit_frames 3600] [--out profiles/orbit_map_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("orbit_map", "static_map", "hybrid", "strict")


def frame(r, wl, leg, pos):
    flare = bool(wl.get("lens_flare", False))
    if leg == "orbit_map":
        r.render_from_ray_map_async(t_offset=0.0, lens_flare=flare, cam_pos=pos, fov=wl["fov"])
    elif leg == "static_map":
        r.render_from_ray_map_async(t_offset=0.0, lens_flare=flare)
    else:
        r.render_async(pos, wl["fov"], math=leg, lens_flare=flare)


def time_leg(r, wl, leg, positions, start, frames):
    n_pos = len(positions)
    for i in range(16):
        frame(r, wl, leg, positions[(start + i) % n_pos])
    r.sync()
    r.timing_reset()
    t0 = time.perf_counter()
    for i in range(frames):
        frame(r, wl, leg, positions[(start + 16 + i) % n_pos])
    r.sync()
    host_ms = (time.perf_counter() - t0) / frames * 1e3
    c = r.counters()
    n = int(c["frames_timed"])
    return {"frames": n, "first_position": (start + 16) % n_pos, "march_ms": c["march_ms_sum"] / n, "post_ms": c["bloom_ms_sum"] / n,
            "frame_ms": c["span_ms"] / n, "host_ms": host_ms, "ray_steps_per_frame": int(c["ray_steps_sum"]) // n}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--orbit_frames", type=int, default=3600, help="positions on the full circle (BASELINE configs[4]: 3600)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbit_map_timing.json"))
    args = ap.parse_args()
    if not (1 <= args.frames <= 500):
        ap.error("--frames: 1 .. 500 (the timing ring holds 510 frames)")
    import bench
    from bhr_amd import workloads
    from bhr_amd.camera import orbit_position
    wl = bench.WORKLOADS["fhd"]
    if wl["disk_tilt"] != 0:
        ap.error("the fhd workload's disk is tilted: an orbit map needs --disk_tilt 0")
    positions = [[float(v) for v in orbit_position(wl["cam_pos"], f, args.orbit_frames)] for f in range(args.orbit_frames)]
    r, _, _, note = workloads.make_scene(wl, math="hybrid", frame_slots=2)
    res = {"method": f"one hybrid context, two frames in flight; legs {LEGS} alternating in one process, {args.frames} frames each after 16 "
                     f"warm-up frames, {args.reps} rounds; the camera steps round a {args.orbit_frames}-position orbit; brackets from the "
                     f"timing ring, frame_ms = span / frames",
           "scene": note, "width": wl["width"], "height": wl["height"], "anti_alias": wl["anti_alias"], "disk_tilt": wl["disk_tilt"],
           "lens_flare": bool(wl.get("lens_flare", False)), "legs": {leg: [] for leg in LEGS}}
    try:
        t_spin = time.perf_counter()                              # clocks up, slot streams calibrated
        while time.perf_counter() - t_spin < 0.5:
            for _ in range(8):
                r.render_async(wl["cam_pos"], wl["fov"])
            r.sync()
        builds = []
        for _ in range(3):                                        # the first build allocates, the later ones reuse
            t0 = time.perf_counter()
            r.build_ray_map(positions[0], wl["fov"])
            builds.append((time.perf_counter() - t0) * 1e3)
        info = r.ray_map_info()
        res.update(build_ms=builds, slots=info["slots"], diff=info["diff"], device_bytes=info["device_bytes"],
                   build_ray_steps=info["ray_steps"], overflow_pixels=info["overflow_pixels"])
        start = 0
        for _ in range(args.reps):
            for leg in LEGS:
                res["legs"][leg].append(time_leg(r, wl, leg, positions, start, args.frames))
            start += args.frames + 16                             # every round a fresh stretch of the orbit, the same for its four legs
    finally:
        r.close()
    print(f"fhd: build {min(res['build_ms']):.3f} ms, K={res['slots']}, overflow {res['overflow_pixels']} px, {res['device_bytes'] / 1e6:.0f} MB", flush=True)
    for leg in LEGS:
        rows = res["legs"][leg]
        print(f"  {leg:10s} march ms " + " ".join(f"{x['march_ms']:7.3f}" for x in rows) + "   frame ms " +
              " ".join(f"{x['frame_ms']:7.3f}" for x in rows) + "   host ms " + " ".join(f"{x['host_ms']:7.3f}" for x in rows), flush=True)
    mean = {leg: sum(x["frame_ms"] for x in res["legs"][leg]) / len(res["legs"][leg]) for leg in LEGS}
    res["mean_frame_ms"] = mean
    res["orbit_map_over_hybrid"] = mean["orbit_map"] / mean["hybrid"]
    res["orbit_map_over_static_map"] = mean["orbit_map"] / mean["static_map"]
    print(f"  orbit_map / hybrid {res['orbit_map_over_hybrid']:.3f}, orbit_map / static_map {res['orbit_map_over_static_map']:.3f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0 if mean["orbit_map"] < mean["hybrid"] else 1


if __name__ == "__main__":
    sys.exit(main())
