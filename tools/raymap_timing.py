#!/usr/bin/env python
"""Ray map: what a frame shaded from the map costs against a marched frame ("Ray map").

Two views: the fhd bench scene and the 4k tilt-25 anti-aliased one (bench.WORKLOADS), each on ONE hybrid context with two frames
in flight.  Per view: the build (host clock around bhr_raymap_build, which synchronises), then three legs -- frames from the
map, strict bhr_render frames, hybrid bhr_render frames -- alternating in this process, --frames frames each after a warm-up,
the round of three legs repeated --reps times to show the spread.  Per leg and round, from the timing ring of those frames:
the mean march bracket (for a map frame: shade + overflow re-march), the mean post-pass bracket, and the frame time as the
span from the first frame's start to the last frame's end over the number of frames (two frames in flight overlap), beside
the host clock ending in a sync.  Also: overflow pixels and crossings per pixel at the default slot count, and the share of
pixels with more than K crossings for K = 1..8 (from the map's CROSSINGS plane).

usage: python tools/raymap_timing.py [--frames 200] [--reps 3] [--views fhd,4k] [--out profiles/raymap_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("map", "strict", "hybrid")


def frame(r, wl, leg):
    flare = bool(wl.get("lens_flare", False))
    if leg == "map":
        r.render_from_ray_map_async(t_offset=0.0, lens_flare=flare)
    else:
        r.render_async(wl["cam_pos"], wl["fov"], math=leg, lens_flare=flare)


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


def crossings_plane(r):
    from bhr_amd import _lib
    out = np.empty((r.height, r.width), dtype=np.int32)
    _lib.check(r._lib.bhr_raymap_read(r._ctx, _lib.RAYMAP_CROSSINGS, out.ctypes.data, out.nbytes))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--views", default="fhd,4k")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raymap_timing.json"))
    args = ap.parse_args()
    if not (1 <= args.frames <= 500):
        ap.error("--frames: 1 .. 500 (the timing ring holds 510 frames)")
    import bench
    from bhr_amd import workloads
    res = {"method": f"one hybrid context per view, two frames in flight; legs {LEGS} alternating in one process, {args.frames} frames each "
                     f"after 16 warm-up frames, {args.reps} rounds; brackets from the timing ring, frame_ms = span / frames",
           "views": {}}
    for name in args.views.split(","):
        wl = bench.WORKLOADS[name]
        r, _, _, note = workloads.make_scene(wl, math="hybrid", frame_slots=2)
        view = {"scene": note, "width": wl["width"], "height": wl["height"], "anti_alias": wl["anti_alias"], "disk_tilt": wl["disk_tilt"],
                "lens_flare": bool(wl.get("lens_flare", False)), "legs": {leg: [] for leg in LEGS}}
        try:
            t_spin = time.perf_counter()                          # clocks up, slot streams calibrated
            while time.perf_counter() - t_spin < 0.5:
                for _ in range(8):
                    r.render_async(wl["cam_pos"], wl["fov"])
                r.sync()
            builds = []
            for _ in range(3):                                    # the first build allocates, the later ones reuse
                t0 = time.perf_counter()
                r.build_ray_map(wl["cam_pos"], wl["fov"])
                builds.append((time.perf_counter() - t0) * 1e3)
            info = r.ray_map_info()
            cr = crossings_plane(r)
            px = cr.size
            view.update(build_ms=builds, slots=info["slots"], diff=info["diff"], device_bytes=info["device_bytes"],
                        build_ray_steps=info["ray_steps"], overflow_pixels=info["overflow_pixels"],
                        overflow_share=info["overflow_pixels"] / px, crossings_per_pixel=float(cr.mean()),
                        crossings_stored_per_pixel=info["crossings_stored"] / px, max_crossings=int(cr.max()),
                        share_above_k={str(k): float((cr > k).mean()) for k in range(1, 9)})
            for _ in range(args.reps):
                for leg in LEGS:
                    view["legs"][leg].append(time_leg(r, wl, leg, args.frames))
        finally:
            r.close()
        res["views"][name] = view
        print(f"{name}: build {min(view['build_ms']):.3f} ms, K={view['slots']}, overflow {view['overflow_pixels']} px "
              f"({100 * view['overflow_share']:.4f} %), {view['crossings_per_pixel']:.3f} crossings / pixel, {view['device_bytes'] / 1e6:.0f} MB", flush=True)
        for leg in LEGS:
            rows = view["legs"][leg]
            print(f"  {leg:7s} march ms " + " ".join(f"{x['march_ms']:7.3f}" for x in rows) + "   frame ms " +
                  " ".join(f"{x['frame_ms']:7.3f}" for x in rows) + "   host ms " + " ".join(f"{x['host_ms']:7.3f}" for x in rows), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
