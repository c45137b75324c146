#!/usr/bin/env python
"""Kerr point stars: what the star plane costs a frame from the Kerr ray map ("Kerr point stars").

tools/stars_timing.py's protocol over the Kerr map.  The fhd bench scene (bench.WORKLOADS["fhd"], pov (6, 0, 0.5)) around the hole
of --spin (default 0.9) under --redshift (default model), and the same scene at 3840 x 2160, each on ONE hybrid context with two
frames in flight.  The camera goes round the video driver's orbit about the spin axis; the map is built once for position 0.  Per
size, legs alternate in one process, --frames frames each after a warm-up, the round repeated --reps times:
  orbit_map        orbit frames from the turned Kerr map, no catalogue: the kernels of the commit before Kerr point stars
                   (profiles/kerr_stars_code_objects.txt) -- the baseline, re-measured here on the same card
  static_map       frames from the map at the build camera, no catalogue
  orbit_stars_N    orbit frames with a Kerr catalogue of N stars: the gather of the turned view and the STARS shade, every frame
  static_stars_N   frames at the build camera with it: the cached plane, the STARS shade only
for N = 6000 (the procedural sky's own stars) and 100 000 (uniform on the sphere).  frame_ms is the span from the first
frame's start to the last frame's end over the number of frames (two frames in flight overlap): what a video pays per frame.
The gather alone is not bracketed by events (it runs ahead of the frame's march bracket, on the frame's stream); it is reported
as  gather_ms = (orbit_stars_N - static_stars_N) - (orbit_map - static_map)  of the mean frame times: what the turned view adds
with a catalogue beyond what it adds without one.  The STARS shade kernels' registers, LDS and scratch come from
bhr_kerr_stars_resources, the gather kernel's from bhr_stars_resources.

usage: python tools/kerr_stars_timing.py [--frames 200] [--reps 3] [--sizes fhd,4k] [--spin 0.9] [--redshift model]
                                         [--out profiles/kerr_stars_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"fhd": (1920, 1080), "4k": (3840, 2160)}
COUNTS = (6000, 100000)


def catalog(r, wl, n):
    import numpy as np
    from bhr_amd import skybox, stars
    cam = r.camera_uniforms(wl["cam_pos"], wl["fov"], 0)
    omega = float(cam.pixel_width) * float(cam.pixel_height)
    if n == 6000:
        return stars.catalog_from_tables(skybox.sky_tables(2048, 1024, 42, 6000), stars.DEFAULT_STAR_GAIN, omega)
    rng = np.random.default_rng(5)
    z, phi = rng.uniform(-1, 1, n), rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(1 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=-1), rng.uniform(0.05, 1.0, (n, 3)) * stars.DEFAULT_STAR_GAIN * omega


def frame(r, turned, pos):
    if turned:
        r.render_from_kerr_ray_map_async(t_offset=0.0, cam_pos=pos)
    else:
        r.render_from_kerr_ray_map_async(t_offset=0.0)


def time_leg(r, turned, positions, start, frames):
    n_pos = len(positions)
    for i in range(16):
        frame(r, turned, positions[(start + i) % n_pos])
    r.sync()
    r.timing_reset()
    t0 = time.perf_counter()
    for i in range(frames):
        frame(r, turned, positions[(start + 16 + i) % n_pos])
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
    ap.add_argument("--spin", type=float, default=0.9)
    ap.add_argument("--redshift", default="model", choices=["model", "exact"])
    ap.add_argument("--orbit_frames", type=int, default=3600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kerr_stars_timing.json"))
    args = ap.parse_args()
    if not (1 <= args.frames <= 500):
        ap.error("--frames: 1 .. 500 (the timing ring holds 510 frames)")
    sizes = args.sizes.split(",")
    if any(s not in SIZES for s in sizes):
        ap.error(f"--sizes: a comma-separated list of {sorted(SIZES)}")
    import bench
    from bhr_amd import workloads
    from bhr_amd.camera import orbit_position
    base = bench.WORKLOADS["fhd"]
    if base["disk_tilt"] != 0:
        ap.error("the fhd workload's disk is tilted: a spinning hole's disk is not")
    res = {"method": f"per size one hybrid context with spin {args.spin:g} and the {args.redshift} redshift, two frames in flight; legs alternating in one "
                     f"process, {args.frames} frames each after 16 warm-up frames, {args.reps} rounds; the camera steps round a "
                     f"{args.orbit_frames}-position orbit; frame_ms = span of the timing ring / frames; gather_ms = (orbit_stars - static_stars) - "
                     f"(orbit_map - static_map) of the means",
           "spin": args.spin, "redshift": args.redshift, "sizes": {}}
    for size in sizes:
        W, H = SIZES[size]
        wl = dict(base, width=W, height=H)
        positions = [[float(v) for v in orbit_position(wl["cam_pos"], f, args.orbit_frames)] for f in range(args.orbit_frames)]
        r, _, _, note = workloads.make_scene(wl, math="hybrid", frame_slots=2)
        r.set_spin(args.spin)
        r.set_redshift(args.redshift)
        legs = {"orbit_map": (0, True), "static_map": (0, False)}
        for n in COUNTS:
            legs[f"orbit_stars_{n}"] = (n, True)
            legs[f"static_stars_{n}"] = (n, False)
        out = {"scene": note, "width": W, "height": H, "cam_pos": wl["cam_pos"], "legs": {leg: [] for leg in legs}, "stars_info": {}}
        try:
            t_spin = time.perf_counter()                              # clocks up, slot streams calibrated
            while time.perf_counter() - t_spin < 0.5:
                for _ in range(8):
                    r.render_async(wl["cam_pos"], wl["fov"])
                r.sync()
            r.build_kerr_ray_map(positions[0], wl["fov"])
            info = r.kerr_ray_map_info()
            out.update(slots=info["slots"], overflow_pixels=info["overflow_pixels"],
                       resources={"shade_stars": r.kerr_stars_resources(args.redshift), "shade_stars_turned": r.kerr_stars_resources(args.redshift, True),
                                  "gather": r.stars_resources(), "gather_turned": r.stars_resources(True)})
            cats = {n: catalog(r, wl, n) for n in COUNTS}
            start = 0
            for _ in range(args.reps):
                have = None
                for leg, (n, turned) in legs.items():
                    if n != have:
                        if n:
                            r.set_kerr_stars(*cats[n])
                        else:
                            r.clear_kerr_stars()
                        have = n
                    out["legs"][leg].append(time_leg(r, turned, positions, start, args.frames))
                    if n and turned:
                        out["stars_info"][str(n)] = r.kerr_stars_info()
                start += args.frames + 16
            r.clear_kerr_stars()
        finally:
            r.close()
        mean = {leg: sum(x["frame_ms"] for x in rows) / len(rows) for leg, rows in out["legs"].items()}
        out["mean_frame_ms"] = mean
        out["gather_ms"] = {str(n): (mean[f"orbit_stars_{n}"] - mean[f"static_stars_{n}"]) - (mean["orbit_map"] - mean["static_map"]) for n in COUNTS}
        out["orbit_stars_over_orbit_map"] = {str(n): mean[f"orbit_stars_{n}"] / mean["orbit_map"] for n in COUNTS}
        out["static_stars_over_static_map"] = {str(n): mean[f"static_stars_{n}"] / mean["static_map"] for n in COUNTS}
        res["sizes"][size] = out
        print(f"{size}: overflow {out['overflow_pixels']} px, kernels {out['resources']}", flush=True)
        for leg, rows in out["legs"].items():
            print(f"  {leg:20s} frame ms " + " ".join(f"{x['frame_ms']:7.3f}" for x in rows) + "   march ms " +
                  " ".join(f"{x['march_ms']:7.3f}" for x in rows) + "   host ms " + " ".join(f"{x['host_ms']:7.3f}" for x in rows), flush=True)
        print("  gather ms " + ", ".join(f"{n}: {v:.3f}" for n, v in out["gather_ms"].items()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
