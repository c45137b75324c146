#!/usr/bin/env python
"""Kerr polarisation: what the Kerr Stokes pass costs a frame from the Kerr ray map, and what the momentum planes cost its build
("Kerr polarisation").

The fhd bench scene (bench.WORKLOADS["fhd"]) around a hole of spin A = 0.9, once per redshift mode, on one context with one frame
slot (every kernel alone on its stream, so the brackets are kernel times).  The map is built under the polarisation, so both legs
shade the same map.  Legs alternate in one process, --frames frames each after a warm-up, the round repeated --reps times:
  off   frames from the Kerr map, no polarisation: the kernels of the commit before it (profiles/kerr_polar_code_objects.txt)
  on    the same frames with a toroidal field set: the Kerr Stokes kernel and the cell reduction behind the shade and fix launches
The timing ring brackets a frame as march (the shade launch and the fix launch over the overflow list: the yardstick) and post
(march end to frame end: bloom H, V + combine -- and, with the polarisation set, the Stokes pass, which is launched behind the
march bracket).  stokes_ms = post_ms(on) - post_ms(off) of the means; stokes_over_shade = stokes_ms / march_ms(off).
The build: host time around build_kerr_ray_map (it synchronises), --builds builds each with and without the polarisation set,
alternating; the map's device bytes either way.

usage: python tools/kerr_stokes_timing.py [--frames 200] [--reps 3] [--builds 5] [--out profiles/kerr_stokes_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPIN = 0.9


def time_leg(r, frames):
    for _ in range(16):
        r.render_from_kerr_ray_map_async(t_offset=0.0)
    r.sync()
    r.timing_reset()
    t0 = time.perf_counter()
    for _ in range(frames):
        r.render_from_kerr_ray_map_async(t_offset=0.0)
    r.sync()
    host_ms = (time.perf_counter() - t0) / frames * 1e3
    c = r.counters()
    n = int(c["frames_timed"])
    return {"frames": n, "march_ms": c["march_ms_sum"] / n, "post_ms": c["bloom_ms_sum"] / n, "frame_ms": c["span_ms"] / n, "host_ms": host_ms}


def time_build(r, wl):
    t0 = time.perf_counter()
    r.build_kerr_ray_map(wl["cam_pos"], wl["fov"])
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kerr_stokes_timing.json"))
    args = ap.parse_args()
    if not (1 <= args.frames <= 500):
        ap.error("--frames: 1 .. 500 (the timing ring holds 510 frames)")
    import bench
    from bhr_amd import workloads
    wl = dict(bench.WORKLOADS["fhd"])
    res = {"method": f"fhd scene, spin {SPIN}, one strict context with one frame slot per redshift mode; legs off / on alternating in one process, "
                     f"{args.frames} frames each after 16 warm-up frames, {args.reps} rounds; march_ms = the shade + fix bracket, post_ms = march "
                     f"end to frame end (holds the Stokes pass); stokes_ms = post_ms(on) - post_ms(off); builds: host ms around the "
                     f"synchronising build, {args.builds} each with and without the momentum planes, alternating",
           "width": wl["width"], "height": wl["height"], "spin": SPIN, "modes": {}}
    for mode in ("model", "exact"):
        r, _, _, note = workloads.make_scene(wl, math="strict", frame_slots=1)
        legs = {"off": [], "on": []}
        builds = {"plain": [], "momentum": []}
        try:
            r.set_spin(SPIN)
            r.set_redshift(mode)
            t_spin = time.perf_counter()                              # clocks up
            while time.perf_counter() - t_spin < 0.5:
                for _ in range(4):
                    r.render_async(wl["cam_pos"], wl["fov"])
                r.sync()
            size = {}
            for _ in range(args.builds):
                for kind in builds:
                    r.set_kerr_polarization("toroidal" if kind == "momentum" else None)
                    builds[kind].append(time_build(r, wl))
                    size[kind] = r.kerr_ray_map_info()["device_bytes"]
            info = r.kerr_ray_map_info()                              # (the last build kept the momenta)
            out = dict(scene=note, map_slots=info["slots"], overflow_pixels=info["overflow_pixels"], map_bytes=size,
                       resources=r.kerr_stokes_resources(mode))
            for _ in range(args.reps):
                for leg in legs:
                    r.set_kerr_polarization("toroidal" if leg == "on" else None)
                    legs[leg].append(time_leg(r, args.frames))
            r.set_kerr_polarization(None)
        finally:
            r.close()
        mean = {leg: {k: sum(x[k] for x in rows) / len(rows) for k in ("march_ms", "post_ms", "frame_ms", "host_ms")} for leg, rows in legs.items()}
        out.update(legs=legs, mean=mean, builds_ms=builds)
        out["build_ms"] = {k: sorted(v)[len(v) // 2] for k, v in builds.items()}
        out["stokes_ms"] = mean["on"]["post_ms"] - mean["off"]["post_ms"]
        out["shade_ms"] = mean["off"]["march_ms"]
        out["stokes_over_shade"] = out["stokes_ms"] / out["shade_ms"]
        print(f"{mode}: Kerr Stokes kernel {out['resources']}, overflow {out['overflow_pixels']} px, map bytes {size}", flush=True)
        for leg, rows in legs.items():
            print(f"  {leg:4s} march ms " + " ".join(f"{x['march_ms']:7.4f}" for x in rows) + "   post ms " + " ".join(f"{x['post_ms']:7.4f}" for x in rows) +
                  "   frame ms " + " ".join(f"{x['frame_ms']:7.4f}" for x in rows), flush=True)
        print(f"  build ms: plain " + " ".join(f"{v:.2f}" for v in builds["plain"]) + "   with momenta " + " ".join(f"{v:.2f}" for v in builds["momentum"]), flush=True)
        print(f"  Stokes pass {out['stokes_ms']:.4f} ms, shade bracket {out['shade_ms']:.4f} ms: {out['stokes_over_shade']:.2f} of it", flush=True)
        res["modes"][mode] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
