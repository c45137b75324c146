#!/usr/bin/env python
"""Motion blur: what a shutter frame of n samples costs ("Motion blur").

The fhd bench scene (bench.WORKLOADS), hybrid, two frames in flight.  Legs: a plain frame, and a shutter frame of n samples
for n in 2, 4, 8, 16 on a 10 degree orbit arc.  Every leg is timed twice, the two passes over all legs interleaved, >=
--seconds of frames each on the host clock, ending in a sync.  Beside it, from one isolated frame per leg (nothing else in
flight): the frame's march bracket (bhr_counters.march_ms: first sample's start to behind the last accumulation), n times the
plain frame's march bracket of the same run, and the accumulation launches' own time -- the sum of the HIP-event brackets
the option "shutter_timing" puts around each of them -- with the bytes they move (first launch 16 B per float of a layer
pair, every later one 24 B) over that time.

usage: python tools/shutter_cost.py [--seconds 1.0] [--out profiles/shutter.json]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLES = (2, 4, 8, 16)


def samples(wl, n):
    x, y, z = wl["cam_pos"]
    pos = []
    for j in range(n):
        a = math.radians(10.0) * (j + 0.5) / n
        pos.append([x * math.cos(a) - y * math.sin(a), x * math.sin(a) + y * math.cos(a), z])
    return pos, [0.05 * ((j + 0.5) / n - 0.5) for j in range(n)]


def frame(r, wl, n):
    if n == 0:
        r.render_async(wl["cam_pos"], wl["fov"])
    else:
        pos, toff = samples(wl, n)
        r.render_shutter_async(pos, wl["fov"], toff)


def time_leg(r, wl, n, seconds):
    """ms per frame over >= `seconds` of frames, two frames in flight, host clock ending in a sync."""
    for _ in range(4):
        frame(r, wl, n)
    r.sync()
    count, t0 = 0, time.perf_counter()
    while True:
        for _ in range(8):
            frame(r, wl, n)
        count += 8
        if time.perf_counter() - t0 >= seconds:
            break
    r.sync()
    return (time.perf_counter() - t0) / count * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shutter.json"))
    args = ap.parse_args()
    import bench
    from bhr_amd import workloads
    wl = bench.WORKLOADS["fhd"]
    r, _, _, note = workloads.make_scene(wl, math="hybrid", frame_slots=2)
    floats = wl["width"] * wl["height"] * 3
    res = {"method": "fhd bench scene, hybrid, two frames in flight, host clock ending in a sync, every leg twice (two interleaved "
                     f"passes), >= {args.seconds} s per leg; march brackets and accumulation times from one isolated frame per leg",
           "scene": note, "width": wl["width"], "height": wl["height"], "legs": {}}
    try:
        t_spin = time.perf_counter()                          # clocks up, slot streams calibrated
        while time.perf_counter() - t_spin < 0.5:
            for _ in range(8):
                r.render_async(wl["cam_pos"], wl["fov"])
            r.sync()
        for rep in range(2):
            for n in (0,) + SAMPLES:
                leg = res["legs"].setdefault("plain" if n == 0 else f"n={n}", {"samples": n, "frame_ms": []})
                r.set_option("shutter_timing", 0)
                leg["frame_ms"].append(time_leg(r, wl, n, args.seconds))
                if rep:
                    continue
                r.sync()
                r.set_option("shutter_timing", 1)              # one isolated frame: its march bracket and its accumulation launches
                frame(r, wl, n)
                c = r.counters()
                leg["march_ms_isolated"], leg["post_ms_isolated"] = c["march_ms"], c["bloom_ms"]
                leg["rays"], leg["ray_steps"] = int(c["rays"]), int(c["ray_steps"])
                if n:
                    t = r.shutter_timing()
                    nbytes = floats * (16 + 24 * (n - 1))        # per float of the two layers: read + write, then two reads + write
                    leg.update(accumulate_launches=t["launches"], accumulate_ms=t["ms"], accumulate_bytes=nbytes,
                               accumulate_gb_per_s=nbytes / (t["ms"] * 1e-3) / 1e9 if t["ms"] > 0 else None)
        plain = res["legs"]["plain"]
        for n in SAMPLES:
            leg = res["legs"][f"n={n}"]
            leg["n_x_plain_march_ms"] = n * plain["march_ms_isolated"]
            leg["n_x_plain_frame_ms"] = [n * v for v in plain["frame_ms"]]
    finally:
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for lab, leg in res["legs"].items():
        print(f"{lab:6s} frame ms {leg['frame_ms'][0]:7.3f} {leg['frame_ms'][-1]:7.3f}  march (isolated) {leg['march_ms_isolated']:7.3f}  "
              f"n x plain march {leg.get('n_x_plain_march_ms', float('nan')):7.3f}  accumulate {leg.get('accumulate_ms', float('nan')):7.4f} ms "
              f"in {leg.get('accumulate_launches', 0)} launches", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
