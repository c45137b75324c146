#!/usr/bin/env python
"""Grading: what the stage costs a frame ("Grading").

The fhd bench scene (bench.WORKLOADS), hybrid, two frames in flight.  Legs: a plain frame, the clip identity (clip, 0 stops,
linear), aces + srgb at +1 stop, and the same with keep_hdr; every leg with outputs "f32" and "u8".  Every leg is timed twice,
the two passes over all legs interleaved, >= --seconds of frames each on the host clock, ending in a sync.  Beside it, from
one isolated frame per leg (nothing else in flight): the grade launches' own time -- the HIP-event brackets the option
"grade_timing" puts around them -- with the bytes they move computed from the shapes (per value 12 B of layers read and 4 B
of FINAL written, 4 B more for the HDR plane, 1 B more for the u8 rows) over that time, and the frame's post-pass bracket
(bhr_counters.bloom_ms: end of the march to the end of the frame).

usage: python tools/grade_cost.py [--seconds 1.0] [--out profiles/grade.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRADES = (("plain", None),
          ("clip identity", dict(tonemap="clip")),
          ("aces+srgb", dict(tonemap="aces", exposure=1.0, transfer="srgb")),
          ("aces+srgb+hdr", dict(tonemap="aces", exposure=1.0, transfer="srgb", keep_hdr=True)))
OUTPUTS = ("f32", "u8")


def time_leg(r, wl, seconds):
    """ms per frame over >= `seconds` of frames, two frames in flight, host clock ending in a sync."""
    for _ in range(4):
        r.render_async(wl["cam_pos"], wl["fov"])
    r.sync()
    count, t0 = 0, time.perf_counter()
    while True:
        for _ in range(8):
            r.render_async(wl["cam_pos"], wl["fov"])
        count += 8
        if time.perf_counter() - t0 >= seconds:
            break
    r.sync()
    return (time.perf_counter() - t0) / count * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grade.json"))
    args = ap.parse_args()
    import bench
    from bhr_amd import workloads
    wl = bench.WORKLOADS["fhd"]
    r, _, _, note = workloads.make_scene(wl, math="hybrid", frame_slots=2)
    values = wl["width"] * wl["height"] * 3
    res = {"method": "fhd bench scene, hybrid, two frames in flight, host clock ending in a sync, every leg twice (two interleaved "
                     f"passes), >= {args.seconds} s per leg; grade launch times and post-pass brackets from one isolated frame per leg",
           "scene": note, "width": wl["width"], "height": wl["height"], "legs": {}}
    try:
        t_spin = time.perf_counter()                          # clocks up, slot streams calibrated
        while time.perf_counter() - t_spin < 0.5:
            for _ in range(8):
                r.render_async(wl["cam_pos"], wl["fov"])
            r.sync()
        for rep in range(2):
            for outputs in OUTPUTS:
                r.set_outputs(outputs)
                for name, grade in GRADES:
                    leg = res["legs"].setdefault(f"{name} / {outputs}", {"grade": grade, "outputs": outputs, "frame_ms": []})
                    r.set_grade(**(grade or {}))
                    r.set_option("grade_timing", 0)
                    leg["frame_ms"].append(time_leg(r, wl, args.seconds))
                    if rep:
                        continue
                    r.sync()
                    r.set_option("grade_timing", 1)             # one isolated frame: its grade launches and its post-pass bracket
                    r.render_async(wl["cam_pos"], wl["fov"])
                    c = r.counters()
                    leg["march_ms_isolated"], leg["post_ms_isolated"] = c["march_ms"], c["bloom_ms"]
                    if grade:
                        t = r.grade_timing()
                        per_value = 12 + 4 + (4 if grade.get("keep_hdr") else 0) + (1 if outputs == "u8" else 0)
                        leg.update(grade_launches=t["launches"], grade_ms=t["ms"], grade_bytes=values * per_value,
                                   grade_gb_per_s=values * per_value / (t["ms"] * 1e-3) / 1e9 if t["ms"] > 0 else None)
        r.set_grade(None)
    finally:
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for lab, leg in res["legs"].items():
        print(f"{lab:22s} frame ms {leg['frame_ms'][0]:7.3f} {leg['frame_ms'][-1]:7.3f}  post-pass (isolated) {leg['post_ms_isolated']:7.3f}  "
              f"grade {leg.get('grade_ms', float('nan')):7.4f} ms, {leg.get('grade_bytes', 0) / 1e6:5.1f} MB, "
              f"{leg.get('grade_gb_per_s') or float('nan'):6.0f} GB/s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
