#!/usr/bin/env python
"""Adaptive supersampling: what a threshold costs and what it buys ("Adaptive supersampling").

The bench scene (bench.WORKLOADS: fhd default view; 4k, tilt 25, lod_radius), hybrid, two frames in flight.  Legs: k = 1;
for k in 2, 4: SSAA-k and adaptive k at every threshold of THRESHOLDS.  Every leg is timed twice, the two passes over all
legs interleaved (a drift of the machine shows as a spread between a leg's repeats), >= --seconds of frames each on the
host clock, ending in a sync.  Per leg: ms per frame, refined share, strict share of the refined, RMSE / max of FINAL against
the SSAA-k FINAL and against the k = 1 FINAL, and measured / model with model = t(k = 1) + share x t(SSAA-k).

usage: python tools/adaptive_supersample.py [--workloads fhd,4k] [--seconds 1.5] [--out profiles/adaptive_supersample.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THRESHOLDS = [-1.0, 0.0, 1 / 255, 2 / 255, 4 / 255, 8 / 255, 16 / 255, 32 / 255, float("inf")]
FACTORS = (2, 4)


def label(k, thr):
    if k == 1:
        return "k=1"
    if thr is None:
        return f"ssaa-{k}"
    if thr in (-1.0, 0.0) or thr == float("inf"):
        return f"adaptive-{k} T={thr:g}"
    return f"adaptive-{k} T={round(thr * 255)}/255"


def time_leg(r, wl, seconds):
    """ms per frame over >= `seconds` of frames, two frames in flight, host clock ending in a sync."""
    for _ in range(8):
        r.render_async(wl["cam_pos"], wl["fov"])
    r.sync()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(16):
            r.render_async(wl["cam_pos"], wl["fov"])
        n += 16
        if time.perf_counter() - t0 >= seconds:
            break
    r.sync()
    return (time.perf_counter() - t0) / n * 1e3


def run(name, wl, seconds):
    from bhr_amd import _lib, workloads
    r, _, _, note = workloads.make_scene(wl, math="hybrid", frame_slots=2)
    legs = [(1, None)] + [(k, t) for k in FACTORS for t in [None] + THRESHOLDS]
    out = {"workload": name, "scene": note, "width": wl["width"], "height": wl["height"], "legs": {}}
    try:
        t_spin = time.perf_counter()                      # clocks up, slot streams calibrated
        while time.perf_counter() - t_spin < 0.5:
            for _ in range(8):
                r.render_async(wl["cam_pos"], wl["fov"])
            r.sync()
        finals = {}
        for rep in range(2):
            for k, thr in legs:
                r.set_supersample(k, thr)
                ms = time_leg(r, wl, seconds)
                leg = out["legs"].setdefault(label(k, thr), {"k": k, "threshold": thr if thr is None or np.isfinite(thr) else "inf", "ms": []})
                leg["ms"].append(ms)
                if rep == 0:
                    finals[(k, thr)] = r.read_layer(_lib.LAYER_FINAL).astype(np.float64)
                    c = r.counters()
                    leg["rays"], leg["ray_steps"] = int(c["rays"]), int(c["ray_steps"])
                    if k > 1 and thr is not None:
                        a = r.adaptive_info()
                        leg["refined_share"] = a["refined"] / a["pixels"]
                        leg["strict_share_of_refined"] = a["strict"] / a["refined"] if a["refined"] else 0.0
        t1 = out["legs"]["k=1"]["ms"]
        for k, thr in legs:
            leg = out["legs"][label(k, thr)]
            if k == 1:
                continue
            for against, ref in (("ssaa", finals[(k, None)]), ("k1", finals[(1, None)])):
                d = finals[(k, thr)] - ref
                leg[f"rmse_vs_{against}"] = float(np.sqrt(np.mean(d * d)))
                leg[f"max_vs_{against}"] = float(np.abs(d).max())
            if thr is not None:
                tk = out["legs"][label(k, None)]["ms"]
                model = [a + leg["refined_share"] * b for a, b in zip(t1, tk)]
                leg["model_ms"] = model
                leg["measured_over_model"] = [m / q for m, q in zip(leg["ms"], model)]
        inf2 = out["legs"][label(2, float("inf"))]["ms"]
        # detect + empty refinement; the detect kernel's floor is 24 B per pixel read once at the HBM rate
        out["fixed_cost_ms"] = [a - b for a, b in zip(inf2, t1)]
        out["detect_floor_ms"] = wl["width"] * wl["height"] * 24 / 8.0e12 * 1e3
    finally:
        r.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="fhd,4k")
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_supersample.json"))
    args = ap.parse_args()
    import bench
    res = {"method": "hybrid, two frames in flight, host clock ending in a sync, every leg twice (two interleaved passes), "
                     f">= {args.seconds} s per leg; model = t(k=1) + refined share x t(SSAA-k)", "workloads": []}
    for name in args.workloads.split(","):
        wl = bench.WORKLOADS[name]
        res["workloads"].append(run(name, wl, args.seconds))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                    # after every workload: a long run leaves what it has
            json.dump(res, f, indent=1)
        for lab, leg in res["workloads"][-1]["legs"].items():
            print(f"{name:4s} {lab:24s} ms {leg['ms'][0]:8.3f} {leg['ms'][-1]:8.3f}  share {leg.get('refined_share', float('nan')):6.3f}  "
                  f"rmse vs ssaa {leg.get('rmse_vs_ssaa', float('nan')):9.2e}  meas/model {leg.get('measured_over_model', [float('nan')])[0]:5.2f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
