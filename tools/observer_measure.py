"""fhd default view: march time of the observer kernel at rest and on the circular orbit next to the strict march of the same view
in the same run -- one context, one frame slot (isolated launches), the three alternating over several rounds, medians -- with
the kernels' registers, LDS and scratch.
usage: tools/observer_measure.py [OUT.json]   (DESIGN 4 "Observer")"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bhr_amd import HipRenderer, observer, scenes
from bhr_amd.textures import compute_disk_texture_resolution

W, H, POV, FOV, ROUNDS, FRAMES = 1920, 1080, [6, 0, 0.5], 90, 7, 20
n_phi, n_r = compute_disk_texture_resolution(W, H, POV, FOV, 2.0, 15.0)
sky, tex = scenes.analytic_skybox(1024, 2048), scenes.noisy_disk(n_r, n_phi)
r = HipRenderer(W, H, sky, tex, step_size=0.1, math="strict", frame_slots=1)
runs = (("strict", None), ("observer_rest", (0.0, 0.0, 0.0)), ("observer_circular", tuple(float(v) for v in observer.velocity("circular", POV))))
ms, steps = {name: [] for name, _ in runs}, {}
for rnd in range(ROUNDS + 1):                       # round 0 warms up: code objects, clocks
    for name, beta in runs:
        kw = {} if beta is None else {"observer": beta}
        r.timing_reset()
        for _ in range(FRAMES):
            r.render_async(POV, FOV, **kw)
        c = r.counters()
        steps[name] = int(c["ray_steps"])
        if rnd:
            ms[name].append(c["march_ms_sum"] / c["frames_timed"])
res = {"how": f"fhd, pov {POV}, step 0.1, math strict, one frame slot; {ROUNDS} rounds of {FRAMES} frames each, the three alternating; medians of the rounds' means",
       "resources": {"strict": {"vgprs": r.counters()["march_vgprs"], "lds_bytes": r.counters()["march_lds_bytes"]},
                     "observer": r.observer_resources(), "observer_ss": r.observer_resources(True)}}
r.close()
for name, _ in runs:
    m = statistics.median(ms[name])
    res[name] = dict(march_ms=round(m, 4), march_ms_min=round(min(ms[name]), 4), march_ms_max=round(max(ms[name]), 4), ray_steps=steps[name],
                     ns_per_kilostep=round(m * 1e9 / steps[name], 4), gsteps_per_s=round(steps[name] / m / 1e6, 1))
for name in ("observer_rest", "observer_circular"):
    res[name]["march_ratio_to_strict"] = round(res[name]["march_ms"] / res["strict"]["march_ms"], 4)
    res[name]["time_per_step_ratio_to_strict"] = round(res[name]["ns_per_kilostep"] / res["strict"]["ns_per_kilostep"], 4)
print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
