"""1920 x 960, default view: march time per ray-step of the projected kernel (full-sphere equirect, and the fisheye dome on the
same frame) next to the observer kernel at rest at the same frame size in the same run -- one context, one frame slot (isolated
launches), the runs alternating over several rounds, medians and the rounds' spread -- with the kernels' registers, LDS and
scratch.  The loops are the same code, but a ray's cost outside the loop (set-up, shading passes, the sky sample, the stores) is
spread over fewer steps where rays are short: the observer kernel is therefore also timed on wider pinhole views of the same
size, whose rays are as short as the panorama's, so that time per step can be compared at equal steps per ray.
usage: tools/projection_measure.py [OUT.json]   (DESIGN 4 "Projections")"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bhr_amd import HipRenderer, scenes
from bhr_amd.textures import compute_disk_texture_resolution

W, H, POV, FOV, ROUNDS, FRAMES = 1920, 960, [6, 0, 0.5], 90, 7, 20
REST = (0.0, 0.0, 0.0)
n_phi, n_r = compute_disk_texture_resolution(W, H, POV, FOV, 2.0, 15.0)
sky, tex = scenes.analytic_skybox(1024, 2048), scenes.noisy_disk(n_r, n_phi)
r = HipRenderer(W, H, sky, tex, step_size=0.1, math="strict", frame_slots=1)
runs = (("observer_rest", dict(observer=REST)), ("equirect_360x180", dict(projection="equirect", observer=REST)),
        ("fisheye_180", dict(projection="fisheye", observer=REST)),
        ("observer_rest_fov130", dict(observer=REST, fov=130)), ("observer_rest_fov150", dict(observer=REST, fov=150)),
        ("observer_rest_fov165", dict(observer=REST, fov=165)))
ms, steps = {name: [] for name, _ in runs}, {}
for rnd in range(ROUNDS + 1):                       # round 0 warms up: code objects, clocks
    for name, kw in runs:
        r.timing_reset()
        for _ in range(FRAMES):
            r.render_async(POV, kw.get("fov", FOV), **{k: v for k, v in kw.items() if k != "fov"})
        c = r.counters()
        steps[name] = int(c["ray_steps"])
        if rnd:
            ms[name].append(c["march_ms_sum"] / c["frames_timed"])
res = {"how": f"{W}x{H}, pov {POV}, step 0.1, one frame slot; {ROUNDS} rounds of {FRAMES} frames each, the runs alternating; medians of the "
              "rounds' means, min and max over the rounds; the observer's frames are the pinhole camera's (fov 90 unless named) at the same size",
       "resources": {"observer": r.observer_resources(), "observer_ss": r.observer_resources(True),
                     "projected": r.projected_resources(), "projected_ss": r.projected_resources(True)}}
r.close()
for name, _ in runs:
    per = sorted(m * 1e6 / steps[name] for m in ms[name])          # ns per ray-step of each round
    m = statistics.median(ms[name])
    res[name] = dict(march_ms=round(m, 4), march_ms_min=round(min(ms[name]), 4), march_ms_max=round(max(ms[name]), 4), ray_steps=steps[name],
                     steps_per_pixel=round(steps[name] / (W * H), 2), ns_per_step=round(statistics.median(per), 6), ns_per_step_min=round(per[0], 6), ns_per_step_max=round(per[-1], 6))
for name in [n for n, _ in runs[1:]]:
    res[name]["time_per_step_ratio_to_observer"] = round(res[name]["ns_per_step"] / res["observer_rest"]["ns_per_step"], 4)
res["observer_rest"]["spread_of_rounds"] = round(res["observer_rest"]["ns_per_step_max"] / res["observer_rest"]["ns_per_step_min"], 4)
print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
