"""The Kerr camera's march time at A = 0.9, pov (3, 2, 0): ms per frame of {the pinhole at rest, the circular camera, the full-sphere
equirect panorama} x {model, exact redshift} next to the Kerr march of the same view -- whose code object is the parent commit's byte
for byte (profiles/kerr_observer_code_objects.txt), so the same run measures both -- on one context per frame size, one frame slot
(isolated launches), three runs of each alternating, with the kernels' registers, LDS and scratch.  The pinhole frames are fhd
(1920 x 1080), the panorama is the 4k resolution's frame under --spin_projection equirect (3840 x 1920).
usage: tools/kerr_observer_measure.py [OUT.json]   (DESIGN 4 "Kerr camera")"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bhr_amd import HipRenderer, observer, scenes
from bhr_amd.textures import compute_disk_texture_resolution

A, POV, FOV, RUNS, FRAMES = 0.9, [3.0, 2.0, 0.0], 90, 3, 10
CIRCULAR = tuple(float(v) for v in observer.kerr_velocity("circular", POV, A))
SIZES = {"fhd": (1920, 1080), "equirect_4k": (3840, 1920)}
runs = {"fhd": (("kerr_march", {}), ("view_rest_pinhole", dict(kerr_observer=(0.0, 0.0, 0.0))), ("view_circular", dict(kerr_observer=CIRCULAR))),
        "equirect_4k": (("view_equirect_360x180", dict(kerr_projection="equirect")),)}
res = {"how": f"A = {A}, pov {POV}, step 0.1, one frame slot; {RUNS} runs of {FRAMES} frames each after a warm-up run, the variants alternating; "
              "march_ms: the median of the runs' means, with every run's mean; kerr_march is bhr_render's Kerr frame, the parent's code object",
       "circular_beta": CIRCULAR}
for size, (W, H) in SIZES.items():
    n_phi, n_r = compute_disk_texture_resolution(W, H, POV, FOV, 2.0, 15.0)
    r = HipRenderer(W, H, scenes.analytic_skybox(1024, 2048), scenes.noisy_disk(n_r, n_phi), step_size=0.1, math="strict", frame_slots=1, spin=A)
    res.setdefault("resources", {"kerr": r.kerr_resources(), **{f"view_{'exact' if e else 'model'}{'_ss' if s else ''}": r.kerr_view_resources(e, s)
                                                                   for e in (False, True) for s in (False, True)}})
    for redshift in ("model", "exact"):
        r.set_redshift(redshift)
        ms, steps = {name: [] for name, _ in runs[size]}, {}
        for run in range(RUNS + 1):                     # run 0 warms up: code objects, clocks
            for name, kw in runs[size]:
                r.timing_reset()
                for _ in range(FRAMES):
                    r.render_async(POV, FOV, skip_bloom=True, **kw)
                c = r.counters()
                steps[name] = int(c["ray_steps"])
                if run:
                    ms[name].append(c["march_ms_sum"] / c["frames_timed"])
        for name, _ in runs[size]:
            res[f"{name}_{redshift}"] = dict(size=[W, H], march_ms=round(statistics.median(ms[name]), 4), runs_ms=[round(m, 4) for m in ms[name]],
                                             ray_steps=steps[name], ns_per_step=round(statistics.median(ms[name]) * 1e6 / steps[name], 6))
    r.set_redshift("model")
    r.close()
for redshift in ("model", "exact"):
    base = res[f"kerr_march_{redshift}"]
    res[f"view_rest_pinhole_{redshift}"]["ratio_to_kerr_march"] = round(res[f"view_rest_pinhole_{redshift}"]["march_ms"] / base["march_ms"], 4)
    base["spread_of_runs"] = round(max(base["runs_ms"]) / min(base["runs_ms"]), 4)
print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
