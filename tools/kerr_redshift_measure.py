"""fhd default view: march time of the Kerr kernel under --redshift exact next to --redshift model, at A = 0.9 and A = -0.9 (the
retrograde disk has most of its hits inside the ISCO, on the plunge branch) and with --supersample 2, each on one frame slot
(isolated launches).  Model and exact alternate, REPEATS contexts of each, so that the spread between the repeats of one mode
stands next to the difference between the modes.  usage: tools/kerr_redshift_measure.py [OUT.json]   (DESIGN 4 "Kerr")"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bhr_amd import HipRenderer, scenes
from bhr_amd.textures import compute_disk_texture_resolution

W, H, POV, REPEATS = 1920, 1080, [6, 0, 0.5], 3
n_phi, n_r = compute_disk_texture_resolution(W, H, POV, 90, 2.0, 15.0)
sky, tex = scenes.analytic_skybox(1024, 2048), scenes.noisy_disk(n_r, n_phi)


def measure(spin, ss, mode, n):
    r = HipRenderer(W, H, sky, tex, step_size=0.1, math="strict", frame_slots=1, supersample=ss, spin=spin, redshift=mode)
    for _ in range(3):
        r.render_async(POV, 90)
    r.timing_reset()
    for _ in range(n):
        r.render_async(POV, 90)
    c = r.counters()
    r.close()
    return c["march_ms_sum"] / c["frames_timed"], int(c["ray_steps"]), int(c["march_vgprs"])


res = {}
for spin, ss, n in ((0.9, 1, 20), (-0.9, 1, 20), (0.9, 2, 10), (-0.9, 2, 10)):
    runs = {"model": [], "exact": []}
    meta = {}
    for _ in range(REPEATS):
        for mode in ("model", "exact"):
            ms, steps, vgprs = measure(spin, ss, mode, n)
            runs[mode].append(round(ms, 4))
            meta[mode] = (steps, vgprs)
    name = f"kerr_{spin:g}" + ("_ss2" if ss == 2 else "")
    med = {m: sorted(v)[len(v) // 2] for m, v in runs.items()}
    res[name] = dict(model_ms=runs["model"], exact_ms=runs["exact"], model_ms_median=med["model"], exact_ms_median=med["exact"],
                     model_spread_ms=round(max(runs["model"]) - min(runs["model"]), 4),
                     exact_minus_model_ms=round(med["exact"] - med["model"], 4),
                     ray_steps=dict(model=meta["model"][0], exact=meta["exact"][0]),
                     vgprs=dict(model=meta["model"][1], exact=meta["exact"][1]))
    print(name, res[name], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
