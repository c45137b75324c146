"""fhd default view: march time of the Kerr kernel at A = 0.9, -0.9 and forced at spin 0, and with --supersample 2, next to the
strict march, each on one frame slot (isolated launches).  usage: tools/kerr_measure.py [OUT.json]   (DESIGN 4 "Kerr")"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bhr_amd import HipRenderer, scenes
from bhr_amd.textures import compute_disk_texture_resolution

W, H = 1920, 1080
n_phi, n_r = compute_disk_texture_resolution(W, H, [6, 0, 0.5], 90, 2.0, 15.0)
sky, tex = scenes.analytic_skybox(1024, 2048), scenes.noisy_disk(n_r, n_phi)
res = {}
for name, spin, ss, n in (("strict", 0.0, 1, 20), ("kerr_0.9", 0.9, 1, 20), ("kerr_0.9_ss2", 0.9, 2, 10), ("kerr_0_forced", 0.0, 1, 20), ("kerr_-0.9", -0.9, 1, 20)):
    r = HipRenderer(W, H, sky, tex, step_size=0.1, math="strict", frame_slots=1, supersample=ss)
    if name != "strict":
        r.set_spin(spin, force_kerr=True)
    for _ in range(3):
        r.render_async([6, 0, 0.5], 90)
    r.timing_reset()
    for _ in range(n):
        r.render_async([6, 0, 0.5], 90)
    c = r.counters()
    res[name] = dict(march_ms=round(c["march_ms_sum"] / c["frames_timed"], 4), ray_steps=int(c["ray_steps"]), vgprs=c["march_vgprs"],
                     gsteps_per_s=round(c["ray_steps"] / (c["march_ms_sum"] / c["frames_timed"]) / 1e6, 1))
    r.close()
    print(name, res[name], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
