"""fhd default view, A = 0.9: march time of the Kerr march over the Disk V2 sources (bhr_set_kerr_disk_source) -- the surface under
the model and the exact redshift, the volume with 2 pieces per step -- next to the texture Kerr frame of the same build and, for
scale, the strict Schwarzschild Disk V2 surface and volume frames; each on one frame slot (isolated launches).  The rows alternate,
REPEATS contexts of each, so that the spread between the repeats of one row stands next to the differences between the rows.
usage: tools/kerr_dv2_measure.py [OUT.json]   (DESIGN 4 "Kerr Disk V2")"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bhr_amd import HipRenderer, drivers, scenes
from bhr_amd.textures import compute_disk_texture_resolution

W, H, POV, REPEATS, SPIN = 1920, 1080, [6, 0, 0.5], 3, 0.9
n_phi, n_r = compute_disk_texture_resolution(W, H, POV, 90, 2.0, 15.0)
sky, tex = scenes.analytic_skybox(1024, 2048), scenes.noisy_disk(n_r, n_phi)


def measure(n, spin=0.0, redshift="model", kerr_disk_model="texture", disk_model="texture"):
    r = HipRenderer(W, H, sky, tex, step_size=0.1, math="strict", frame_slots=1, spin=spin, redshift=redshift)
    drivers.use_kerr_analytic_disk(r, kerr_disk_model)
    drivers.use_analytic_disk(r, disk_model)
    for _ in range(2):
        r.render_async(POV, 90)
    r.timing_reset()
    for _ in range(n):
        r.render_async(POV, 90)
    c = r.counters()
    r.close()
    return c["march_ms_sum"] / c["frames_timed"], int(c["ray_steps"]), int(c["march_vgprs"])


rows = (("kerr_texture", 20, dict(spin=SPIN)), ("kerr_v2", 20, dict(spin=SPIN, kerr_disk_model="v2")),
        ("kerr_v2_exact", 20, dict(spin=SPIN, redshift="exact", kerr_disk_model="v2")), ("kerr_v2_volume", 8, dict(spin=SPIN, kerr_disk_model="v2_volume")),
        ("strict_v2", 20, dict(disk_model="v2")), ("strict_v2_volume", 8, dict(disk_model="v2_volume")))
runs, meta = {name: [] for name, _, _ in rows}, {}
for _ in range(REPEATS):
    for name, n, kw in rows:
        ms, steps, vgprs = measure(n, **kw)
        runs[name].append(round(ms, 4))
        meta[name] = (steps, vgprs)
res = {}
for name, n, kw in rows:
    v = runs[name]
    res[name] = dict(march_ms=v, march_ms_median=sorted(v)[len(v) // 2], spread_ms=round(max(v) - min(v), 4), frames_per_run=n, ray_steps=meta[name][0],
                     march_vgprs=meta[name][1])
    print(name, res[name], flush=True)
base = res["kerr_texture"]["march_ms_median"]
res["over_kerr_texture"] = {name: round(res[name]["march_ms_median"] / base, 3) for name, _, _ in rows}
res["kerr_over_strict"] = dict(v2=round(res["kerr_v2"]["march_ms_median"] / res["strict_v2"]["march_ms_median"], 3),
                               v2_volume=round(res["kerr_v2_volume"]["march_ms_median"] / res["strict_v2_volume"]["march_ms_median"], 3))
print(res["over_kerr_texture"], res["kerr_over_strict"], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
