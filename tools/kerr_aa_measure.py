"""fhd default view: march time of the anti-aliased Kerr kernel (bhr_set_kerr_anti_alias) next to the Kerr kernel without it, at
A = 0.9 under both redshifts and with --supersample 2, each on one frame slot (isolated launches); and for scale the strict
Schwarzschild march with --anti_alias lod_radius next to the one without.  Off and on alternate, REPEATS contexts of each, so that
the spread between the repeats of one setting stands next to the difference between the two.
usage: tools/kerr_aa_measure.py [OUT.json]   (DESIGN 4 "Kerr anti-aliasing")"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bhr_amd import HipRenderer, scenes
from bhr_amd.textures import compute_disk_texture_resolution

W, H, POV, REPEATS = 1920, 1080, [6, 0, 0.5], 3
n_phi, n_r = compute_disk_texture_resolution(W, H, POV, 90, 2.0, 15.0)
sky, tex = scenes.analytic_skybox(1024, 2048), scenes.noisy_disk(n_r, n_phi)


def measure(n, ss=1, spin=0.0, redshift="model", kerr_aa=False, anti_alias="disabled"):
    r = HipRenderer(W, H, sky, tex, step_size=0.1, math="strict", frame_slots=1, supersample=ss, spin=spin, redshift=redshift, anti_alias=anti_alias)
    if kerr_aa:
        r.set_kerr_anti_alias(True, 1.0)
    for _ in range(3):
        r.render_async(POV, 90)
    r.timing_reset()
    for _ in range(n):
        r.render_async(POV, 90)
    c = r.counters()
    r.close()
    return c["march_ms_sum"] / c["frames_timed"], int(c["ray_steps"]), int(c["march_vgprs"])


res = {}
rows = (("kerr_0.9", 20, dict(spin=0.9), dict(kerr_aa=True)), ("kerr_0.9_exact", 20, dict(spin=0.9, redshift="exact"), dict(kerr_aa=True)),
        ("kerr_0.9_ss2", 10, dict(spin=0.9, ss=2), dict(kerr_aa=True)), ("strict_schwarzschild", 20, dict(), dict(anti_alias="lod_radius")))
for name, n, base, on in rows:
    runs, meta = {"off": [], "on": []}, {}
    for _ in range(REPEATS):
        for key, kw in (("off", base), ("on", dict(base, **on))):
            ms, steps, vgprs = measure(n, **kw)
            runs[key].append(round(ms, 4))
            meta[key] = (steps, vgprs)
    med = {m: sorted(v)[len(v) // 2] for m, v in runs.items()}
    res[name] = dict(off_ms=runs["off"], on_ms=runs["on"], off_ms_median=med["off"], on_ms_median=med["on"],
                     off_spread_ms=round(max(runs["off"]) - min(runs["off"]), 4), on_over_off=round(med["on"] / med["off"], 3),
                     ray_steps=dict(off=meta["off"][0], on=meta["on"][0]), vgprs=dict(off=meta["off"][1], on=meta["on"][1]))
    print(name, res[name], flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
