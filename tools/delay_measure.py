"""fhd default view and 4k with the disk tilted by 25 degrees (no anti-aliasing): march time of the delayed kernel at scale 1 next
to the strict march of the same view in the same run -- one context per view, one frame slot (isolated launches), the two
alternating over several rounds, medians -- with the kernels' registers, LDS, scratch and waves per SIMD.
usage: tools/delay_measure.py [--strict-only] [OUT.json]   (DESIGN 4 "Light delay")
--strict-only times the strict march alone, through nothing the light delay added: the same script then runs on a tree of the
commit before it, which gives the third column of the table."""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bhr_amd import HipRenderer, scenes
from bhr_amd.textures import compute_disk_texture_resolution

argv = [a for a in sys.argv[1:] if a != "--strict-only"]
STRICT_ONLY = len(argv) != len(sys.argv) - 1
POV, FOV, ROUNDS = [6, 0, 0.5], 90, 7
VIEWS = (("fhd", 1920, 1080, 0.0, 20), ("4k_tilt25", 3840, 2160, 25.0, 8))
res = {"how": f"pov {POV}, fov {FOV}, step 0.1, math strict, anti_alias off, one frame slot; {ROUNDS} rounds, strict and delayed (scale 1) "
              "alternating; medians of the rounds' means"}
for view, W, H, tilt, frames in VIEWS:
    n_phi, n_r = compute_disk_texture_resolution(W, H, POV, FOV, 2.0, 15.0)
    sky, tex = scenes.analytic_skybox(1024, 2048), scenes.noisy_disk(n_r, n_phi)
    r = HipRenderer(W, H, sky, tex, step_size=0.1, math="strict", frame_slots=1, disk_tilt=tilt)
    runs = (("strict", None),) if STRICT_ONLY else (("strict", None), ("delayed", 1.0))
    ms, steps = {name: [] for name, _ in runs}, {}
    for rnd in range(ROUNDS + 1):                       # round 0 warms up: code objects, clocks
        for name, scale in runs:
            kw = {} if scale is None else {"light_delay": scale}
            r.timing_reset()
            for _ in range(frames):
                r.render_async(POV, FOV, **kw)
            c = r.counters()
            steps[name] = int(c["ray_steps"])
            if rnd:
                ms[name].append(c["march_ms_sum"] / c["frames_timed"])
    out = {"frame": f"{W}x{H}, disk_tilt {tilt:g}, {frames} frames a round",
           "resources": {"strict": {"vgprs": r.counters()["march_vgprs"], "lds_bytes": r.counters()["march_lds_bytes"]}}}
    if not STRICT_ONLY:
        for key, ss in (("delayed", False), ("delayed_ss", True)):
            k = r.delayed_resources(ss)
            k["waves_per_simd"] = min(8, 512 // (8 * ((k["vgprs"] + 7) // 8)))     # gfx950: 512 VGPRs per lane and SIMD, allotted in eights
            out["resources"][key] = k
    r.close()
    for name, _ in runs:
        m = statistics.median(ms[name])
        out[name] = dict(march_ms=round(m, 4), march_ms_min=round(min(ms[name]), 4), march_ms_max=round(max(ms[name]), 4), ray_steps=steps[name],
                         ns_per_kilostep=round(m * 1e9 / steps[name], 4), gsteps_per_s=round(steps[name] / m / 1e6, 1))
    if not STRICT_ONLY:
        out["delayed"]["march_ratio_to_strict"] = round(out["delayed"]["march_ms"] / out["strict"]["march_ms"], 4)
        out["delayed"]["same_steps_as_strict"] = steps["delayed"] == steps["strict"]
    res[view] = out
print(json.dumps(res, indent=1))
if argv:
    with open(argv[0], "w") as f:
        json.dump(res, f, indent=1)
