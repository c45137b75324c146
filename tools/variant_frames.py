"""One small frame of every march variant, with the library of the tree this file sits in: the sha256 of the f32 FINAL layer and
the frame's ray_steps, as JSON.  Run on two trees, the outputs say whether a change of the host launch path (march_launch.hip:
variant_args, march_kernel) left every variant's frame what it was, bit for bit.
usage: tools/variant_frames.py [OUT.json]
Frames of 160 x 96 (full tiles) and the ragged 67 x 45, at supersample 1 and 2 (both kernel twins), math strict."""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bhr_amd import HipRenderer, _lib, scenes

POV, FOV = [6.0, 0.0, 0.5], 90.0
BETA = (0.3, 0.1, -0.2)
# (name, (spin, force_kerr, redshift), render_async's keywords)
CASES = (
    ("strict", (0.0, False, "model"), {}),
    ("kerr_0.7_model", (0.7, False, "model"), {}),
    ("kerr_0.7_exact", (0.7, False, "exact"), {}),
    ("kerr_forced_spin_0", (0.0, True, "model"), {}),
    ("observer_sky_shift", (0.0, False, "model"), dict(observer=BETA, observer_sky=True)),
    ("observer_plain_sky", (0.0, False, "model"), dict(observer=BETA, observer_sky=False)),
    ("equirect_360x180_at_rest", (0.0, False, "model"), dict(projection="equirect", projection_fov=(360.0, 180.0))),
    ("fisheye_200_observer", (0.0, False, "model"), dict(projection="fisheye", projection_fov=(200.0,), observer=BETA)),
    ("light_delay_1", (0.0, False, "model"), dict(light_delay=1.0)),
    ("light_delay_0", (0.0, False, "model"), dict(light_delay=0.0)),
)

out = {}
sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
for W, H in ((160, 96), (67, 45)):
    r = HipRenderer(W, H, sky, tex, step_size=0.1, math="strict")
    for ss in (1, 2):
        r.set_supersample(ss)
        for name, (spin, force, redshift), kw in CASES:
            r.set_spin(spin, force_kerr=force)      # the spin before the exact redshift, which is a Kerr kernel's
            r.set_redshift(redshift)
            r.timing_reset()
            r.render_async(POV, FOV, **kw)
            final = r.read_layer(_lib.LAYER_FINAL)
            out[f"{W}x{H}/ss{ss}/{name}"] = {"final_sha256": hashlib.sha256(final.tobytes()).hexdigest(), "ray_steps": int(r.counters()["ray_steps"])}
            r.set_redshift("model")                 # ... and off again before the spin goes
    r.close()
text = json.dumps(out, indent=1)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
