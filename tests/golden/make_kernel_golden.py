#!/usr/bin/env python3
"""Generates tests/golden/march_ref_*.npz, bloom_ref.npz and texture_ref.npz by running the reference's
OWN kernel function objects.

Run in the build container only (needs /root/reference; the GPU box never sees it):
    python tests/golden/make_kernel_golden.py [-j 8]

How: ``ti_shim`` (next to this file) is registered as the ``taichi`` module, then the reference's
``render.py`` is imported unmodified and its ``TaichiRenderer`` is constructed on small inputs.  Every
call below goes through the reference's host methods (``render``, ``generate_background``,
``eval_noise``, ``update_disk_texture_gpu`` ...), which launch the reference's ``_ray_march_kernel``,
``_bloom_kernel``, ``_generate_background_kernel``, ``_noise_eval_kernel``,
``_compose_disk_texture_kernel`` and the mip kernels (render.py:2389-3489) as plain Python.  The shim
holds primitive-op semantics only; what executes is the reference's statements.  Only inputs and
outputs are stored, never source text.

Each march scene is run twice: ``f64`` (Python floats: the rounding-free value of the statements) and
``f32`` (numpy.float32 scalars: IEEE binary32 after every operation, the closest thing available to
the reference's ``--device cpu`` build, whose default_fp is f32).  Inputs are the seeded textures of
``bhr_amd.scenes`` (recreated by the tests; their SHA-256 is stored so a drift fails loudly).

Instrumentation recorded through the shim's observers (no kernel logic involved): per-pixel RK4 step
counts (= calls of ``_compute_acceleration`` / 4), the escape direction handed to ``_sample_skybox``,
and the arguments/results of sampled ``_apply_g_factor`` / ``_sample_disk_mip`` /
``_color_temp_to_tint`` calls (unit-level pins of the shading, the LOD pick and the tint).
"""
import argparse
import concurrent.futures as cf
import hashlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

# name -> size, camera, reference-constructor arguments, frame number, texture choice
MARCH_SCENES = {
    # BASELINE configs[1] view (fhd default scene), miniature
    "default": dict(width=64, height=36, cam_pos=[6, 0, 0.5], fov=90, frame=0, tex=(32, 128), kw=dict(
        step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=0.0, anti_alias="disabled")),
    # tests/e2e_render.py:27-43 view (configs[0])
    "e2e": dict(width=64, height=36, cam_pos=[6, 0, 0.5], fov=60, frame=0, tex=(32, 128), kw=dict(
        step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=3.5, disk_tilt=15.0, anti_alias="disabled")),
    # configs[2]: tilt 25, lod_radius anti-aliasing, lens flare on
    "tilt_aa": dict(width=64, height=36, cam_pos=[6, 0, 0.5], fov=90, frame=0, tex=(64, 512), kw=dict(
        step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=25.0, anti_alias="lod_radius",
        aa_strength=1.0, lens_flare=True)),
    # compare_aa.py:43 view: far camera, strong minification
    "far_aa": dict(width=64, height=36, cam_pos=[-20, 0, 2], fov=60, frame=0, tex=(64, 512), kw=dict(
        step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=20.0, anti_alias="lod_radius",
        aa_strength=1.5)),
    # camera inside the disk annulus: several plane crossings per ray
    "inside": dict(width=64, height=36, cam_pos=[3.2, 0.5, 0.12], fov=100, frame=0, tex=(32, 128), kw=dict(
        step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=9.0, disk_tilt=3.0, anti_alias="disabled")),
    # camera on the polar axis: build_camera's fallback basis (render.py:108-111)
    "polar": dict(width=48, height=32, cam_pos=[0, 0, 8], fov=70, frame=0, tex=(64, 512), kw=dict(
        step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=6.0, disk_tilt=0.0, anti_alias="lod_radius")),
    # configs[3] step size, off-axis camera, a rotated disk (frame 7 -> t_offset 0.7, render.py:3897)
    "fine_rot": dict(width=48, height=27, cam_pos=[4, 3, 1.5], fov=75, frame=7, tex=(32, 128), kw=dict(
        step_size=0.05, r_max=10.0, r_disk_inner=2.0, r_disk_outer=8.0, disk_tilt=5.0, anti_alias="disabled",
        disk_rotation_speed=0.1)),
    # the far_aa view through a texture whose mip chain stops early: 4x12 -> 2x6 -> 1x3 is three levels
    # (generate_disk_mipmaps, render.py:1118), so _sample_disk_mip clamps the lod 3 crossings to level 2;
    # a sky that is neither a power of two nor 1:2
    "few_levels": dict(width=32, height=18, cam_pos=[-20, 0, 2], fov=60, frame=0, tex=(4, 12), sky=(37, 101), kw=dict(
        step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=20.0, anti_alias="lod_radius",
        aa_strength=1.5)),
    # the same view, the smallest 1:3 texture with four levels (8x24 ... 1x3): lod 3 has its own level; a 2x2 sky
    "four_levels": dict(width=32, height=18, cam_pos=[-20, 0, 2], fov=60, frame=0, tex=(8, 24), sky=(2, 2), kw=dict(
        step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=20.0, anti_alias="lod_radius",
        aa_strength=1.5)),
}
SKY_SHAPE = (64, 128)   # a scene's "sky" entry overrides it
N_UNIT = 192  # sampled ti.func calls kept per scene


def _setup(mode):
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    import ti_shim
    ti_shim.install()
    ti_shim.set_default_fp(mode)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import render as ref
    return ti_shim, ref


def _inputs(tex_shape, sky_shape=SKY_SHAPE):
    import bhr_amd  # noqa: F401
    from bhr_amd import scenes
    return scenes.analytic_skybox(*sky_shape), scenes.noisy_disk(*tex_shape)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _pick(rows, n):
    if len(rows) <= n:
        return np.array(rows, dtype=np.float64)
    idx = np.linspace(0, len(rows) - 1, n).astype(int)
    return np.array([rows[i] for i in idx], dtype=np.float64)


def run_march(task):
    name, mode = task
    t0 = time.time()
    ti, ref = _setup(mode)
    s = MARCH_SCENES[name]
    W, H = s["width"], s["height"]
    sky, tex = _inputs(s["tex"], s.get("sky", SKY_SHAPE))
    r = ref.TaichiRenderer(W, H, sky, tex, **s["kw"])

    steps = np.zeros((W, H), dtype=np.int64)
    esc = np.zeros((W, H, 3), dtype=np.float64)
    cur = [None]
    gf, mip = [], []

    def on_iter(idx):
        cur[0] = idx

    def on_acc(args, out):
        steps[cur[0]] += 1

    def on_sky(args, out):
        esc[cur[0]] = [float(c) for c in args[0]]

    def on_g(args, out):
        base, hit_pos, hit_r, to_cam, cam_pos, r_in, r_out, tilt = args
        gf.append([*base, *hit_pos, hit_r, *to_cam, *cam_pos, r_in, r_out, tilt, *out])

    def on_mip(args, out):
        mip.append([*args, *out])

    ti.iter_hook = on_iter
    ti.observe("_compute_acceleration", on_acc)
    ti.observe("_sample_skybox", on_sky)
    ti.observe("_apply_g_factor", on_g)
    ti.observe("_sample_disk_mip", on_mip)

    # the reference's render() (render.py:3865-3923); the layers it combines are read back the way it does
    layers = {}
    orig_bloom = r._bloom_kernel

    def bloom_spy(*a):
        layers["bg"] = r.image_field.to_numpy()
        layers["disk"] = r.disk_layer_field.to_numpy()  # before the kernel's in-place update (3112-3114)
        return orig_bloom(*a)

    r._bloom_kernel = bloom_spy
    final = r.render(s["cam_pos"], s["fov"], frame=s["frame"])
    layers["blur"] = r.blur_field.to_numpy()
    layers["disk_after_bloom"] = r.disk_layer_field.to_numpy()
    ti.iter_hook = None
    for n in ("_compute_acceleration", "_sample_skybox", "_apply_g_factor", "_sample_disk_mip"):
        ti.observe(n, None)
    assert (steps % 4 == 0).all()

    dt = np.float64 if mode == "f64" else np.float32     # observer records; field contents are f32 in both modes
    out = {f"{mode}_{k}": v for k, v in layers.items()}
    out[f"{mode}_final"] = np.asarray(final)                                  # (H, W, 3), flare included
    out[f"{mode}_steps"] = (steps // 4).astype(np.int32)
    out[f"{mode}_escape_dir"] = esc.astype(dt)
    out[f"{mode}_gfactor_calls"] = _pick(gf, N_UNIT).astype(dt).reshape(-1, 19)
    out[f"{mode}_mip_calls"] = _pick(mip, N_UNIT).astype(dt).reshape(-1, 10)
    out["sky_sha256"], out["tex_sha256"] = _sha(sky), _sha(tex)
    print(f"  march {name:9s} {mode}: {time.time() - t0:6.1f} s, {int(steps.sum()) // 4} steps, "
          f"{len(gf)} hits", flush=True)
    return name, out


def run_bloom(mode):
    """_bloom_kernel on a synthetic layer wide enough for a real radius (R = int(0.02 W) = 3) and on a
    frame narrower than one tap (R = 0)."""
    ti, ref = _setup(mode)
    out = {}
    for tag, (W, H) in (("wide", (160, 20)), ("narrow", (40, 6))):
        sky, tex = _inputs((32, 128))
        r = ref.TaichiRenderer(W, H, sky, tex)
        rng = np.random.default_rng(17)
        layer = rng.random((W, H, 3), dtype=np.float32) ** 4
        layer[rng.random((W, H)) < 0.35] = 0.0           # lum == 0 pixels: the threshold branch
        layer[:, H // 2] = 0.0
        r.disk_layer_field.from_numpy(layer)
        R = int(W * 0.02)
        r._bloom_kernel(r.disk_layer_field, r.bright_field, r.blur_field, 0, 0.4, R, (W / 640.0) ** 2)
        out[f"{tag}_layer"] = layer
        out[f"{tag}_{mode}_blur"] = r.blur_field.to_numpy()
        out[f"{tag}_{mode}_layer_after"] = r.disk_layer_field.to_numpy()
        out[f"{tag}_radius"] = R
    print(f"  bloom {mode} done", flush=True)
    return out


def run_texture(mode):
    """Noise, background generator, compose kernel and mip chain through the reference's host methods."""
    ti, ref = _setup(mode)
    dt = np.float64 if mode == "f64" else np.float32     # observer records only
    out = {}
    n_r, n_phi = 16, 48
    sky, _ = _inputs((32, 128))
    r = ref.TaichiRenderer(32, 18, sky, np.zeros((n_r, n_phi, 4), dtype=np.float32), r_disk_inner=2.0, r_disk_outer=15.0)

    # ---- eval_noise (render.py:3769-3790)
    rng = np.random.default_rng(23)
    coords = np.concatenate([rng.uniform(-4, 4, (400, 3)), rng.uniform(-900, 900, (300, 3)),
                             rng.integers(-3, 4, (60, 3)).astype(np.float64)]).astype(np.float32)
    out["noise_coords"] = coords
    out[f"{mode}_simplex"] = r.eval_noise(coords, mode="simplex")
    out[f"{mode}_fbm_4_05_2"] = r.eval_noise(coords, mode="fbm", octaves=4, persistence=0.5, lacunarity=2.0)
    out[f"{mode}_fbm_5_045_2"] = r.eval_noise(coords[:300], mode="fbm", octaves=5, persistence=0.45,
                                              lacunarity=2.0)

    # ---- background generator (render.py:3491-3562, 3332-3451)
    r.init_background_layer(n_r, n_phi, seed=42)
    out["bg_az"] = np.array([r._bg_az_freq, r._bg_az_shear])
    for t in (0.0, 5.0, 36.5):
        r.generate_background(t)
        out[f"{mode}_bg_t{t:g}"] = r._comp_field.to_numpy()

    # ---- compose + mips on that field with synthetic entity planes (render.py:3714-3767)
    comp = r._comp_field.to_numpy()
    comp[5:11] = rng.random((6, n_r, n_phi)) * np.array([1, 0.1, 1, 0.1, 1, 0.1])[:, None, None]
    r._comp_field.from_numpy(comp)
    stats = np.array([0.31, 0.07], dtype=np.float32)
    row_stats = np.stack([0.2 + 0.8 * rng.random(n_r), 0.05 + 0.3 * rng.random(n_r)], axis=1).astype(np.float32)
    r._param_stats_field.from_numpy(stats)
    r._param_row_stats_field.from_numpy(row_stats)
    tints = []
    ti.observe("_color_temp_to_tint", lambda args, o: tints.append([args[0], *o]))
    r._parametric_gpu_ready = True
    for t in (0.0, 12.5):
        if t == 0.0:
            r.compose_interactive_texture()   # lifecycle path: compose (t_offset 0) + copy-base + 4 downsamples
        else:
            r.update_disk_texture_gpu(t)      # same kernels with a rolled source column (render.py:3202-3207)
        out[f"{mode}_tex_t{t:g}"] = r.disk_texture_field.to_numpy()
        out[f"{mode}_mips_t{t:g}"] = r.disk_mips_field.to_numpy()
    ti.observe("_color_temp_to_tint", None)
    out[f"{mode}_tint_calls"] = _pick(tints, 256).astype(dt)
    out["compose_comp"] = comp.astype(np.float32)
    out["compose_stats"], out["compose_row_stats"] = stats, row_stats
    out["compose_omega"] = r._omega_rows_field.to_numpy().astype(np.float32)
    out["compose_edge"] = r._edge_field.to_numpy().astype(np.float32)
    print(f"  texture {mode} done", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--only", default=None, help="comma-separated march scene names (debug)")
    a = ap.parse_args()
    names = list(MARCH_SCENES) if a.only is None else a.only.split(",")
    tasks = [(n, m) for n in names for m in ("f64", "f32")]
    merged = {}
    with cf.ProcessPoolExecutor(max_workers=a.j) as ex:
        fb = [ex.submit(run_bloom, m) for m in ("f64", "f32")] if a.only is None else []
        ft = [ex.submit(run_texture, m) for m in ("f64", "f32")] if a.only is None else []
        for name, out in ex.map(run_march, tasks):
            merged.setdefault(name, {}).update(out)
        for name, d in merged.items():
            s = MARCH_SCENES[name]
            meta = dict(width=s["width"], height=s["height"], cam_pos=np.array(s["cam_pos"], dtype=np.float64),
                        fov=float(s["fov"]), frame=s["frame"], tex_shape=np.array(s["tex"]),
                        sky_shape=np.array(s.get("sky", SKY_SHAPE)))
            np.savez_compressed(os.path.join(a.out, f"march_ref_{name}.npz"), **meta, **d)
        if fb:
            d = {}
            for f in fb:
                d.update(f.result())
            np.savez_compressed(os.path.join(a.out, "bloom_ref.npz"), **d)
            d = {}
            for f in ft:
                d.update(f.result())
            np.savez_compressed(os.path.join(a.out, "texture_ref.npz"), **d)
    for f in sorted(os.listdir(a.out)):
        if f.endswith("_ref.npz") or f.startswith("march_ref_"):
            print(f, os.path.getsize(os.path.join(a.out, f)))


if __name__ == "__main__":
    main()
