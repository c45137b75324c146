"""Frame drivers on top of HipRenderer: single image and video (render.py:4031-4153, 4356-4511).

Kept from the reference: the lifecycle call sequence, the orbit camera, the resume format
(``.frames_<md5(output)[:16]>/progress.json`` = {params, completed}), PNG frames written by a
2-thread pool, MP4 assembly through imageio/pyav when those packages exist.
New: frames can be sharded round-robin over ranks (``rank``/``world``): every rank replays the
cheap CPU lifecycle for every frame index and renders only its own frames; normalisation
statistics are recomputed at every ``frame % 60 == 0`` by *frame index* (so the output does not
depend on the sharding), which also makes a resumed video identical to an uninterrupted one.
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import time
from typing import List, Optional

import numpy as np

from . import rules
from .camera import orbit_position
from .lifecycle import make_factories
from .output import Y4MStream, FrameSink, VIDEO_LEVEL, DEVICE, DITHERS, png_write, quantize, quantize16, write_passes
from .renderer import HipRenderer, R_DISK_INNER_DEFAULT, R_DISK_OUTER_DEFAULT, check_grade
from .skybox import load_or_generate_skybox
from .textures import compute_disk_texture_resolution, load_disk_texture


def check_depth_and_dither(bit_depth: int, dither: str, video_codec: str = "auto") -> None:
    """The combinations the output side takes: 16-bit output is neither dithered (65536 levels need none) nor JPEG-coded."""
    if bit_depth not in (8, 16):
        raise ValueError(f"bit_depth must be 8 or 16, got {bit_depth!r}")
    if dither not in DITHERS:
        raise ValueError(f"dither must be one of {DITHERS}, got {dither!r}")
    rules.refuse_on("bit_depth_16", locals())


def save_image(image: np.ndarray, path: str, bit_depth: int = 8, dither: str = "none") -> None:
    """float image -> 8-bit PNG with truncation, not rounding (render.py:420-425).  Encoded by the
    library (row bands deflated in parallel); non-PNG extensions go through PIL as in the reference.
    ``bit_depth=16``: a 16-bit PNG of output.quantize16(image) (PNG only).  ``dither="blue"``: the 8-bit values are
    output.quantize(image, dither="blue").  Both quantise on the host with the device's formulas restated, whichever way
    the image was rendered."""
    check_depth_and_dither(bit_depth, dither)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if bit_depth == 16:
        if not path.lower().endswith(".png"):
            raise ValueError(f"bit_depth 16 writes PNG files, got {path!r}")
        png_write(path, quantize16(image))
    elif path.lower().endswith(".png"):
        png_write(path, quantize(image, dither=dither))
    else:
        from PIL import Image
        Image.fromarray(quantize(image, dither=dither)).save(path)
    print(f"Saved: {path}")


HDR_FORMATS = (".pfm", ".hdr")


def check_hdr_path(path: str) -> None:
    if not str(path).lower().endswith(HDR_FORMATS):
        raise ValueError(f"the HDR master is written as .pfm or .hdr, got {path!r}")


def rgbe_encode(image: np.ndarray) -> np.ndarray:
    """(H, W, 3) float -> (H, W, 4) uint8 Radiance RGBE: the shared exponent is frexp's of the largest channel, the mantissas
    are truncated (m * 256 / 2^e), a pixel whose largest channel is below 1e-32 is four zeros."""
    x = np.clip(np.nan_to_num(np.asarray(image, dtype=np.float32), nan=0.0, posinf=np.float32(65504.0)), 0.0, None)
    big = x.max(axis=-1)
    _, e = np.frexp(big)
    live = big >= 1e-32
    scale = np.where(live, np.ldexp(np.float32(1.0), 8 - np.where(live, e, 0)), np.float32(0.0)).astype(np.float32)
    out = np.empty(x.shape[:2] + (4,), dtype=np.uint8)
    out[..., :3] = np.minimum(np.floor(x * scale[..., None]), 255).astype(np.uint8)
    out[..., 3] = np.where(live, e + 128, 0).astype(np.uint8)
    return out


def save_hdr(image: np.ndarray, path: str) -> None:
    """The scene-linear float frame (HipRenderer.read_hdr) as a file, encoded on the host.  ``.pfm``: the f32 values as they
    are, little-endian, rows bottom-up (header "PF", "W H", "-1.0").  ``.hdr``: Radiance RGBE, flat (no run-length coding),
    rows top-down, header "#?RADIANCE" / "FORMAT=32-bit_rle_rgbe" (rgbe_encode)."""
    check_hdr_path(path)
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"save_hdr takes an (H, W, 3) image, got {image.shape}")
    h, w = image.shape[:2]
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "wb") as f:
        if path.lower().endswith(".pfm"):
            f.write(f"PF\n{w} {h}\n-1.0\n".encode("ascii"))
            f.write(np.ascontiguousarray(image[::-1], dtype="<f4").tobytes())
        else:
            f.write(f"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y {h} +X {w}\n".encode("ascii"))
            f.write(rgbe_encode(image).tobytes())
    print(f"Saved: {path}")


def init_lifecycle_system(renderer: HipRenderer, n_r: int, n_phi: int, seed: int = 42) -> dict:
    """Background parameters + the three pre-aged entity populations + a first composed texture
    (render.py:4079-4130)."""
    renderer.init_background_layer(n_r=n_r, n_phi=n_phi, seed=seed)
    factories = make_factories(n_r, n_phi, renderer.r_disk_inner, renderer.r_disk_outer, seed=seed)
    renderer.generate_background(t=0.0)
    renderer.accumulate_entity_layer(factories, now=0.0)
    renderer.recompute_interactive_stats()
    renderer.compose_interactive_texture()
    return factories


def advance_lifecycle_frame(renderer: HipRenderer, factories: dict, t: float, dt: float,
                            recompute_stats: bool = False, solo_idx: int = -1, compose: bool = True) -> None:
    """Tick the factories and rebuild the texture for time t (render.py:4133-4153).
    ``compose=False`` only advances the CPU state (used by ranks skipping a frame they do not render)."""
    for f in factories.values():
        f.tick(now=t, dt=dt)
    if not compose and not recompute_stats:
        return
    renderer.generate_background(t=t)
    renderer.accumulate_entity_layer(factories, now=t)
    if recompute_stats:
        renderer.recompute_interactive_stats()
    if compose:
        renderer.compose_interactive_texture(solo_idx=solo_idx)


def use_analytic_disk(renderer: HipRenderer, disk_model: str) -> bool:
    """--disk_model v2 / v2_volume: Disk V2 with the renderer's radii and default structure (seed 42)."""
    if disk_model == "texture":
        return False
    if disk_model not in ("v2", "v2_volume"):
        raise ValueError(f"unknown disk_model {disk_model!r}")
    from .disk_v2 import DiskV2Params
    renderer.use_disk_v2(DiskV2Params(r_in=renderer.r_disk_inner, r_out=renderer.r_disk_outer), seed=42,
                         volume=disk_model == "v2_volume")
    return True


KERR_DISK_MODELS = ("texture", "v2", "v2_volume")


def use_kerr_analytic_disk(renderer: HipRenderer, kerr_disk_model: str) -> bool:
    """--spin_disk_model v2 / v2_volume: use_analytic_disk for the Kerr march (HipRenderer.use_kerr_disk_v2)."""
    if kerr_disk_model == "texture":
        return False
    from .disk_v2 import DiskV2Params
    renderer.use_kerr_disk_v2(DiskV2Params(r_in=renderer.r_disk_inner, r_out=renderer.r_disk_outer), seed=42,
                              volume=kerr_disk_model == "v2_volume")
    return True


def _checked_kerr_disk_model(kerr_disk_model, facts) -> str:
    """The Kerr march's disk source as render_image / render_video take it: one of KERR_DISK_MODELS, and what
    rules.FEATURES["kerr_disk_model"] refuses is refused."""
    if kerr_disk_model not in KERR_DISK_MODELS:
        raise ValueError(f"--spin_disk_model is one of {KERR_DISK_MODELS}, got {kerr_disk_model!r}")
    rules.refuse_on("kerr_disk_model", facts)
    return kerr_disk_model


KERR_LINE_KEYS = ("path", "g_map_path", "n_bins", "g_range", "index", "power", "emissivity", "orders", "r_inner", "r_outer", "energy_kev")


def _checked_kerr_line(kerr_line, facts):
    """--spin_line PATH.npz / --spin_g_map PATH.png / kerr_line=dict(path=, g_map_path=, n_bins=, g_range=, index=, power=,
    emissivity=, orders=, r_inner=, r_outer=, energy_kev=): the relativistically broadened emission line of a spinning hole's disk
    and its redshift map, from the Kerr ray map of the view (HipRenderer.set_kerr_line; bhr_amd.line) -> dict(settings=, path=,
    g_map_path=, energy_kev=) with the defaults filled in, or None.  What rules.FEATURES["kerr_line"] refuses is refused first, then
    the values."""
    if kerr_line is None:
        return None
    from . import line as line_mod
    unknown = sorted(set(kerr_line) - set(KERR_LINE_KEYS))
    if unknown:
        raise ValueError(f"--spin_line: unknown settings {unknown} (known: {', '.join(KERR_LINE_KEYS)})")
    rules.refuse_on("kerr_line", facts)
    if kerr_line.get("path") is None and kerr_line.get("g_map_path") is None:
        raise ValueError("--spin_line: neither a path for the profile nor one for the redshift map: nothing to write")
    settings = line_mod.check_settings(**{k: kerr_line[k] for k in line_mod.DEFAULTS if k in kerr_line})
    energy = float(kerr_line.get("energy_kev", line_mod.DEFAULT_ENERGY_KEV))
    if not (energy > 0 and energy < float("inf")):
        raise ValueError(f"--spin_line_energy is the line's rest energy in keV, finite and greater than 0, got {energy}")
    return dict(settings=settings, path=kerr_line.get("path"), g_map_path=kerr_line.get("g_map_path"), energy_kev=energy)


def _kerr_line_facts(kerr_line) -> dict:
    if kerr_line is None:
        return {}
    return dict(kerr_line=True, kerr_line_path=kerr_line.get("path"), g_map_path=kerr_line.get("g_map_path"))


def _save_kerr_line(renderer, kerr_line, n_rows=None) -> None:
    """The profile of device row 0 -- or of rows 0 .. n_rows - 1, one per frame -- to the line's .npz."""
    from . import line as line_mod
    prof = renderer.kerr_line(0, n_rows, energy_kev=kerr_line["energy_kev"])
    info = renderer.kerr_line_info(0)
    if kerr_line["path"] is not None:
        line_mod.save_npz(kerr_line["path"], prof)
    frames = "" if n_rows is None else f"{n_rows} frames, frame 0: "
    print(f"Line profile: {prof['settings']['n_bins']} bins, {frames}{info['samples']} samples, {info['overflow_pixels']} overflow pixels skipped, "
          f"g from {np.ravel(prof['g_red'])[0]:.3f} to {np.ravel(prof['g_blue'])[0]:.3f}, mean {np.ravel(prof['g_mean'])[0]:.3f}"
          + ("" if kerr_line["path"] is None else f"; saved: {kerr_line['path']}"))


def make_renderer(width, height, cam_pos, fov, step_size=0.1, skybox_path=None, n_stars=6000, tex_w=2048,
                  tex_h=1024, r_max=10.0, disk_texture_path=None, r_disk_inner=R_DISK_INNER_DEFAULT,
                  r_disk_outer=R_DISK_OUTER_DEFAULT, disk_tilt=0.0, lens_flare=False, anti_alias="disabled",
                  aa_strength=1.0, disk_rotation_speed=0.1, device_index=0, rows=None, frame_slots=None, math=None,
                  supersample=1, supersample_threshold=None, spin=0.0, redshift="model", stars=None, kerr_stars=None):
    """Renderer with a placeholder (or file) disk texture, as the reference's entry points build it
    (render.py:4044-4064, 4627-4644).  Returns (renderer, use_lifecycle, n_r, n_phi).
    ``stars``: None, or the point stars of check_stars -- the procedural sky is then built WITHOUT its baked star blobs and its
    ``n_stars`` stars become the renderer's catalogue (HipRenderer.set_stars), with the solid angle of a pixel of the view
    (cam_pos, fov) in their flux, so that the look does not depend on the resolution.
    ``kerr_stars``: None, or the Kerr point stars of check_kerr_stars -- the same for a spinning hole: the starless sky, and the
    catalogue set as the KERR ray map's (HipRenderer.set_kerr_stars)."""
    stars = check_stars(stars, skybox_path=skybox_path, supersample=supersample, spin=spin, redshift=redshift)
    kerr_stars = check_kerr_stars(kerr_stars, spin=spin, redshift=redshift, skybox_path=skybox_path, stars=stars is not None, supersample=supersample)
    # procedural sky: the host draws its random tables, the device rasterises them (nebula resize, star blobs in
    # NumPy's accumulation order, Milky-Way glow; skyglow.hip); an image file is loaded as it is
    procedural_sky = not (skybox_path and os.path.isfile(skybox_path))
    if procedural_sky:
        print(f"Texture not found: {skybox_path}, generating procedural skybox..." if skybox_path
              else "Generating procedural skybox...")
        skybox = np.zeros((tex_h, tex_w, 3), dtype=np.float32)          # fixes the size; built on the device below
    else:
        skybox, tex_h, tex_w = load_or_generate_skybox(skybox_path, tex_w, tex_h, n_stars)
    disk_tex = load_disk_texture(disk_texture_path)
    use_lifecycle = disk_tex is None
    if use_lifecycle:
        n_phi, n_r = compute_disk_texture_resolution(width, height, cam_pos, fov, r_disk_inner, r_disk_outer)
        disk_tex = np.zeros((n_r, n_phi, 4), dtype=np.float32)
    else:
        n_r, n_phi = disk_tex.shape[:2]
    renderer = HipRenderer(width, height, skybox, disk_tex, step_size=step_size, r_max=r_max,
                           r_disk_inner=r_disk_inner, r_disk_outer=r_disk_outer, disk_tilt=disk_tilt,
                           lens_flare=lens_flare, anti_alias=anti_alias, aa_strength=aa_strength,
                           disk_rotation_speed=disk_rotation_speed, device_index=device_index, rows=rows,
                           frame_slots=frame_slots, supersample=supersample, supersample_threshold=supersample_threshold,
                           **({} if math is None else {"math": math}), **({"spin": spin} if spin != 0 else {}),
                           **({"redshift": redshift} if redshift != "model" else {}))
    if procedural_sky and (stars is not None or kerr_stars is not None):
        from .skybox import sky_tables
        from .stars import catalog_from_tables
        # (the checks have refused both at once: the catalogue is the Schwarzschild map's or the Kerr map's)
        points, set_catalog = (stars, renderer.set_stars) if stars is not None else (kerr_stars, renderer.set_kerr_stars)
        renderer.build_procedural_skybox(seed=42, n_stars=n_stars, starless=True)
        cam = renderer.camera_uniforms(cam_pos, fov, 0)
        dirs, flux = catalog_from_tables(sky_tables(tex_w, tex_h, 42, n_stars), points["gain"], float(cam.pixel_width) * float(cam.pixel_height))
        set_catalog(dirs, flux, max_magnification=points["max_magnification"])
    elif procedural_sky:
        renderer.build_procedural_skybox(seed=42, n_stars=n_stars)
    return renderer, use_lifecycle, n_r, n_phi


def render_image(width: int, height: int, cam_pos: List[float], fov: float, step_size: float,
                 skybox_path: Optional[str] = None, n_stars: int = 6000, tex_w: int = 2048, tex_h: int = 1024,
                 r_max: float = 10.0, device: str = "hip", disk_texture_path: Optional[str] = None,
                 r_disk_inner: float = R_DISK_INNER_DEFAULT, r_disk_outer: float = R_DISK_OUTER_DEFAULT,
                 disk_tilt: float = 0.0, lens_flare: bool = False, anti_alias: str = "disabled",
                 aa_strength: float = 1.0, disk_rotation_speed: float = 0.1, disk_generation_scale: int = 2,
                 force_regenerate_disk_texture: bool = False, ignore_taichi_cache: bool = False,
                 gpus: int = 1, disk_model: str = "texture", math: Optional[str] = None,
                 supersample: int = 1, supersample_threshold: Optional[float] = None, bit_depth: int = 8,
                 dither: str = "none", grade: Optional[dict] = None, hdr_path: Optional[str] = None,
                 passes_path: Optional[str] = None, spin: float = 0.0, redshift: str = "model",
                 observer=None, observer_sky: bool = True, stars: Optional[dict] = None,
                 projection: Optional[str] = None, projection_fov=None, light_delay=None, polarization: Optional[dict] = None,
                 stokes_path: Optional[str] = None, ticks_path: Optional[str] = None, kerr_polarization: Optional[dict] = None,
                 kerr_view: Optional[dict] = None, kerr_stars: Optional[dict] = None, kerr_passes_path: Optional[str] = None,
                 kerr_anti_alias: Optional[float] = None, kerr_disk_model: str = "texture", kerr_line: Optional[dict] = None) -> np.ndarray:
    """One frame -> (H, W, 3) float32 (render.py:4031-4076).  ``gpus > 1`` tiles the frame in row
    blocks over that many devices of this node (bhr_group_render).  ``math``: march arithmetic
    ("strict" | "hybrid" | "fast"; None = HipRenderer's default, strict).  ``supersample``: k x k rays per
    pixel (one device only); ``supersample_threshold``: adaptive -- only for the pixels whose k = 1 neighbours differ by more
    than it (HipRenderer.set_supersample; None: every pixel).  ``bit_depth`` / ``dither`` are checked here and applied by
    save_image to the frame this returns (the f32 frame does not depend on them).  ``grade``: None, or a dict of
    HipRenderer.set_grade's arguments (tonemap, exposure, white, transfer) -- the frame this returns is the graded one (one
    device only).  ``hdr_path``: also writes the frame's scene-linear plane there (save_hdr; needs a grade, implies keep_hdr).
    ``passes_path``: also builds the view's ray map and writes its geometry passes and the frame's bg / disk / blur layers
    there as a compressed .npz (output.write_passes); the image itself is rendered as without it (one device, one ray per
    pixel, the texture disk source).  ``spin``: a / M of a spinning hole (HipRenderer.set_spin; one device, the texture source,
    no tilt, no anti-aliasing, no passes).  ``redshift``: "model" or "exact", the disk's g-factor of the Kerr metric
    (HipRenderer.set_redshift; the Kerr march at any spin, with a spin's restrictions).  ``observer``: the velocity beta of a
    camera that moves through ``cam_pos`` (HipRenderer.render_async; bhr_amd.observer.velocity names some), ``observer_sky``:
    whether the sky takes its Doppler factor; one device, the texture source, no anti-aliasing, no spin, no adaptive
    supersampling, no passes.  ``stars``: None, or dict(gain=, max_magnification=) -- point stars (check_stars): the sky is built
    without its baked stars, the view's ray map is built and the frame is shaded from it with the star catalogue, by the strict
    arithmetic whatever ``math`` says.  ``projection``: "equirect" or "fisheye" with ``projection_fov`` in degrees
    (HipRenderer.render_async; bhr_amd.projection): the width x height frame through that camera instead of the pinhole, ``fov``
    unused (bhr_amd.projection.frame_size is the command line's size rule); combines with ``observer`` and takes what it takes
    (check_projection).  ``light_delay``: a scale in [0, 16] -- every disk crossing shaded at the time its light left the gas
    (HipRenderer.render_async; 1 is physical); one device, the texture source, the strict Schwarzschild march of the pinhole
    camera that stands still (check_light_delay).  ``polarization``: None, or dict(field=, fraction=, cell=) -- Stokes Q / U maps
    of the disk (check_polarization): the view's ray map is built and the frame is shaded from it, the way ``stars`` does it, by the
    strict arithmetic whatever ``math`` says, with the Stokes pass behind the shade; ``stokes_path`` then takes the planes, the cell
    grid, the field, Pi_0, the convention and the camera as a compressed .npz (bhr_amd.polarization.write_stokes) and ``ticks_path``
    the frame with a polarisation tick per cell drawn over it (draw_ticks) as a PNG.  ``kerr_view``: None, or the Kerr camera of a
    spinning hole (check_kerr_view: a named or fixed velocity, the sky's shift, an equirect or fisheye projection) -- the frame is
    HipRenderer.render_async(kerr_observer=, kerr_projection=)'s.  ``kerr_stars``: None, or dict(gain=, max_magnification=) --
    point stars around a spinning hole (check_kerr_stars): the starless sky, the catalogue as the Kerr map's, a Kerr ray map of the
    view, and the still from that map -- kerr_polarization's route, with which it combines.  ``kerr_passes_path``: ``passes_path``
    for a still under a spin (check_kerr_passes): also builds the Kerr ray map of the view and writes its passes, the frame's bg /
    disk / blur layers, and the hole's spin and redshift there; the image itself is rendered as without it.  ``kerr_anti_alias``: None,
    or the LOD strength of the Kerr march's anti-aliasing (HipRenderer.set_kerr_anti_alias): ray differentials and mip LOD for a
    spinning hole's marched frame -- with supersample, the exact redshift, lens flare and a grade; not without a spin, with the Kerr
    ray map's features, the Kerr camera or several GPUs (rules.FEATURES["kerr_anti_alias"]).  ``kerr_disk_model``: "texture", or
    "v2" / "v2_volume" -- the Kerr march shades the Disk V2 model with the renderer's radii and default structure, as a surface on
    the plane or as the finite-thickness volume (HipRenderer.use_kerr_disk_v2; use_kerr_analytic_disk): with supersample, the
    exact redshift (v2), lens flare and a grade; not without a spin, with disk_model, the Kerr ray map's features, the Kerr camera,
    the Kerr anti-aliasing or several GPUs (rules.FEATURES["kerr_disk_model"]).  ``kerr_line``: dict(path=, g_map_path=, n_bins=,
    g_range=, index=, power=, emissivity=, orders=, energy_kev=) -- the disk's emission line profile and redshift map of a still under a
    spin (_checked_kerr_line): builds the Kerr ray map of the view, as kerr_passes_path does, renders the still from it with the line
    pass behind the shade, and writes the profile as a .npz and the map as a .png; kerr_polarization, kerr_stars and
    kerr_passes_path may stand beside it."""
    check_depth_and_dither(bit_depth, dither=dither)
    # the facts of this call, built once; the features are refused in this order (rules.py has what each refuses)
    f = rules.Facts(dict(
        gpus=gpus, disk_model=disk_model, disk_tilt=disk_tilt, anti_alias=anti_alias, supersample=supersample, supersample_threshold=supersample_threshold,
        spin=spin, redshift=redshift, skybox_path=skybox_path, observer=observer is not None, projection=projection is not None, projection_fov=projection_fov,
        light_delay=light_delay is not None, stars=stars is not None, polarization=polarization is not None, kerr_polarization=kerr_polarization is not None,
        kerr_stars=kerr_stars is not None, passes=passes_path is not None, passes_path=passes_path, kerr_passes_path=kerr_passes_path, stokes_path=stokes_path,
        ticks_path=ticks_path, kerr_anti_alias=kerr_anti_alias is not None, kerr_disk_model=kerr_disk_model, **_kerr_view_facts(kerr_view),
        **_kerr_line_facts(kerr_line)))
    kerr_disk_model = _checked_kerr_disk_model(kerr_disk_model, f)      # ahead of the rest, so that each refusal names --spin_disk_model
    kerr_view = checked("kerr_view", kerr_view, f)
    if kerr_view is not None:                                  # refused ahead of any device work, like the rest
        kerr_view_beta(kerr_view, cam_pos, spin)
    checked("light_delay", light_delay, f)
    checked("projection", projection, f)
    stars = checked("stars", stars, f)
    checked("observer", observer, f)
    rules.refuse_on("passes", f)
    # ``kerr_polarization``: the same dict for a spinning hole (check_kerr_polarization): the view's KERR ray map is built with the
    # photon momenta and the frame is shaded from it, the Kerr Stokes pass behind the shade; stokes_path and ticks_path serve it too
    kerr_polarization = checked("kerr_polarization", kerr_polarization, f)
    if kerr_polarization is None:
        polarization = checked("polarization", polarization, f)
    grade = f["grade"] = check_grade(grade)
    if hdr_path is not None:
        check_hdr_path(hdr_path)
        if grade is None:
            raise ValueError("hdr_path needs a grade: the HDR plane is written by the grading stage (tonemap 'clip' keeps the picture as it is)")
        grade["keep_hdr"] = True
    rules.refuse_on("tiles spin", f)
    # the Kerr point stars and the Kerr passes, behind every refusal above: each names --spin_stars / --spin_passes and the other flag
    kerr_stars = checked("kerr_stars", kerr_stars, f)
    rules.refuse_on("kerr_passes", f)
    kerr_anti_alias = _checked_kerr_anti_alias(kerr_anti_alias, f)
    kerr_line = _checked_kerr_line(kerr_line, f)
    if gpus > 1:
        from .multigpu import render_image_tiled
        return render_image_tiled(width, height, cam_pos, fov, gpus, step_size=step_size, skybox_path=skybox_path,
                                  n_stars=n_stars, tex_w=tex_w, tex_h=tex_h, r_max=r_max,
                                  disk_texture_path=disk_texture_path, r_disk_inner=r_disk_inner,
                                  r_disk_outer=r_disk_outer, disk_tilt=disk_tilt, lens_flare=lens_flare,
                                  anti_alias=anti_alias, aa_strength=aa_strength,
                                  disk_rotation_speed=disk_rotation_speed, disk_model=disk_model, math=math)
    renderer, use_lifecycle, n_r, n_phi = make_renderer(
        width, height, cam_pos, fov, step_size, skybox_path, n_stars, tex_w, tex_h, r_max, disk_texture_path,
        r_disk_inner, r_disk_outer, disk_tilt, lens_flare, anti_alias, aa_strength, disk_rotation_speed, math=math,
        supersample=supersample, supersample_threshold=supersample_threshold, spin=spin,
        **({"redshift": redshift} if redshift != "model" else {}), **({} if stars is None else {"stars": stars}),
        **({} if kerr_stars is None else {"kerr_stars": kerr_stars}))
    if use_analytic_disk(renderer, disk_model) or use_kerr_analytic_disk(renderer, kerr_disk_model):
        pass
    elif use_lifecycle:
        factories = init_lifecycle_system(renderer, n_r, n_phi, seed=42)
        advance_lifecycle_frame(renderer, factories, t=0.0, dt=0.0, recompute_stats=True)
    t0 = time.time()
    print(f"HIP: {width}x{height}, cam_pos={list(cam_pos)}, fov={fov}°, step_size={step_size}")
    if grade is not None:
        renderer.set_grade(**grade)
    if kerr_anti_alias is not None:
        renderer.set_kerr_anti_alias(True, kerr_anti_alias)
    if polarization is not None:
        renderer.set_polarization(**polarization)          # ahead of the frame: its Stokes pass rides behind the shade launch
    if kerr_polarization is not None or kerr_stars is not None or kerr_line is not None:
        from . import _lib
        if kerr_polarization is not None:
            renderer.set_kerr_polarization(**kerr_polarization)   # ahead of the build: the map then keeps the photon momenta
        if kerr_line is not None:                                 # the line pass rides behind the shade launch; the planes feed the map
            renderer.set_kerr_line(samples=kerr_line["g_map_path"] is not None, **kerr_line["settings"])
        renderer.build_kerr_ray_map(cam_pos, fov)
        renderer.render_from_kerr_ray_map_async(frame=0)
        img = renderer.read_layer(_lib.LAYER_FINAL)
        polarization = kerr_polarization                       # the outputs below are the same
        if kerr_line is not None:
            _save_kerr_line(renderer, kerr_line)
            if kerr_line["g_map_path"] is not None:
                from . import line as line_mod
                line_mod.save_g_map(kerr_line["g_map_path"], renderer.kerr_line_samples()["g"])
                print(f"Saved: {kerr_line['g_map_path']}")
    elif stars is not None or polarization is not None:
        from . import _lib
        renderer.build_ray_map(cam_pos, fov)
        renderer.render_from_ray_map_async(frame=0)
        img = renderer.read_layer(_lib.LAYER_FINAL)
    elif kerr_view is not None:
        img = renderer.render(cam_pos, fov, frame=0, **_kerr_view_kw(kerr_view, kerr_view_beta(kerr_view, cam_pos, spin)))
    else:
        img = renderer.render(cam_pos, fov, frame=0, observer=observer, observer_sky=observer_sky, projection=projection,
                              projection_fov=projection_fov, light_delay=light_delay)
    for label, si in (("Point stars", stars and renderer.stars_info()), ("Kerr point stars", kerr_stars and renderer.kerr_stars_info())):
        if si:
            print(f"{label}: {si['n']} stars, {si['images']} images, {si['capped']} triangles capped at magnification "
                  f"{si['max_magnification']:g}, {si['skipped_span']} over the span")
    if polarization is not None:
        from . import polarization as pol_mod
        planes, cells = renderer.stokes(), renderer.stokes_cells()
        deg, _ = pol_mod.degree_and_angle(cells[..., 0], cells[..., 1], cells[..., 2])
        print(f"Polarization: field {polarization['field']}, fraction {polarization['fraction']:g}, {cells.shape[1]} x {cells.shape[0]} cells of "
              f"{polarization['cell']} pixels, largest cell degree {float(deg.max()) if deg.size else 0.0:.3f}")
        if stokes_path is not None:
            pol_mod.write_stokes(stokes_path, cells, polarization["cell"], polarization["field"], polarization["fraction"],
                                 camera=dict(cam_pos=list(cam_pos), fov=fov), stokes=planes,
                                 **({} if kerr_polarization is None else {"hole": dict(spin=spin, redshift=redshift)}))
            print(f"Saved: {stokes_path}")
        if ticks_path is not None:
            from .output import png_write, quantize
            png_write(ticks_path, pol_mod.draw_ticks(quantize(img), cells, polarization["cell"]))
            print(f"Saved: {ticks_path}")
    if hdr_path is not None:
        save_hdr(renderer.read_hdr(), hdr_path)
    c = renderer.counters()
    if passes_path is not None or kerr_passes_path is not None:          # (the checks have refused both at once: the passes of one map)
        from . import _lib
        layers = {"bg": renderer.read_layer(_lib.LAYER_BG), "disk": renderer.read_layer(_lib.LAYER_DISK),
                  "blur": renderer.read_layer(_lib.LAYER_BLUR)}
        if passes_path is not None:
            renderer.build_ray_map(cam_pos, fov)
            passes, info, hole, label = renderer.ray_map_passes(), renderer.ray_map_info(), {}, "ray map"
        else:
            if not renderer.kerr_ray_map_info()["built"]:      # (a still with Kerr point stars or a Kerr polarisation came from the view's map)
                renderer.build_kerr_ray_map(cam_pos, fov)
            info, passes = renderer.kerr_ray_map_info(), renderer.kerr_ray_map_passes()
            hole, label = {"hole": dict(spin=info["spin"], redshift=info["redshift"])}, f"Kerr ray map, spin {info['spin']:g}, {info['redshift']} redshift"
        path = passes_path if passes_path is not None else kerr_passes_path
        write_passes(path, passes, layers, **hole)
        print(f"Saved: {path} ({label}: {info['slots']} slots, {info['crossings_stored']} crossings, "
              f"{info['overflow_pixels']} overflow pixels)")
    dt = time.time() - t0
    print(f"Done in {dt:.3f}s  (march {c['march_ms']:.2f} ms, bloom {c['bloom_ms']:.2f} ms, "
          f"{c['ray_steps'] / 1e6:.1f} Mray-steps, {c['ray_steps'] / max(c['march_ms'], 1e-6) / 1e3:.0f} Mray-steps/s)")
    renderer.close()
    return img


# ---- what may be rendered together --------------------------------------------------------------------------------------------------------
# Every check_* below validates its feature's own value (_VALID) and then asks rules.py for the feature's refusals, with its keywords as
# the facts; render_image and render_video build their facts once and go through checked() in their own order.  All of it raises
# ValueError, naming the combination, before any device work.
def _valid_points(who: str, gain: str, magnification: str):
    def valid(points, f):
        if points is None:
            return None
        from .stars import DEFAULT_MAX_MAGNIFICATION, DEFAULT_STAR_GAIN
        out = {"gain": DEFAULT_STAR_GAIN, "max_magnification": DEFAULT_MAX_MAGNIFICATION}
        unknown = set(points) - set(out)
        if unknown:
            raise ValueError(f"{who} takes gain and max_magnification, got {sorted(unknown)}")
        out.update(points)
        if not (out["gain"] > 0 and np.isfinite(out["gain"])):
            raise ValueError(f"{gain} must be greater than 0, got {out['gain']}")
        if not 1.0 <= out["max_magnification"] <= 1e6:
            raise ValueError(f"{magnification} must be between 1 and 1e6, got {out['max_magnification']}")
        return out
    return valid


def _valid_stokes(who: str):
    def valid(polarization, f):
        if polarization is None:
            if who == "polarization" and (f["stokes_path"] is not None or f["ticks_path"] is not None):
                raise ValueError("stokes_output and polarization_ticks need a polarization: they are its outputs")
            return None
        from .polarization import DEFAULT_CELL, DEFAULT_FRACTION, check
        unknown = set(polarization) - {"field", "fraction", "cell"}
        if unknown or "field" not in polarization:
            raise ValueError(f"{who} takes field, fraction and cell, got {sorted(polarization)}")
        return check(polarization["field"], polarization.get("fraction", DEFAULT_FRACTION), polarization.get("cell", DEFAULT_CELL))
    return valid


def _valid_observer(observer, f):
    from .observer import check_beta
    return None if observer is None else check_beta(observer)


def _valid_projection(projection, f):
    if projection is None:
        if f["projection_fov"] is not None:
            raise ValueError("projection_fov needs a projection: it is the field of view of an equirect or fisheye camera")
        return None
    from .projection import check
    return check(projection, f["projection_fov"])


def _valid_light_delay(scale, f):
    if scale is None:
        return None
    try:
        out = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"light_delay is a scale in [0, 16], got {scale!r}") from None
    if not 0.0 <= out <= 16.0:            # a NaN fails the comparison too
        raise ValueError(f"light_delay is a scale in [0, 16], got {scale!r}")
    return out


def _valid_kerr_view(kerr_view, f):
    if kerr_view is None:
        return None
    from . import observer as obs_mod
    unknown = set(kerr_view) - {"observer", "velocity", "sky", "projection", "projection_fov"}
    if unknown:
        raise ValueError(f"kerr_view takes observer, velocity, sky, projection and projection_fov, got {sorted(kerr_view)}")
    out = dict(observer=kerr_view.get("observer"), velocity=kerr_view.get("velocity"), sky=kerr_view.get("sky"),
               projection=kerr_view.get("projection"), projection_fov=kerr_view.get("projection_fov"))
    if out["observer"] is not None and out["velocity"] is not None:
        raise ValueError("--spin_observer names a velocity and --spin_observer_velocity gives one: take one of the two")
    if out["observer"] == "infall":
        raise ValueError("--spin_observer infall is not offered: the free fall from rest at infinity is not radial around a spinning hole "
                         f"(one of {obs_mod.KERR_KINDS})")
    if out["observer"] is not None and out["observer"] not in obs_mod.KERR_KINDS:
        raise ValueError(f"--spin_observer must be one of {obs_mod.KERR_KINDS}, got {out['observer']!r}")
    if out["sky"] is not None and out["observer"] is None and out["velocity"] is None:
        raise ValueError("--spin_observer_sky needs --spin_observer or --spin_observer_velocity: it belongs to a camera that moves")
    out["sky"] = obs_mod.check_sky("shift" if out["sky"] is None else out["sky"])
    if out["velocity"] is not None:
        out["velocity"] = obs_mod.check_beta(out["velocity"])
    if out["projection"] is None and out["projection_fov"] is not None:
        raise ValueError("--spin_projection_fov needs --spin_projection equirect or fisheye: it is the field of view of that camera")
    if out["projection"] is not None:
        from .projection import check
        _, fov_h, fov_v = check(out["projection"], out["projection_fov"])
        out["projection_fov"] = (fov_h, fov_v) if out["projection"] == "equirect" else (fov_h,)
    if out["observer"] is None and out["velocity"] is None and out["projection"] is None:
        raise ValueError("kerr_view needs an observer, a velocity or a projection")
    return out


_VALID = {
    "stars": _valid_points("stars", "star gain", "star max_magnification"),
    "kerr_stars": _valid_points("--spin_stars", "--spin_stars: --star_gain", "--spin_stars: --star_max_magnification"),
    "polarization": _valid_stokes("polarization"), "kerr_polarization": _valid_stokes("--spin_polarization"),
    "observer": _valid_observer, "projection": _valid_projection, "light_delay": _valid_light_delay, "kerr_view": _valid_kerr_view,
}


def _checked_kerr_anti_alias(strength, facts):
    """The LOD strength of the Kerr anti-aliasing as render_image / render_video take it, or None: finite and not negative, and what
    rules.FEATURES["kerr_anti_alias"] refuses is refused."""
    if strength is None:
        return None
    strength = float(strength)
    if not (strength >= 0.0 and np.isfinite(strength)):
        raise ValueError(f"--spin_aa_strength is finite and not negative, got {strength}")
    rules.refuse("kerr_anti_alias", facts)
    return strength


def checked(feature: str, value, facts, surface: str = "api"):
    """A feature's value checked -> the value with its defaults filled in, or None without one (nothing is refused then): its own
    validation, then the feature's refusals of rules.FEATURES against ``facts`` (a dict of rules.FACTS, or a rules.Facts)."""
    f = facts if isinstance(facts, rules.Facts) else rules.Facts(facts)
    out = _VALID[feature](value, f)
    if value is not None:
        rules.refuse(feature, f, surface)
    return out


def check_stars(stars, skybox_path=None, supersample=1, spin: float = 0.0, redshift: str = "model", gpus: int = 1,
                disk_model: str = "texture", observer=None):
    """--stars point / stars=dict(gain=, max_magnification=): the procedural sky's stars as a catalogue of lensed points rendered
    through a ray map.  -> the dict with its defaults filled in, or None.  (``observer``: the camera's velocity, or None.)"""
    return checked("stars", stars, dict(locals(), observer=observer is not None))


def check_kerr_stars(kerr_stars, spin: float = 0.0, redshift: str = "model", skybox_path=None, stars: bool = False, supersample=1,
                     spin_map_supersample: int = 1, spin_shutter_map: bool = False, shutter: float = 0.0, spin_observer: bool = False,
                     spin_projection: bool = False, gpus: int = 1, world: int = 1, video: bool = False, spin_map: bool = False):
    """--spin_stars point / kerr_stars=dict(gain=, max_magnification=): the procedural sky's stars as a catalogue of lensed points
    rendered through the KERR ray map of a spinning hole (HipRenderer.set_kerr_stars).  -> the dict with its defaults filled in,
    or None.  It needs a spin or the exact redshift (the Kerr march); a still builds a Kerr ray map of the view, a video needs
    spin_map."""
    return checked("kerr_stars", kerr_stars, locals())


def check_kerr_passes(kerr_passes_path, spin: float = 0.0, redshift: str = "model", supersample=1, spin_observer: bool = False,
                      spin_projection: bool = False, gpus: int = 1, video: bool = False) -> None:
    """--spin_passes PATH.npz / kerr_passes_path: the geometry passes of a still under a spin, from a Kerr ray map of the view."""
    if kerr_passes_path is not None:
        rules.refuse("kerr_passes", locals())


def check_observer(observer, anti_alias="disabled", disk_model: str = "texture", supersample_threshold=None, gpus: int = 1,
                   world: int = 1, spin: float = 0.0, redshift: str = "model", passes: bool = False, shutter: float = 0.0,
                   maps: bool = False) -> None:
    """What a frame of a moving observer takes: a velocity within |beta| <= 0.995 and what rules.FEATURES["observer"] does not
    refuse (an observer takes any ``world``: frame-sharded observer videos are legal).  None: the camera stands still and nothing
    is checked."""
    checked("observer", observer, locals())


def check_projection(projection, projection_fov=None, anti_alias="disabled", disk_model: str = "texture", supersample_threshold=None,
                     gpus: int = 1, world: int = 1, spin: float = 0.0, redshift: str = "model", passes: bool = False, shutter: float = 0.0,
                     maps: bool = False, stars: bool = False):
    """What a frame under a projection takes (bhr_amd.projection.check: "equirect" or "fisheye" and its angles) -- the observer
    march's terms.  -> (kind, fov_h, fov_v), or None without a projection (``projection_fov`` alone is an error)."""
    return checked("projection", projection, locals())


def check_light_delay(scale, anti_alias="disabled", disk_model: str = "texture", supersample_threshold=None, gpus: int = 1,
                      world: int = 1, spin: float = 0.0, redshift: str = "model", observer: bool = False, projection: bool = False,
                      passes: bool = False, shutter: float = 0.0, maps: bool = False, stars: bool = False):
    """What a frame with light delay takes: a scale in [0, 16], one device and one rank, the strict Schwarzschild march of the
    pinhole camera that stands still.  -> the scale as a float, or None without one (nothing is checked)."""
    return checked("light_delay", scale, locals())


def check_kerr_view(kerr_view, spin: float = 0.0, redshift: str = "model", disk_tilt: float = 0.0, anti_alias="disabled",
                    disk_model: str = "texture", supersample_threshold=None, gpus: int = 1, observer: bool = False, projection: bool = False,
                    light_delay: bool = False, passes: bool = False, shutter: float = 0.0, maps: bool = False, stars: bool = False,
                    spin_map: bool = False):
    """kerr_view=dict(observer=, velocity=, sky=, projection=, projection_fov=): the Kerr camera of a spinning hole (--spin_observer
    and its companions) -> the dict with its defaults filled in, or None without one.  ``observer``: "static", "circular" or
    "zamo" (bhr_amd.observer.kerr_velocity) or ``velocity``: a fixed beta, one of the two at most; ``sky``: "shift" (default) or
    "plain"; ``projection``: "equirect" or "fisheye" with ``projection_fov`` (bhr_amd.projection.check).  It needs a spin or the
    exact redshift and takes what the Kerr march takes, on one GPU, marched (``spin_map``: a Kerr ray map or a Kerr polarisation)."""
    return checked("kerr_view", kerr_view, dict(locals(), kerr_map=spin_map))


def _kerr_view_facts(kerr_view) -> dict:
    """The Kerr camera as the rules see it: one that moves, or one with a projection (which may move as well)."""
    return dict(spin_observer=kerr_view is not None and kerr_view.get("projection") is None,
                spin_projection=kerr_view is not None and kerr_view.get("projection") is not None)


def kerr_view_beta(kerr_view: dict, pos, spin: float):
    """The velocity of the Kerr camera ``kerr_view`` (check_kerr_view's dict) at ``pos``: its fixed one, its named one evaluated
    there, or None for a camera without either (a projection at rest)."""
    from . import observer as obs_mod
    if kerr_view["velocity"] is not None:
        return tuple(kerr_view["velocity"])
    if kerr_view["observer"] is not None:
        return tuple(float(v) for v in obs_mod.kerr_velocity(kerr_view["observer"], pos, spin))
    return None


def _kerr_view_kw(kerr_view: dict, beta) -> dict:
    """HipRenderer.render_async's keywords of one frame of the Kerr camera moving with ``beta`` (None: the call without a velocity)."""
    return dict(kerr_observer=beta, kerr_observer_sky=kerr_view["sky"] == "shift", kerr_projection=kerr_view["projection"],
                kerr_projection_fov=kerr_view["projection_fov"])


def check_passes(passes_path, gpus: int = 1, supersample: int = 1, disk_model: str = "texture") -> None:
    """What a still image with geometry passes takes: a .npz path, one device, one ray per pixel, the texture source."""
    if passes_path is not None:
        rules.refuse("passes", locals())


def check_polarization(polarization, video: bool = False, ray_map: bool = False, orbit_map: bool = False, shutter_map: bool = False,
                       shutter: float = 0.0, supersample=1, map_supersample: int = 1, disk_model: str = "texture", gpus: int = 1,
                       world: int = 1, spin: float = 0.0, redshift: str = "model", observer: bool = False, projection: bool = False,
                       light_delay: bool = False, stokes_path=None, ticks_path=None):
    """polarization=dict(field=, fraction=, cell=) (bhr_amd.polarization.check: a preset or three numbers, Pi_0 in [0, 1], a cell
    of 8, 16 or 32 pixels): Stokes Q / U maps of the disk, computed through a ray map of the view.  -> the dict with its defaults
    filled in, or None without one (``stokes_path`` / ``ticks_path`` alone are an error)."""
    return checked("polarization", polarization, locals())


def check_kerr_polarization(kerr_polarization, polarization: bool = False, video: bool = False, spin_map: bool = False, orbit: bool = False,
                            spin: float = 0.0, redshift: str = "model", shutter: float = 0.0, supersample=1, supersample_threshold=None,
                            map_supersample=1, gpus: int = 1, world: int = 1, disk_model: str = "texture", ray_map: bool = False,
                            orbit_map: bool = False, shutter_map: bool = False, observer: bool = False, projection: bool = False,
                            light_delay: bool = False, stars: bool = False, passes: bool = False, stokes_path=None, ticks_path=None):
    """kerr_polarization=dict(field=, fraction=, cell=): Stokes Q / U maps of the disk of a SPINNING hole, carried along each ray
    by the Walker-Penrose constant (--spin_polarization; HipRenderer.set_kerr_polarization) -> the dict with its defaults filled
    in, or None without one.  It needs a spin or the exact redshift (the Kerr march); a still builds a Kerr ray map of the view,
    a video needs spin_map and a camera that stands still."""
    return checked("kerr_polarization", kerr_polarization, locals())


def check_ray_map(ray_map: bool, orbit: bool = False, shutter: float = 0.0, supersample=1, disk_model: str = "texture",
                  gpus: int = 1, world: int = 1) -> None:
    """What a video from a ray map takes: a camera that stands still, an instantaneous exposure, one ray per pixel, the
    texture disk source, one GPU."""
    if ray_map:
        rules.refuse("ray_map", locals())


def check_orbit_map(orbit_map: bool, video: bool = True, orbit: bool = True, ray_map: bool = False, disk_tilt: float = 0.0,
                    shutter: float = 0.0, supersample=1, disk_model: str = "texture", gpus: int = 1, world: int = 1) -> None:
    """What an orbit video from ONE ray map takes: --video --orbit, a disk that is not tilted (the orbit's turn about z is then
    a symmetry of everything a ray's path depends on), an instantaneous exposure, one ray per pixel, the texture disk source,
    one GPU -- and not --ray_map, which is the map of a camera that stands still."""
    if orbit_map:
        rules.refuse("orbit_map", locals())


def check_shutter_map(shutter_map: bool, shutter: float = 0.5, orbit: bool = False, ray_map: bool = False, orbit_map: bool = False,
                      disk_tilt: float = 0.0, supersample=1, disk_model: str = "texture", gpus: int = 1, world: int = 1) -> None:
    """What a motion-blurred video from ONE ray map takes: an open shutter, one ray per pixel, the texture disk source, one GPU,
    and under --orbit a disk that is not tilted (a camera that stands still takes any disk) -- and neither --ray_map nor
    --orbit_map, which are the maps of instantaneous exposures."""
    if shutter_map:
        rules.refuse("shutter_map", locals())


def check_spin_map(spin_map: bool, spin: float = 0.0, redshift: str = "model", video: bool = True, shutter: float = 0.0, supersample=1,
                   map_supersample=1, gpus: int = 1, world: int = 1, ray_map: bool = False, orbit_map: bool = False, shutter_map: bool = False,
                   observer: bool = False, projection: bool = False, light_delay: bool = False, stars: bool = False,
                   polarization: bool = False) -> None:
    """--spin_map is the Kerr ray map of a video (render_video): one march of a spinning hole's view, every frame shaded from it
    -- under --orbit turned about the spin axis to the frame's camera.  It needs a spin or the exact redshift (the Kerr march),
    a video, an instantaneous exposure, one ray per pixel and one GPU, and none of the Schwarzschild maps or of what a spin
    refuses anyway."""
    if spin_map:
        rules.refuse("spin_map", locals())


def check_spin_shutter_map(spin_shutter_map: bool, spin: float = 0.0, redshift: str = "model", video: bool = True, shutter: float = 0.5,
                           spin_map: bool = False, ray_map: bool = False, orbit_map: bool = False, shutter_map: bool = False, supersample=1,
                           map_supersample=1, spin_polarization: bool = False, spin_observer: bool = False, spin_projection: bool = False,
                           observer: bool = False, projection: bool = False, light_delay: bool = False, stars: bool = False,
                           polarization: bool = False, gpus: int = 1, world: int = 1) -> None:
    """--spin_shutter_map is motion blur from ONE Kerr ray map (render_video): a spinning hole's view marched once, every sample of
    every exposure shaded from it -- the disk's roll and, under --orbit, the camera's turn about the spin axis are what the map
    leaves free.  It needs a spin or the exact redshift (the Kerr march), a video, an open shutter, one ray per pixel of the
    context (--spin_map_supersample is the map's own factor) and one GPU."""
    if spin_shutter_map:
        rules.refuse("spin_shutter_map", dict(locals(), kerr_polarization=spin_polarization))


# A video's map as render_video drives it: per mode the build of its one map, with the line it prints, the frame from it and the
# free.  fr: the frame's camera and, under a shutter, its samples.  (The build view needs no entry: frame 0 of the orbit under
# ``orbit``, else the camera that stands still -- ray_map has no orbit and orbit_map always one, by their checks.)
def _build_map(label: str):
    def build(renderer, cam_pos, fov, map_supersample):
        renderer.build_ray_map(cam_pos, fov, supersample=map_supersample)
        info = renderer.ray_map_info()
        print(f"  {label} built: {info['slots']} slots, {info['overflow_pixels']} overflow pixels, {info['device_bytes'] / 1e6:.0f} MB")
    return build


def _build_kerr_map(renderer, cam_pos, fov, map_supersample):
    # (map_supersample: the Kerr map's own factor, render_video's spin_map_supersample)
    if map_supersample == 1:
        renderer.build_kerr_ray_map(cam_pos, fov)
    else:
        renderer.build_kerr_ray_map(cam_pos, fov, supersample=map_supersample)
    info = renderer.kerr_ray_map_info()
    factor = "" if map_supersample == 1 else f"{map_supersample} x {map_supersample} rays per pixel, "
    print(f"  Kerr ray map built (spin {info['spin']:g}, {info['redshift']} redshift): {factor}{info['slots']} slots, {info['overflow_pixels']} overflow pixels, "
          f"{info['device_bytes'] / 1e6:.0f} MB")


_MAP_MODES = {
    # the same frame from the map: shade, no march
    "ray_map": dict(build=_build_map("ray map"), free="free_ray_map", frame=lambda r, fr: r.render_from_ray_map_async(frame=0)),
    # the map turned to the frame's camera
    "orbit_map": dict(build=_build_map("orbit ray map"), free="free_ray_map",
                      frame=lambda r, fr: r.render_from_ray_map_async(frame=0, cam_pos=fr["cam_pos"], fov=fr["fov"])),
    # the marched shutter loop's samples from the map
    "shutter_map": dict(build=_build_map("shutter ray map"), free="free_ray_map",
                        frame=lambda r, fr: r.render_shutter_from_ray_map_async(fr["t_offsets"], fr["positions"] if fr["orbit"] else None, fr["fov"])),
    # the Kerr map; an orbit frame turned to its camera
    "spin_map": dict(build=_build_kerr_map, free="free_kerr_ray_map",
                     frame=lambda r, fr: r.render_from_kerr_ray_map_async(frame=0, cam_pos=fr["cam_pos"] if fr["orbit"] else None)),
    # the marched shutter loop's samples from the Kerr map
    "spin_shutter_map": dict(build=_build_kerr_map, free="free_kerr_ray_map",
                             frame=lambda r, fr: r.render_shutter_from_kerr_ray_map_async(fr["t_offsets"], fr["positions"] if fr["orbit"] else None, fr["fov"])),
}


def _lib_max_png_width(bit_depth: int = 8) -> int:
    from . import _lib
    lib = _lib.load()
    return int(lib.bhr_png16_device_max_width() if bit_depth == 16 else lib.bhr_png_device_max_width())


def _frames_dir(output_path: str) -> str:
    name = ".frames_" + hashlib.md5(output_path.encode()).hexdigest()[:16]
    return os.path.join(os.path.dirname(output_path), name)


VIDEO_CODECS = ("auto", "mjpeg")


def assemble_video(temp_dir: str, n_frames: int, fps: int, output_path: str, codec: str = "auto", spherical: bool = False) -> bool:
    """Frames -> MP4.  ``codec="mjpeg"``: the frame_%04d.jpg files of render_video(video_codec="mjpeg") become the samples
    of a Motion-JPEG track as they are (mp4.write_jpeg_mp4, object type 0x6C); nothing is re-coded and no external
    encoder is looked for.  ``codec="auto"``:
    PNG frames -> MP4 (render.py:4497-4503: libx264 through imageio's pyav plugin).  In order of preference: imageio +
    pyav as the reference; an ``ffmpeg`` binary on PATH (same codec, same pixel format); failing both, the frames
    themselves muxed into an MP4 as PNG-coded samples (mp4.write_png_mp4: lossless, plays in ffmpeg / mpv / VLC, and is one
    ffmpeg call away from the H.264 file).  Returns False only when a frame is missing.  ``spherical``: the frames are
    full-sphere equirectangular panoramas -- where this module's own muxer writes the file (Motion-JPEG, PNG-in-MP4) the video
    track gets the Spherical Video V1 box and players open it as a 360-degree video; the pyav and ffmpeg routes write no such
    metadata."""
    if codec not in VIDEO_CODECS:
        raise ValueError(f"codec must be one of {VIDEO_CODECS}, got {codec!r}")
    ext = ".jpg" if codec == "mjpeg" else ".png"
    frames = [os.path.join(temp_dir, f"frame_{frame:04d}{ext}") for frame in range(n_frames)]
    missing = [p for p in frames if not os.path.isfile(p)]
    if missing:
        print(f"{len(missing)} of {n_frames} frames are missing (first: {missing[0]}): no video assembled")
        return False
    if codec == "mjpeg":
        from .mp4 import jpeg_size, write_jpeg_mp4
        w, h = jpeg_size(frames[0])
        nbytes = write_jpeg_mp4(frames, fps, output_path, w, h, **({"spherical": True} if spherical else {}))
        print(f"Video saved: {output_path} ({n_frames} JPEG-coded frames, {nbytes / 1e6:.0f} MB, Motion-JPEG in MP4)")
        return True
    try:
        import imageio.v3 as iio
        import av  # noqa: F401
    except ImportError:
        iio = None
    if iio is not None:
        writer = iio.imopen(output_path, "w", plugin="pyav")
        writer.init_video_stream("libx264", fps=fps)
        for p in frames:
            writer.write_frame(iio.imread(p))
        writer.close()
        print(f"Video saved: {output_path}")
        return True
    if shutil.which("ffmpeg"):
        import subprocess
        rc = subprocess.call(["ffmpeg", "-y", "-loglevel", "error", "-framerate", str(fps), "-i", os.path.join(temp_dir, "frame_%04d.png"),
                              "-c:v", "libx264", "-crf", "18", "-pix_fmt", "yuv420p", output_path])
        if rc == 0:
            print(f"Video saved: {output_path}")
            return True
        print(f"ffmpeg failed ({rc}) on the PNG frames; writing them into the MP4 as they are")
    from .mp4 import png_size, write_png_mp4
    w, h = png_size(frames[0])
    nbytes = write_png_mp4(frames, fps, output_path, w, h, **({"spherical": True} if spherical else {}))
    print(f"Video saved: {output_path} ({n_frames} PNG-coded frames, {nbytes / 1e6:.0f} MB, lossless; no H.264 encoder in this "
          f"environment -- re-code with: ffmpeg -i {output_path} -c:v libx264 -crf 18 -pix_fmt yuv420p out.mp4)")
    return True


SHUTTER_MAX_SAMPLES = 64


def shutter_times(frame, shutter: float, n: int) -> List[float]:
    """The n fractional frame numbers at which frame ``frame`` is sampled under a shutter open for ``shutter`` of a frame
    time: u_j = frame + shutter * ((j + 0.5) / n - 0.5), the midpoints of n equal parts of the exposure, in binary64.  They
    are centred on the frame (n = 1 is the frame itself) and span shutter * (n - 1) / n."""
    return [float(frame) + float(shutter) * ((j + 0.5) / n - 0.5) for j in range(n)]


def check_shutter(shutter, shutter_samples) -> None:
    if isinstance(shutter, bool) or not isinstance(shutter, (int, float)) or not (0.0 <= shutter <= 1.0):
        raise ValueError(f"shutter must be between 0 and 1 (the share of the frame time the shutter is open), got {shutter!r}")
    if isinstance(shutter_samples, bool) or not isinstance(shutter_samples, int) or not (1 <= shutter_samples <= SHUTTER_MAX_SAMPLES):
        raise ValueError(f"shutter_samples must be an integer between 1 and {SHUTTER_MAX_SAMPLES}, got {shutter_samples!r}")


def check_map_supersample(k, ray_map: bool = False, orbit_map: bool = False, shutter_map: bool = False) -> None:
    """--map_supersample k / render_video(map_supersample=k): the ray map's own supersampling factor (k x k records per
    pixel, resolved in the shade).  1, 2, 4 or 8, and above 1 only with one of the three maps.  Raises ValueError before any
    device work."""
    if isinstance(k, bool) or not isinstance(k, int) or k not in (1, 2, 4, 8):
        raise ValueError(f"map_supersample must be 1, 2, 4 or 8, got {k!r}")
    rules.refuse_on("map_supersample", rules.Facts(dict(locals(), map_supersample=k)))


def check_spin_map_supersample(k, spin_map: bool = False, spin_polarization: bool = False, spin_shutter_map: bool = False) -> None:
    """--spin_map_supersample k / render_video(spin_map=True, spin_map_supersample=k): the Kerr ray map's own supersampling
    factor (k x k records per pixel, resolved in the shade; HipRenderer.build_kerr_ray_map(supersample=k)).  1, 2, 4 or 8, above
    1 only with --spin_map or --spin_shutter_map (whose samples are then resolved one by one, ahead of the mean) and not with
    --spin_polarization (the Stokes planes need a map with one ray per pixel).  Raises ValueError naming both flags, before any
    device work."""
    if isinstance(k, bool) or not isinstance(k, int) or k not in (1, 2, 4, 8):
        raise ValueError(f"spin_map_supersample must be 1, 2, 4 or 8, got {k!r}")
    rules.refuse_on("spin_map_supersample", rules.Facts(dict(locals(), spin_map_supersample=k, kerr_polarization=spin_polarization)))


VIDEO_HDRS = ("pq", "hlg")
HDR_COLOR_TRC = {"pq": "smpte2084", "hlg": "arib-std-b67"}     # ffmpeg's names of the two transfers


def check_video_hdr(video_hdr, hdr_white=203.0, hdr_exposure=0.0, width: int = 2, height: int = 2, world: int = 1,
                    video_codec: str = "auto", video_stream: str = "auto"):
    """What an HDR video stream takes (render_video(video_hdr=...)): "pq" or "hlg", a white level in (0, 10000] nits (PQ) and an
    exposure of -16 .. 16 stops, even frame sizes, one rank, PNG frames (not video_codec="mjpeg") and a stream to write
    (not video_stream="off").  Returns None without ``video_hdr``, else the ``hdr`` dict of output.Y4MStream.  Raises ValueError
    before any device work."""
    if video_hdr is None:
        return None
    if video_hdr not in VIDEO_HDRS:
        raise ValueError(f"video_hdr must be one of {VIDEO_HDRS}, got {video_hdr!r}")
    from .output import check_hdr
    hdr = check_hdr(dict(transfer=video_hdr, exposure=hdr_exposure, white_nits=hdr_white))
    rules.refuse("video_hdr", locals())
    return hdr


def hdr_ffmpeg_args(video_hdr: str, output_path: str) -> List[str]:
    """The command that encodes the HDR stream from its standard input: HEVC Main 10 with the stream's colour description
    (BT.2020 primaries, PQ or HLG transfer, BT.2020 non-constant-luminance matrix, limited range) signalled in the file."""
    if video_hdr not in VIDEO_HDRS:
        raise ValueError(f"video_hdr must be one of {VIDEO_HDRS}, got {video_hdr!r}")
    return ["ffmpeg", "-y", "-loglevel", "error", "-f", "yuv4mpegpipe", "-i", "-", "-c:v", "libx265", "-pix_fmt", "yuv420p10le",
            "-color_primaries", "bt2020", "-color_trc", HDR_COLOR_TRC[video_hdr], "-colorspace", "bt2020nc", "-color_range", "tv",
            output_path]


def hdr_sidecar(hdr: dict, max_cll: float, max_fall: float, frames: int) -> dict:
    """The record written beside an HDR stream (``<output stem>.hdr10.json``): what a remux step needs to signal the stream's
    colour description and, for PQ, its content light levels, which are known only once the last frame is written."""
    return {"transfer": hdr["transfer"], "white_nits": hdr["white_nits"], "exposure": hdr["exposure"], "primaries": "bt2020",
            "matrix": "bt2020nc", "range": "limited", "max_cll": max_cll, "max_fall": max_fall, "frames": frames}


def progress_params(n_frames, fov, orbit, disk_rotation_speed, orbit_degrees, video_codec="auto", video_quality=90,
                    bit_depth=8, dither="none", shutter=0.0, shutter_samples=8, grade=None, ray_map=False, orbit_map=False,
                    shutter_map=False, map_supersample=1, video_hdr=None, hdr_white=203.0, hdr_exposure=0.0, observer=None,
                    stars=None, projection=None, light_delay=None, polarization=None, spin_map=False, kerr_view=None,
                    spin_map_supersample=1, spin_shutter_map=False, kerr_stars=None) -> dict:
    """The ``params`` of a progress record: the reference's five, and the output settings that change the frame files only
    where they are not the defaults -- a record written before those settings existed still matches a default run.  A
    resume whose params differ from the record's starts over."""
    params = {"n_frames": n_frames, "fov": fov, "orbit": orbit, "disk_rotation_speed": disk_rotation_speed,
              "orbit_degrees": orbit_degrees}
    if video_codec == "mjpeg":
        params.update(video_codec=video_codec, video_quality=video_quality)
    if bit_depth != 8:
        params.update(bit_depth=bit_depth)
    if dither != "none":
        params.update(dither=dither)
    if shutter > 0:
        params.update(shutter=shutter, shutter_samples=shutter_samples)
    if grade is not None:
        params.update(tonemap=grade["tonemap"], exposure=grade["exposure"], white=grade["white"], transfer=grade["transfer"])
    if ray_map:
        params.update(ray_map=True)
    if orbit_map:
        params.update(orbit_map=True)
    if shutter_map:
        params.update(shutter_map=True)
    if spin_map:
        params.update(spin_map=True)
    if spin_shutter_map:
        params.update(spin_shutter_map=True)
    if spin_map_supersample > 1:
        params.update(spin_map_supersample=spin_map_supersample)
    if map_supersample > 1:
        params.update(map_supersample=map_supersample)
    if video_hdr is not None:
        params.update(video_hdr=video_hdr, hdr_white=hdr_white, hdr_exposure=hdr_exposure)
    if observer is not None:
        params.update(observer=observer)
    if stars is not None:
        params.update(stars=dict(stars))
    if projection is not None:
        params.update(projection=projection)
    if light_delay is not None:
        params.update(light_delay=light_delay)
    if polarization is not None:
        params.update(polarization={"field": list(polarization["field"]), "fraction": polarization["fraction"], "cell": polarization["cell"]})
    if kerr_view is not None:
        params.update(kerr_view={k: (list(v) if isinstance(v, tuple) else v) for k, v in kerr_view.items()})
    if kerr_stars is not None:
        params.update(kerr_stars=dict(kerr_stars))
    return params


def _drop_stream(stream, encoder, err) -> None:
    """The yuv420p stream is an extra: when its consumer dies (an ffmpeg without libx264 exits at once and every later
    write fails with EPIPE) the stream is closed, the encoder reaped, and the render goes on with the PNG frames, from
    which assemble_video builds the MP4 at the end as the reference does (render.py:4497-4503).  Returns None."""
    print(f"Warning: video stream failed ({err}); continuing with the PNG frames")
    try:
        stream.close()
    except Exception:
        pass
    if encoder is not None:
        try:
            encoder.stdin.close()
        except Exception:
            pass
        try:
            encoder.kill()
        except Exception:
            pass
        try:
            encoder.wait(timeout=10)
        except Exception:
            pass
    return None


def render_video(renderer: HipRenderer, width: int, height: int, n_frames: int, fps: int, output_path: str,
                 fov: float, static_cam_pos: List[float], orbit: bool = False, resume: bool = False,
                 disk_rotation_speed: float = 0.1, orbit_degrees: float = 360.0, rank: int = 0, world: int = 1,
                 assemble: bool = True, png_level: int = DEVICE, sink_slots: int = 0, sink_workers: int = 0,
                 video_stream: str = "auto", stats: Optional[dict] = None, supersample: Optional[int] = None,
                 supersample_threshold: Optional[float] = None, video_codec: str = "auto", video_quality: int = 90,
                 bit_depth: int = 8, dither: str = "none", shutter: float = 0.0, shutter_samples: int = 8,
                 grade: Optional[dict] = None, ray_map: bool = False, orbit_map: bool = False, shutter_map: bool = False,
                 map_supersample: int = 1, video_hdr: Optional[str] = None, hdr_white: float = 203.0, hdr_exposure: float = 0.0,
                 observer: Optional[str] = None, observer_velocity=None, observer_sky: bool = True,
                 infall_to: Optional[float] = None, stars: Optional[dict] = None, projection: Optional[str] = None, projection_fov=None,
                 light_delay=None, polarization: Optional[dict] = None, stokes_path: Optional[str] = None, spin_map: bool = False,
                 kerr_polarization: Optional[dict] = None, kerr_view: Optional[dict] = None, spin_map_supersample: int = 1,
                 spin_shutter_map: bool = False, kerr_stars: Optional[dict] = None, kerr_anti_alias: Optional[float] = None, kerr_disk_model: str = "texture",
                 kerr_line: Optional[dict] = None,
                 **_deprecated_kwargs) -> None:
    """N frames -> PNGs (+ MP4) (render.py:4356-4511).  Frame f is rendered by rank f % world.

    What does not combine is refused with ValueError, naming the combination, before any device work: every feature below refuses
    the rows of its entry in rules.FEATURES, in the order of the calls at the top of this function.

    ``video_stream``: the reference assembles the MP4 by reading every PNG back (render.py:4497-4503).  Here a
    single-rank, non-resumed session can also hand the frames straight to the encoder as a yuv420p YUV4MPEG2
    stream converted on the device (output.Y4MStream): "auto" pipes it into ``ffmpeg -f yuv4mpegpipe`` when an
    ffmpeg binary is on PATH (MP4 written while the frames render; otherwise PNGs + assemble_video as before),
    "y4m" writes ``<output stem>.y4m`` beside the output, "off" never streams.  PNG frames and progress.json are
    written in every mode (resume format of the reference).

    ``png_level``: output.DEVICE (default) filters and Huffman-codes every frame on the GPU (csrc/png_device.hip; the
    sink's threads only fetch and write the finished files); 0..9 selects the host encoder at that zlib level
    (smaller files, ~50 ms of a host core per fhd frame at level 1).

    ``supersample``: k x k rays per pixel for the frames of the video (None: as the renderer is set);
    ``supersample_threshold``: with it, adaptive (only the pixels whose k = 1 neighbours differ by more than it).

    ``video_codec``: "auto" is everything above.  "mjpeg" makes the video without any external encoder: every frame is
    coded as baseline JPEG of ``video_quality`` (1..100) on the device (csrc/jpeg_device.hip), the frame files are
    ``frame_%04d.jpg`` in the same frames directory, and assemble_video muxes them into the MP4 as Motion-JPEG.  No PNG
    is written, the yuv420p stream and the search for ffmpeg / pyav are skipped, resume looks for the .jpg files, and the
    progress record's params carry the codec and the quality (a resume across codecs or qualities starts over).  In this
    mode the renderer's outputs selection is restored on return ("auto" leaves it at "u8", as it always has).

    ``bit_depth=16``: the frame files are 16-bit PNGs (bhr_sink_create_png16; on the device up to its width limit, else on the
    host); the yuv420p stream stays 8-bit (``video_hdr`` is the 10-bit stream), and the PNG-in-MP4 fallback muxes the files as it muxes any PNG.  ``dither="blue"``:
    every 8-bit consumer of the loop -- PNG or JPEG frames, the yuv420p stream -- gets the blue-noise dithered rows
    (HipRenderer.set_dither; the renderer's mode is restored on return).  The progress record carries the two only when
    they are not the defaults, as it does the codec: a resume with other values starts over.

    ``shutter`` (0..1, the share of the frame time the shutter is open) above 0: motion blur.  Frame f is the mean of
    ``shutter_samples`` (1..64) marches (HipRenderer.render_shutter_async) at the fractional frame numbers u_j of
    shutter_times(f, shutter, shutter_samples): sample j is marched from orbit_position(static_cam_pos, u_j, ...) (the static
    position without ``orbit``) with the disk rolled by t_offset = (u_j - f) * disk_rotation_speed, the Keplerian roll of the
    texture within the exposure.  The texture itself is the frame's, composed once at t = f * dt: the populations and the
    noise are NOT sampled within the exposure.  With ``shutter == 0`` the loop calls render_async exactly as it always has,
    whatever ``shutter_samples`` is; the progress record carries the two values only when ``shutter > 0``, and a resume with
    other values starts over.

    ``grade``: None (the frames are as the renderer is set), or a dict of HipRenderer.set_grade's arguments (tonemap, exposure,
    white, transfer): every consumer of the loop -- PNG (8 and 16 bit) or JPEG frames, the dither, the yuv420p stream -- gets the
    graded frame; the renderer's own grade is restored on return.  The progress record carries the four values only when a
    grade is given, and a resume with other values starts over.  The frames keep no HDR plane.

    ``ray_map=True`` (a camera that stands still): the view is marched ONCE, before the loop (HipRenderer.build_ray_map), and
    every frame is shaded from that map under the frame's texture (render_from_ray_map_async) instead of being marched again.
    The frames are the STRICT arithmetic's whatever the renderer's ``math``: byte for byte those of a math="strict" run
    without the flag.  The progress record carries ``ray_map`` when it is set, and a resume with the other setting starts over.

    ``orbit_map=True`` (with ``orbit``, a disk that is not tilted): ONE ray map serves the whole orbit.  The orbit turns the
    camera rigidly about z, which is a symmetry of the hole, the untilted disk and the escape sphere, so the rays of frame f are
    the rays of frame 0 turned by the orbit angle.  The map is built once for orbit_position(static_cam_pos, 0, ...) and frame f
    is shaded from it turned to orbit_position(static_cam_pos, f, ...) (render_from_ray_map_async(cam_pos=...)).  Frame 0 is
    byte for byte the math="strict" frame; a later frame is the strict march of the SYMMETRIC rays, not byte-identical to the
    marched frame of its view: as far from it as two strict marches of symmetric views are from each other (f32 rounding of
    the march, per-channel RMSE of a few 1e-5).  The progress record carries ``orbit_map`` when it is set, and a resume with the other setting starts over.

    ``spin_map=True`` (a renderer with a spin or the exact redshift): ONE Kerr ray map serves the whole video
    (HipRenderer.build_kerr_ray_map).  A camera that stands still: its view is marched once, before the loop, and every frame is
    shaded from the map (render_from_kerr_ray_map_async), bit for bit the marched frame.  With ``orbit``: the spin axis is z, so
    the orbit is an exact symmetry of everything a Kerr ray's path depends on; frame 0's view is marched once and every frame is
    shaded from the map turned to the frame's camera -- frame 0 is the marched frame, the others are as far from theirs as two
    Kerr marches of symmetric views are from each other.  The map is freed at the end.  The progress record carries ``spin_map``
    when it is set, and a resume with the other setting starts over.

    ``spin_map_supersample`` = k in {1, 2, 4, 8} (with ``spin_map=True``): the Kerr map's own factor
    (HipRenderer.build_kerr_ray_map(supersample=k)) -- k x k records per pixel, every frame from the map resolved with
    set_supersample's filter; with a camera that stands still the frames are byte for byte those of the marched video of a
    renderer with ``supersample=k``, and no march runs per frame.  ``supersample`` and ``map_supersample`` stay 1 with this map.
    The progress record carries ``spin_map_supersample`` when it is above 1,
    and a resume with another factor starts over.

    ``spin_shutter_map=True`` (a renderer with a spin or the exact redshift, ``shutter > 0``): motion blur from ONE Kerr ray map
    -- ``shutter_map`` for the spinning hole.  The map is built once (frame 0's view under ``orbit``, else ``static_cam_pos``; with
    ``spin_map_supersample`` = k its own factor) and every frame is render_shutter_from_kerr_ray_map_async of exactly the sample
    times, positions and t_offsets the ``shutter_map`` loop hands render_shutter_from_ray_map_async; no sample is marched.
    The progress record carries
    ``spin_shutter_map`` when it is set, and a resume with the other setting starts over.

    ``shutter_map=True`` (with ``shutter > 0``): motion blur from ONE ray map.  What differs between the samples of an exposure
    -- the disk's roll, and under ``orbit`` the camera's turn about z -- is what a map leaves free, so no sample is marched: the
    map is built once (for orbit_position(static_cam_pos, 0, ...) under ``orbit``, else for ``static_cam_pos``) and every frame is
    render_shutter_from_ray_map_async of exactly the sample times, positions and t_offsets the marched shutter loop hands
    render_shutter_async.  The bg and disk layers are the STRICT arithmetic's whatever the renderer's ``math``, the post-pass is
    the renderer's own (exact f32 under math="strict", split f16 under fast / hybrid).  With a camera that stands still and
    math="strict" the frames are byte for byte those of the shutter video without the flag; under ``orbit`` they are the means
    of orbit-map frames (see above).  The progress record carries ``shutter_map`` when it is set, and a resume with the other setting starts over.

    ``map_supersample`` = k in {1, 2, 4, 8}: the factor of the one map the three modes above build
    (HipRenderer.build_ray_map(supersample=k)) -- k x k records per pixel, every frame from the map resolved with
    set_supersample's filter; ``supersample`` itself stays 1 with a map.  The progress record carries
    ``map_supersample`` when it is above 1, and a resume with another factor starts over.

    ``video_hdr`` = "pq" or "hlg": the loop's stream is the HDR one (output.Y4MStream(hdr=...); include/bhr_output.h states the
    formulas): 10-bit BT.2020 frames under that transfer, made on the device from every frame's unclipped scene-linear plane --
    ``hdr_exposure`` stops applied, and under PQ scene value 1.0 shown at ``hdr_white`` nits -- while the frame files stay what
    they would be without it: the SDR frames and the HDR stream come out of one render of each frame, whatever produces it
    (marched, shutter, ray_map, orbit_map, shutter_map).  The renderer's grade is the caller's with keep_hdr, and without a
    caller's grade {clip, 0 stops, linear, keep_hdr}, which gives the ungraded frame bit for bit; it is restored on return.
    ``video_stream="auto"`` with an ``ffmpeg`` on PATH pipes the stream into hdr_ffmpeg_args(video_hdr, output_path) (libx265);
    without one, or with "y4m", the stream is ``<output stem>.y4m`` and the MP4 is assembled from the SDR frames as before.
    After the loop ``<output stem>.hdr10.json`` (hdr_sidecar) records the stream's colour description, its MaxCLL and MaxFALL
    -- known only then -- and its frame count.  Refused with ValueError, before any device work: several ranks, a resume that
    finds completed frames (a stream cannot be resumed), ``video_codec="mjpeg"``, ``video_stream="off"``, odd frame sizes.  The
    progress record carries ``video_hdr``, ``hdr_white`` and ``hdr_exposure`` only when ``video_hdr`` is set.

    ``observer`` ("static", "circular" or "infall": bhr_amd.observer.velocity) or ``observer_velocity`` (a fixed beta): the
    camera moves.  Every frame is render_async(..., observer=beta_f, observer_sky=...) with the named velocity evaluated at
    that frame's own camera position (bhr_amd.observer.frame_plan), so an ``orbit`` with "circular" is the view from the
    orbiting camera.  ``infall_to`` = R (with "infall", without ``orbit``) moves the camera radially from |static_cam_pos| to R
    along static_cam_pos, uniformly in the falling observer's proper time.  The progress
    record carries the observer's settings when one is given, and a resume with others starts over.

    ``projection`` ("equirect" or "fisheye") with ``projection_fov``: every frame is render_async(..., projection=...) -- the
    width x height frames through that camera instead of the pinhole, ``fov`` unused -- from the moving camera when an observer
    is given as well.  The progress record
    carries the projection when one is given, and a resume under another starts over.  A full-sphere equirect video muxed by
    this package (Motion-JPEG, PNG-in-MP4) carries the Spherical Video V1 box (assemble_video).

    ``light_delay`` (a scale in [0, 16]): every frame is render_async(..., light_delay=scale) with the frame's own camera
    position and t_offset, with and without ``orbit`` -- each disk crossing shaded at the time its light left the gas.
    The progress record carries the scale when one
    is given, and a resume under another starts over.

    ``polarization`` (dict(field=, fraction=, cell=); needs ``ray_map=True``): every frame from the map is followed by the Stokes
    pass (HipRenderer.set_polarization), and the frames' cell grids -- never the full planes -- are collected into ONE compressed
    .npz at ``stokes_path`` (default ``<output stem>.stokes.npz``) with ``cells`` of shape (n_frames, gh, gw, 3).  Refused with
    a resume that finds frames already rendered (their grids are gone).  The renderer's polarisation is switched off on return.  The progress record names the polarisation
    only when it is set.

    ``kerr_view`` (check_kerr_view's dict; the renderer has a spin or the exact redshift set): every frame is
    render_async(..., kerr_observer=beta_f, kerr_projection=...) -- the Kerr march through the Kerr camera, with the named velocity
    evaluated at that frame's own camera position (bhr_amd.observer.kerr_frame_plan), so an ``orbit`` with "circular" is the
    fly-around on the equatorial geodesic.  The progress record carries the camera when one is given, and a resume under another starts over.

    ``kerr_anti_alias`` (the LOD strength; the renderer has a spin or the exact redshift set): the Kerr march's anti-aliasing
    (HipRenderer.set_kerr_anti_alias) is switched on for the video's marched frames, still or orbiting, and stays set on return.  A
    renderer that has it on already counts as asked: either way the Kerr ray map's features, the Kerr camera and several ranks are
    refused (rules.FEATURES["kerr_anti_alias"]).  The renderer is asked last of all, behind every other refusal.
    ``kerr_disk_model``: "texture", or "v2" / "v2_volume" -- the Kerr march's Disk V2 source (HipRenderer.use_kerr_disk_v2 with the
    renderer's radii and default structure) for the video's marched frames, still or orbiting; it stays set on return.  What
    rules.FEATURES["kerr_disk_model"] refuses is refused ahead of everything else.

    ``kerr_line`` (needs ``spin_map=True`` and no ``orbit``): render_image's dict -- a dynamic spectrum.  Every frame's line pass fills a
    device row of its own (HipRenderer.kerr_line_reserve(n_frames)); the rows are read once at the end and the .npz holds ``flux`` and
    ``counts`` of shape (n_frames, n_bins).  One GPU, no resume; a redshift map is a still's."""
    # the facts of this call, built once: what the call says, and what the renderer is set to -- which is read when the first rule asks
    # for it and not before (without a feature that needs them the renderer is not asked anything, as ever)
    moving = observer is not None or observer_velocity is not None or infall_to is not None
    f = facts = rules.Facts(dict(
        video=True, orbit=orbit, shutter=shutter, world=world, ray_map=ray_map, orbit_map=orbit_map, shutter_map=shutter_map, spin_map=spin_map,
        spin_shutter_map=spin_shutter_map, map_supersample=map_supersample, spin_map_supersample=spin_map_supersample, supersample_said=supersample,
        observer=moving, projection=projection is not None or projection_fov is not None, projection_fov=projection_fov, light_delay=light_delay is not None,
        stars=stars is not None, kerr_polarization=kerr_polarization is not None, kerr_stars=kerr_stars is not None, stokes_path=stokes_path,
        # (stokes_path alone counts as polarization's unless kerr_polarization, which it serves too, is there)
        polarization=polarization is not None or (stokes_path is not None and kerr_polarization is None), **_kerr_view_facts(kerr_view),
        kerr_disk_model=kerr_disk_model, kerr_anti_alias=lambda f: kerr_anti_alias is not None or getattr(renderer, "_kerr_anti_alias", None) is not None,
        **_kerr_line_facts(kerr_line), spin=lambda f: renderer.spin, redshift=lambda f: renderer.redshift, disk_tilt=lambda f: renderer.disk_tilt, anti_alias=lambda f: renderer.anti_alias,
        disk_model=lambda f: "texture" if getattr(renderer, "_dv2", None) is None else "v2",
        supersample=lambda f: renderer.supersample if supersample is None else supersample,
        supersample_threshold=lambda f: supersample_threshold if supersample is not None or supersample_threshold is not None
        else getattr(renderer, "supersample_threshold", None)))
    # the features are refused in this order (rules.py has what each refuses); the Kerr map's own factor first, then motion blur from
    # the Kerr map, so that each refusal names it
    kerr_disk_model = _checked_kerr_disk_model(kerr_disk_model, f)      # ahead of the rest, so that each refusal names --spin_disk_model
    check_spin_map_supersample(spin_map_supersample, spin_map=spin_map, spin_polarization=f["kerr_polarization"], spin_shutter_map=spin_shutter_map)
    rules.refuse_on("spin_shutter_map", f, "video")
    kerr_view, kerr_plan = checked("kerr_view", kerr_view, f, "video"), None
    if kerr_view is not None and (kerr_view["observer"] is not None or kerr_view["velocity"] is not None):
        from . import observer as obs_mod
        kerr_plan = obs_mod.kerr_frame_plan(n_frames, static_cam_pos, renderer.spin, kerr_view["observer"], kerr_view["velocity"], orbit, orbit_degrees)
    rules.refuse_on("spin_map", f, "video")
    # ``kerr_polarization`` (needs ``spin_map=True`` and no ``orbit``): polarization's outputs for a spinning hole -- set ahead of
    # the map's build, which then keeps the photon momenta; every frame's cell grid is collected into the one .npz
    kerr_polarization = checked("kerr_polarization", kerr_polarization, f, "video")
    plan = None
    if moving:
        from . import observer as obs_mod
        if observer is not None and observer_velocity is not None:
            raise ValueError("observer names a velocity and observer_velocity gives one: take one of the two")
        if infall_to is not None and observer != "infall":
            raise ValueError("infall_to is the path of observer='infall'")
        rules.refuse("observer", f, "video")
        plan = obs_mod.frame_plan(n_frames, static_cam_pos, observer, observer_velocity, orbit, orbit_degrees, infall_to)
    proj = checked("projection", projection, f, "video")
    light_delay = checked("light_delay", light_delay, f, "video")
    check_map_supersample(map_supersample, ray_map=ray_map, orbit_map=orbit_map, shutter_map=shutter_map)
    check_shutter(shutter, shutter_samples=shutter_samples)
    if kerr_polarization is None:
        polarization = checked("polarization", polarization, f, "video")
    if video_stream not in ("auto", "y4m", "off"):
        raise ValueError(f"video_stream must be 'auto', 'y4m' or 'off', got {video_stream!r}")
    hdr = check_video_hdr(video_hdr, hdr_white=hdr_white, hdr_exposure=hdr_exposure, width=width, height=height, world=world,
                          video_codec=video_codec, video_stream=video_stream)
    grade = check_grade(grade)
    if grade is not None:
        grade["keep_hdr"] = False
    rules.refuse_on("shutter_map orbit_map ray_map", f, "video")
    # the checks have refused every combination of two: the video's one map, or none
    mode = next((m for m in ("ray_map", "orbit_map", "shutter_map", "spin_map", "spin_shutter_map") if f[m]), None)
    # point stars: the renderer carries the catalogue (make_renderer(stars=)); the frames that show it are the map's
    stars = checked("stars", stars, f, "video")
    if stars is not None and renderer.stars_info()["n"] == 0:
        raise ValueError("point stars: the renderer has no star catalogue (make_renderer(stars=...) sets it)")
    # ``kerr_stars`` (needs ``spin_map=True``): point stars around a spinning hole, behind every refusal above -- the renderer
    # carries the Kerr catalogue (make_renderer(kerr_stars=)) and every frame from the Kerr map shows it; under ``orbit`` each frame
    # gathers the star plane of its turned view.  The progress record names the stars only when there are any.
    kerr_stars = checked("kerr_stars", kerr_stars, f, "video")
    if kerr_stars is not None and renderer.kerr_stars_info()["n"] == 0:
        raise ValueError("--spin_stars: the renderer has no Kerr star catalogue (make_renderer(kerr_stars=...) sets it)")
    kerr_line = _checked_kerr_line(kerr_line, f)
    if kerr_line is not None and resume:
        raise ValueError("--spin_line does not combine with --resume: the spectra of the frames rendered earlier are not on disk")
    if video_codec not in VIDEO_CODECS:
        raise ValueError(f"video_codec must be one of {VIDEO_CODECS}, got {video_codec!r}")
    check_depth_and_dither(bit_depth, dither=dither, video_codec=video_codec)
    mjpeg = video_codec == "mjpeg"
    if mjpeg and not (isinstance(video_quality, int) and 1 <= video_quality <= 100):
        raise ValueError(f"video_quality must be an integer between 1 and 100, got {video_quality!r}")
    ext = ".jpg" if mjpeg else ".png"
    if kerr_anti_alias is not None:                      # its own value and what the call itself says, ahead of any device work
        kerr_anti_alias = _checked_kerr_anti_alias(kerr_anti_alias, f)
    if supersample is not None:
        renderer.set_supersample(supersample, supersample_threshold)
    elif supersample_threshold is not None:
        renderer.set_supersample(renderer.supersample, supersample_threshold)
    os.makedirs(os.path.dirname(output_path) or ".", exist_ok=True)
    temp_dir = _frames_dir(output_path)
    submitted: List[int] = []
    progress_file = os.path.join(temp_dir, f"progress.json" if world == 1 else f"progress.rank{rank}.json")
    params = progress_params(
        n_frames=n_frames, fov=fov, orbit=orbit, disk_rotation_speed=disk_rotation_speed, orbit_degrees=orbit_degrees, video_codec=video_codec,
        video_quality=video_quality, bit_depth=bit_depth, dither=dither, shutter=shutter, shutter_samples=shutter_samples, grade=grade, ray_map=ray_map,
        orbit_map=orbit_map, shutter_map=shutter_map, map_supersample=map_supersample, video_hdr=video_hdr, hdr_white=hdr_white, hdr_exposure=hdr_exposure,
        observer=None if plan is None else {"kind": observer, "velocity": None if observer_velocity is None else list(observer_velocity),
                                            "sky": bool(observer_sky), "infall_to": infall_to},
        stars=stars, projection=None if proj is None else {"kind": proj[0], "fov": [proj[1], proj[2]]}, light_delay=light_delay, polarization=polarization,
        spin_map=spin_map, kerr_view=kerr_view, spin_map_supersample=spin_map_supersample, spin_shutter_map=spin_shutter_map, kerr_stars=kerr_stars)

    # Resume (render.py:4380-4434).  With several ranks the decision to start over is taken ONCE: every rank looks
    # at the same merged record of all ranks' progress files, only frame files and progress files are removed (never
    # the directory another rank may be creating or writing into), and each rank removes only what belongs to it.
    completed = set()
    os.makedirs(temp_dir, exist_ok=True)
    if resume:
        records = []
        for name in sorted(os.listdir(temp_dir)):
            if name == "progress.json" or (name.startswith("progress.rank") and name.endswith(".json")):
                try:
                    with open(os.path.join(temp_dir, name)) as f:
                        records.append(json.load(f))
                except (OSError, ValueError):
                    pass
        if records and any(r.get("params", {}) != params for r in records):
            print("Warning: parameters changed, starting over")
            for fr in range(rank, n_frames, world):                  # this rank's own frames
                try:
                    os.remove(os.path.join(temp_dir, f"frame_{fr:04d}{ext}"))
                except OSError:
                    pass
            # every stale record goes -- also the ones a run with another world size left under the other naming
            # (progress.json <-> progress.rank<r>.json), or every later --resume would see the mismatch again and start
            # over for ever.  Rank 0 removes the files no rank of THIS run owns; each rank removes its own.
            mine = os.path.basename(progress_file)
            current = {"progress.json"} if world == 1 else {f"progress.rank{r}.json" for r in range(world)}
            for name in sorted(os.listdir(temp_dir)):
                is_record = name == "progress.json" or (name.startswith("progress.rank") and name.endswith(".json"))
                if is_record and (name == mine or (rank == 0 and name not in current)):
                    try:
                        os.remove(os.path.join(temp_dir, name))
                    except OSError:
                        pass
        elif records:
            done = set()
            for r in records:                                        # a different world size last time: still counted
                done |= set(r.get("completed", []))
            completed = {f for f in done if os.path.isfile(os.path.join(temp_dir, f"frame_{f:04d}{ext}"))}
            print(f"Resuming: {len(completed)}/{n_frames} frames already rendered")
    if hdr is not None and completed:
        raise ValueError(f"--video_hdr does not resume: {len(completed)} frames are already rendered and a stream cannot be taken "
                         "up in the middle; render without --resume")

    if (polarization is not None or kerr_polarization is not None) and completed:
        raise ValueError(f"polarization does not resume: {len(completed)} frames are already rendered and their cell grids are gone; "
                         "render without --resume")

    # the Kerr anti-aliasing, behind every refusal above: asked for by the call, or on in the renderer (which is asked here, with the
    # first device work, and not before)
    if kerr_anti_alias is not None:
        renderer.set_kerr_anti_alias(True, kerr_anti_alias)
    elif getattr(renderer, "_kerr_anti_alias", None) is not None:
        rules.refuse("kerr_anti_alias", facts)
    # the Kerr march's Disk V2 source (kerr_disk_model): set for the video's marched frames, still or orbiting, and stays set on return
    use_kerr_analytic_disk(renderer, kerr_disk_model)
    total_t0 = time.time()
    rendered = 0
    # the reference saves through a 2-thread PIL pool (render.py:4412-4413); here the frame is quantised
    # on the device, copied into a pinned ring and encoded by worker threads while the next frames render
    if mjpeg:
        png_level = DEVICE                               # the JPEG coder runs on the device only
    if png_level == DEVICE and not mjpeg and width > _lib_max_png_width(bit_depth):
        print(f"  frames wider than {_lib_max_png_width(bit_depth)} pixels are PNG-encoded on the host (zlib level {VIDEO_LEVEL})")
        png_level = VIDEO_LEVEL
    if png_level == DEVICE and sink_workers <= 0:
        sink_workers = 4                                 # copy + write only
    if mjpeg:
        outputs_before = renderer.outputs
        sink = FrameSink(renderer, slots=sink_slots, workers=sink_workers, codec="jpeg", quality=video_quality)
    else:
        sink = FrameSink(renderer, slots=sink_slots, workers=sink_workers, level=png_level, bit_depth=bit_depth)
    dither_before = renderer.dither
    if dither != dither_before:
        renderer.set_dither(dither)
    grade_before = renderer.grade
    if hdr is not None:
        # the HDR stream reads the frame's scene-linear plane: the caller's grade, or the one that is the ungraded frame, keeps it
        grade = dict(grade or check_grade(dict(tonemap="clip", exposure=0.0, transfer="linear")), keep_hdr=True)
    if grade is not None:
        renderer.set_grade(**grade)
    stream = encoder = None
    streamable = world == 1 and not completed and width % 2 == 0 and height % 2 == 0 and not mjpeg
    if streamable and video_stream == "auto" and assemble and shutil.which("ffmpeg"):
        import subprocess
        encoder = subprocess.Popen(hdr_ffmpeg_args(video_hdr, output_path) if hdr is not None else
                                   ["ffmpeg", "-y", "-loglevel", "error", "-f", "yuv4mpegpipe", "-i", "-", "-c:v", "libx264",
                                    "-pix_fmt", "yuv420p", output_path], stdin=subprocess.PIPE)
        stream = Y4MStream(renderer, f"/proc/self/fd/{encoder.stdin.fileno()}", fps, hdr=hdr)
    elif streamable and (video_stream == "y4m" or hdr is not None):
        stream = Y4MStream(renderer, os.path.splitext(output_path)[0] + ".y4m", fps, hdr=hdr)

    # the loop's consumers read the quantised rows (PNG sink) and, with a yuv420p stream, the f32 frame: the V pass of every
    # frame stores exactly those (12 bytes per pixel less to write without a stream, 24 with the blur layer nobody reads)
    # (16-bit frames and dithered rows are quantised from the f32 frame by kernels of their own: the frame keeps f32)
    # (the HDR stream reads the frame's HDR plane, which the grade stage stores: the frame's own stores are as without a stream)
    if bit_depth == 16:
        renderer.set_outputs("f32")
    else:
        renderer.set_outputs("u8" if stream is None or hdr is not None else "f32+u8")
    n_r, n_phi = renderer.dtex_h, renderer.dtex_w
    factories = init_lifecycle_system(renderer, n_r, n_phi, seed=42)
    dt = disk_rotation_speed
    print(f"  lifecycle system ready (n_r={n_r}, n_phi={n_phi}), rank {rank}/{world}")
    if kerr_polarization is not None:
        renderer.set_kerr_polarization(**kerr_polarization)     # ahead of the build: the map then keeps the photon momenta
    if kerr_line is not None:
        renderer.set_kerr_line(**kerr_line["settings"])
        renderer.kerr_line_reserve(n_frames)                    # a device row per frame, read once at the end
    if mode is not None:
        # the one march of the video.  A camera that stands still: its view; an orbit: frame 0's (the orbit's radius is |pov|, not
        # the pov's xy norm: not the pov itself), which every frame's camera is a turn of about z
        _MAP_MODES[mode]["build"](renderer, orbit_position(static_cam_pos, 0, n_frames, orbit_degrees) if orbit else static_cam_pos, fov,
                                  spin_map_supersample if mode in ("spin_map", "spin_shutter_map") else map_supersample)
    stokes_grids = {}
    if polarization is not None:
        renderer.set_polarization(**polarization)
    t_loop0 = time.time()                               # ``stats`` (bench.py): the one-off set-up apart from the frame loop

    # (the map, a polarisation set above and the renderer's outputs, dither and grade do not outlive a frame loop that raises)
    try:
        try:
            for frame in range(n_frames):
                t = frame * dt
                mine = frame % world == rank and frame not in completed
                # the factories advance on every frame index on every rank; statistics are a function of the
                # frame index (every 60th), texture composition only happens for frames rendered here
                advance_lifecycle_frame(renderer, factories, t, dt, recompute_stats=(frame % 60 == 0), compose=mine)
                if not mine:
                    continue
                cam_pos = orbit_position(static_cam_pos, frame, n_frames, orbit_degrees) if orbit else static_cam_pos
                if plan is not None:
                    cam_pos, beta = plan[frame]                    # the moving observer: the frame's position and its velocity there
                t0 = time.time()
                fr = dict(cam_pos=cam_pos, fov=fov, orbit=orbit)
                if shutter > 0:
                    times = shutter_times(frame, shutter, shutter_samples)
                    fr["positions"] = [orbit_position(static_cam_pos, u, n_frames, orbit_degrees) if orbit else static_cam_pos for u in times]
                    fr["t_offsets"] = [(u - frame) * disk_rotation_speed for u in times]
                if mode is not None:                               # from the video's map: shade, no march
                    if kerr_line is not None:
                        renderer.set_kerr_line_row(frame)
                    _MAP_MODES[mode]["frame"](renderer, fr)
                    if polarization is not None or kerr_polarization is not None:      # (ray_map, or spin_map under kerr_polarization)
                        stokes_grids[frame] = renderer.stokes_cells()      # the frame's cell grid (synchronises: a few kB per frame)
                elif shutter > 0:
                    renderer.render_shutter_async(fr["positions"], fov, fr["t_offsets"])
                elif kerr_view is not None:                        # marched by the Kerr camera's object, at the frame's own velocity
                    renderer.render_async(cam_pos, fov, frame=0, **_kerr_view_kw(kerr_view, None if kerr_plan is None else kerr_plan[frame][1]))
                else:                                              # marched: the frame of the moving camera, through the projection, with light delay
                    renderer.render_async(cam_pos, fov, frame=0, observer=None if plan is None else beta, observer_sky=observer_sky,
                                          projection=projection, projection_fov=projection_fov, light_delay=light_delay)   # (lens flare: on the device)
                sink.submit(os.path.join(temp_dir, f"frame_{frame:04d}{ext}"))
                if stream is not None:
                    try:
                        stream.submit()
                    except Exception as e:                      # the encoder went away (EPIPE): the PNG frames carry on
                        stream, encoder = _drop_stream(stream, encoder, e), None
                elapsed = time.time() - t0
                rendered += 1
                submitted.append(frame)
                if rendered % 50 == 0 or frame >= n_frames - world:
                    sink.drain()                                # progress.json only lists frames that are on disk
                    completed.update(submitted)
                    submitted.clear()
                    with open(progress_file, "w") as f:
                        json.dump({"params": params, "completed": sorted(completed)}, f)
                if rendered % 100 == 0 or frame == n_frames - 1:
                    print(f"  frame {frame}/{n_frames} {elapsed * 1e3:.1f} ms, done {len(completed)}")
        finally:
            if polarization is not None:
                renderer.set_polarization(None)
            if kerr_polarization is not None:
                renderer.set_kerr_polarization(None)
            if kerr_line is not None and rendered != n_frames:
                renderer.set_kerr_line(None)
        frames_written, bytes_written = sink.drain()
        sink.close()
        if kerr_line is not None:
            # one GPU and no resume (above): every frame was rendered here, so every row is filled
            _save_kerr_line(renderer, kerr_line, n_frames)
            renderer.set_kerr_line(None)
        hole = {} if kerr_polarization is None else {"hole": dict(spin=renderer.spin, redshift=renderer.redshift)}
        polarization = polarization if kerr_polarization is None else kerr_polarization
        if polarization is not None:
            from .polarization import write_stokes
            path = stokes_path if stokes_path is not None else os.path.splitext(output_path)[0] + ".stokes.npz"
            # one GPU and no resume (check_polarization, above): every frame was rendered here, so every grid is here
            if len(stokes_grids) != n_frames:
                raise RuntimeError(f"polarization: {len(stokes_grids)} cell grids for {n_frames} frames; {path} is not written")
            write_stokes(path, np.stack([stokes_grids[f] for f in range(n_frames)]), polarization["cell"], polarization["field"],
                         polarization["fraction"], camera=dict(cam_pos=list(static_cam_pos), fov=fov), **hole)
            print(f"Saved: {path} ({n_frames} cell grids of {polarization['cell']}-pixel cells)")
    finally:
        if mode is not None:
            getattr(renderer, _MAP_MODES[mode]["free"])()
        if mjpeg:
            renderer.set_outputs(outputs_before)
        if dither != dither_before:
            renderer.set_dither(dither_before)
        if grade is not None:
            renderer.set_grade(**(grade_before or {}))
    if stats is not None:
        stats.update(setup_s=t_loop0 - total_t0, loop_s=time.time() - t_loop0, frames=rendered)
    streamed = False
    if stream is not None:
        try:
            n_streamed, _ = stream.drain()
        except Exception as e:
            stream, encoder = _drop_stream(stream, encoder, e), None
    if stream is not None and hdr is not None:
        max_cll, max_fall = stream.light_levels()
        sidecar = os.path.splitext(output_path)[0] + ".hdr10.json"
        with open(sidecar, "w") as f:
            json.dump(hdr_sidecar(hdr, max_cll, max_fall, n_streamed), f)
        print(f"HDR stream: {video_hdr}, MaxCLL {max_cll:.1f} nits, MaxFALL {max_fall:.1f} nits ({sidecar})")
    if stream is not None:
        stream.close()
        if encoder is not None:
            encoder.stdin.close()
            streamed = encoder.wait() == 0 and n_streamed == n_frames
            print(f"Video saved: {output_path} (yuv420p stream, {n_streamed} frames)" if streamed
                  else "ffmpeg failed on the stream; falling back to the PNG frames")
        else:
            print(f"YUV4MPEG2 stream: {os.path.splitext(output_path)[0]}.y4m ({n_streamed} frames)")
    completed.update(submitted)
    with open(progress_file, "w") as f:
        json.dump({"params": params, "completed": sorted(completed)}, f)
    if rendered:
        print(f"Session rendered {rendered} frames in {time.time() - total_t0:.1f} s "
              f"({rendered / (time.time() - total_t0):.1f} fps incl. {'JPEG' if mjpeg else 'PNG'} encode "
              f"{'on the device' if png_level == DEVICE else f'(zlib level {png_level})'}, "
              f"{bytes_written / max(frames_written, 1) / 1e6:.2f} MB/frame, {sink.workers} encoder threads)")
    if world > 1 or not assemble:
        return       # rank 0 assembles after a barrier (cli.py)
    if len(completed) < n_frames:
        print(f"Warning: only {len(completed)}/{n_frames} frames completed. Run again to resume.")
        return
    if not streamed:
        from .projection import full_sphere
        assemble_video(temp_dir, n_frames, fps, output_path, codec=video_codec,
                       **({"spherical": True} if proj is not None and full_sphere(projection, projection_fov) else {}))
