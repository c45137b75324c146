"""Command line of the reference (render.py:4518-4694), same flags and defaults, on the HIP backend.

Additions: ``--device hip`` (the default and only backend; ``gpu`` is accepted as an alias, ``cpu`` is
refused -- this build has no CPU path), ``-r 8k``, ``--gpus N`` (row-block tiling of a still image
inside one process; for ``--video`` launch one process per GPU with torchrun and frames are sharded
round-robin by RANK / WORLD_SIZE), ``--disk_model`` (the analytic Disk V2 sources of the march kernel), ``--observer`` /
``--observer_velocity`` (a camera that moves: aberration and Doppler shift), ``--stars point`` (the procedural sky's stars as a
catalogue of lensed points rendered through a ray map), ``--light_delay`` (every disk crossing shaded at the
time its light left the gas), ``--projection`` / ``--projection_fov`` (equirectangular 360-degree
frames and fisheye dome masters instead of the pinhole camera), ``--polarization`` (Stokes Q / U maps of the disk through a ray map),
``--spin_observer`` / ``--spin_projection`` and their companions (the moving and the panoramic camera of a spinning hole),
``--spin_stars point`` (the catalogue of lensed points through a Kerr ray map), ``--spin_passes`` (a Kerr ray map's passes of a still)
``--spin_anti_alias lod_radius`` / ``--spin_aa_strength`` (ray differentials and mip LOD for the spinning hole's disk) and
``--spin_disk_model v2 | v2_volume`` (the analytic Disk V2 sources under a spin).
"""
from __future__ import annotations

import argparse
import math
import os
from typing import Optional

from .renderer import R_DISK_INNER_DEFAULT, R_DISK_OUTER_DEFAULT

DISK_GENERATION_SCALE_CHOICES = (1, 2, 4)
RESOLUTIONS = {"8k": (7680, 4320), "4k": (3840, 2160), "fhd": (1920, 1080), "hd": (1280, 720), "sd": (640, 360)}


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Schwarzschild black-hole ray tracer (MI355X / HIP)")
    p.add_argument("--pov", type=float, nargs=3, default=[6, 0, 0.5], metavar=("X", "Y", "Z"),
                   help="camera position (default: 6 0 0.5)")
    p.add_argument("--fov", type=float, default=None, help="field of view 0-180 deg (default: 90)")
    p.add_argument("--resolution", "-r", type=str, default="fhd", choices=list(RESOLUTIONS),
                   help="8k/4k/fhd/hd/sd (default: fhd)")
    p.add_argument("--texture", "-t", type=str, default=None, help="skybox texture path")
    p.add_argument("--output", "-o", type=str, default="output/blackhole.png",
                   help="output path (default: output/blackhole.png)")
    p.add_argument("--step_size", "-s", type=float, default=0.1, help="integration step (default: 0.1)")
    p.add_argument("--r_max", type=float, default=10, help="escape radius (default: 10)")
    p.add_argument("--n_stars", type=int, default=6000, help="stars of the procedural skybox (default: 6000)")
    p.add_argument("--disk_texture", type=str, default=None,
                   help="disk texture path (default: procedural; still images only)")
    p.add_argument("--disk_generation_scale", type=int, default=2, choices=DISK_GENERATION_SCALE_CHOICES,
                   help="[deprecated] ignored by the lifecycle system (default: 2)")
    p.add_argument("--force_regenerate_disk_texture", action="store_true",
                   help="[deprecated] the lifecycle system always regenerates")
    p.add_argument("--disk_inner_radius", "--ar1", dest="disk_inner_radius", type=float,
                   default=R_DISK_INNER_DEFAULT, help=f"disk inner radius (default: {R_DISK_INNER_DEFAULT})")
    p.add_argument("--disk_outer_radius", "--ar2", dest="disk_outer_radius", type=float,
                   default=R_DISK_OUTER_DEFAULT, help=f"disk outer radius (default: {R_DISK_OUTER_DEFAULT})")
    p.add_argument("--disk_tilt", type=float, default=0.0, help="disk tilt in degrees (default: 0)")
    p.add_argument("--lens_flare", action="store_true", help="enable the lens flare")
    p.add_argument("--anti_alias", type=str, default="disabled", choices=["disabled", "lod_radius"],
                   help="disabled | lod_radius (ray-differential mip LOD) (default: disabled)")
    p.add_argument("--aa_strength", type=float, default=1.0, help="LOD multiplier 0.5-2.0 (default: 1.0)")
    p.add_argument("--device", "-d", type=str, default="hip", choices=["hip", "gpu", "cpu"],
                   help="hip (MI355X). 'gpu' is an alias; 'cpu' is refused: there is no CPU path")
    p.add_argument("--disk_model", type=str, default="texture", choices=["texture", "v2", "v2_volume"],
                   help="disk source of still images: the lifecycle texture (default), the analytic Disk V2 model at "
                        "each plane crossing, or its finite-thickness emission-absorption integral")
    p.add_argument("--gpus", type=int, default=1, help="row-block tile a still image over N GPUs of this node")
    p.add_argument("--math", type=str, default="hybrid", choices=["hybrid", "strict", "fast"],
                   help="march arithmetic.  strict: the reference's operations one by one with exactly rounded sqrt / divide "
                        "(ray paths bit-identical to an IEEE f32 evaluation of the reference).  hybrid (default): strict on the "
                        "8x8 tiles whose rays pass near the photon sphere, the fast arithmetic elsewhere -- within 3e-5 RMSE of "
                        "strict, 1.7x faster; anti-aliased (--anti_alias lod_radius) and tilted views add guards to the fast tiles and "
                        "march the pixels they flag again with the strict arithmetic.  fast: v_rsq / v_rcp + fast-math "
                        "everywhere (the analogue of Taichi's fast_math=True)")
    p.add_argument("--supersample", type=int, default=1, choices=[1, 2, 4, 8],
                   help="k x k rays per pixel, box-filtered inside the march (default: 1; one GPU)")
    p.add_argument("--supersample_threshold", type=float, default=None,
                   help="adaptive supersampling: the k x k rays of --supersample only for the pixels whose largest difference to an "
                        "edge neighbour in the one-ray frame exceeds this value (omitted: every pixel)")
    p.add_argument("--spin", type=float, default=0.0, metavar="A",
                   help="spin of the hole, the dimensionless a/M with |A| <= 0.998 (default: 0, a Schwarzschild hole).  Positive: the "
                        "hole turns with the disk's orbital motion; negative: a retrograde disk.  The spin axis is the disk normal.  "
                        "Marched in Kerr-Schild form by a kernel of its own, whatever --math says.  Not with --disk_tilt, "
                        "--anti_alias lod_radius, --disk_model v2 / v2_volume, --supersample_threshold, --shutter (unless --spin_shutter_map), the "
                        "ray-map flags, --passes or --gpus > 1; plain --supersample works")
    p.add_argument("--spin_anti_alias", type=str, default=argparse.SUPPRESS, choices=["lod_radius"],
                   help="--spin / --redshift exact: anti-aliasing of the spinning hole's disk.  lod_radius: every Kerr ray carries ray "
                        "differentials (the variational equations of the Kerr march, integrated beside the ray) and every disk crossing "
                        "samples the mip level of its footprint, as --anti_alias lod_radius does for the hole that does not spin.  "
                        "Still images and --video [--orbit]; combines with --supersample, --redshift exact, --lens_flare, the grade "
                        "and every sink.  Not without --spin / --redshift exact, with --spin_map, --spin_shutter_map, "
                        "--spin_polarization, --spin_stars, --spin_passes, --spin_observer / --spin_projection or --gpus > 1")
    p.add_argument("--spin_disk_model", type=str, default=argparse.SUPPRESS, choices=["v2", "v2_volume"],
                   help="with --spin or --redshift exact: the Kerr march shades the analytic Disk V2 model instead of the disk texture -- "
                        "v2: the thin disk's temperature law on the plane, inner edge at --disk_inner_radius; v2_volume: the "
                        "finite-thickness emission-absorption integral (the model redshift only).  Stills and --video [--orbit], "
                        "with --supersample, --lens_flare and a grade.  Not with --disk_model v2 / v2_volume, --spin_map, "
                        "--spin_shutter_map, --spin_polarization, --spin_stars, --spin_passes, --spin_observer, --spin_projection, "
                        "--spin_anti_alias or --gpus > 1")
    p.add_argument("--spin_line", type=str, default=argparse.SUPPRESS, metavar="PATH.npz",
                   help="--spin / --redshift exact: the disk's relativistically broadened emission line (the Fe K alpha profile) -- the flux "
                        "g^4 x emissivity x solid angle of every disk crossing, binned in g = E_obs / E_em, from a Kerr ray map of the view; "
                        "written as a .npz (edges, flux, counts, g_mean, g_red, g_blue, energy).  A still builds the map and renders the "
                        "frame from it; with --video --spin_map the file holds one spectrum per frame.  May stand beside "
                        "--spin_polarization, --spin_stars and --spin_passes.  Not with --orbit, --shutter, --supersample, "
                        "--spin_map_supersample, --spin_shutter_map, --spin_observer / --spin_projection, --spin_anti_alias, "
                        "--spin_disk_model or --gpus > 1")
    p.add_argument("--spin_line_bins", type=int, default=argparse.SUPPRESS, metavar="N", help="--spin_line: bins of the histogram, 1 .. 4096 (default: 256)")
    p.add_argument("--spin_line_range", type=float, nargs=2, default=argparse.SUPPRESS, metavar=("GMIN", "GMAX"),
                   help="--spin_line: the histogram's range [GMIN, GMAX) of g (default: 0 2); what falls outside is counted in under / over")
    p.add_argument("--spin_line_index", type=float, default=argparse.SUPPRESS, metavar="Q",
                   help="--spin_line: the emissivity's power law (r / r_inner)^-Q, 0 .. 16 (default: 3)")
    p.add_argument("--spin_line_emissivity", type=str, default=argparse.SUPPRESS, choices=["powerlaw", "texture"],
                   help="--spin_line: powerlaw (default) is the power law alone; texture multiplies it by the disk texture's opacity under the "
                        "frame's roll, which makes a video's spectrum move")
    p.add_argument("--spin_line_orders", type=str, default=argparse.SUPPRESS, choices=["first", "all"],
                   help="--spin_line: first (default) counts a pixel's first disk crossing, an opaque disk; all counts every crossing (under "
                        "texture weighted by the transmittance in front of it)")
    p.add_argument("--spin_line_energy", type=float, default=argparse.SUPPRESS, metavar="KEV",
                   help="--spin_line: the line's rest energy in keV (default: 6.4); it only labels energy = g x E0 in the file")
    p.add_argument("--spin_g_map", type=str, default=argparse.SUPPRESS, metavar="PATH.png",
                   help="--spin / --redshift exact, still images: the redshift map -- the g of each pixel's first disk crossing in false colour, "
                        "diverging about g = 1 (blue above, red below, black where no disk is hit); takes --spin_line's companions")
    p.add_argument("--spin_aa_strength", type=float, default=argparse.SUPPRESS, metavar="S",
                   help="--spin_anti_alias lod_radius: LOD multiplier, finite and not negative (default: 1.0)")
    p.add_argument("--redshift", type=str, default="model", choices=["model", "exact"],
                   help="redshift of the disk around the hole of --spin.  model (default): the reference's g-factor model with "
                        "Kerr's orbital frequency.  exact: the g-factor of the Kerr metric -- frame dragging, the Doppler term from "
                        "the photon's own angular momentum, and gas that plunges inside the ISCO with the ISCO orbit's energy and "
                        "angular momentum.  It is the Kerr kernel's: with --spin 0 the Schwarzschild hole is marched by it too, "
                        "and what --spin does not combine with, --redshift exact does not either")
    p.add_argument("--observer", type=str, default=None, choices=["static", "circular", "infall"],
                   help="a camera that moves: aberration squeezes the sky and the shadow towards the direction of motion, the "
                        "Doppler factor brightens and blue-shifts what lies ahead.  static: at rest (the default picture, marched by the "
                        "observer kernel); circular: on the circular geodesic through the camera position, in the disk's sense "
                        "(half the speed of light at r = 3; outside 1.5 r_s and off the z axis); infall: in radial free fall from "
                        "rest at infinity.  A still evaluates the velocity at --pov, --video at every frame's own camera position.  "
                        "Marched by a strict kernel of its own whatever --math says.  Not with --spin, --redshift exact, --anti_alias "
                        "lod_radius, --disk_model v2 / v2_volume, --supersample_threshold, --gpus > 1, --shutter, the ray-map flags or --passes")
    p.add_argument("--observer_velocity", type=float, nargs=3, default=None, metavar=("BX", "BY", "BZ"),
                   help="the moving camera's velocity given directly, in units of c as the static observer at the camera measures "
                        "it, |beta| <= 0.995; instead of --observer")
    p.add_argument("--observer_sky", type=str, default=None, choices=["shift", "plain"],
                   help="--observer / --observer_velocity: shift (default) = the sky takes the Doppler factor too (brightness and "
                        "colour, values above 1 go to the HDR plane); plain = the sky is aberrated only")
    p.add_argument("--infall_to", type=float, default=None, metavar="R",
                   help="--observer infall --video: the camera falls radially from |pov| to R >= 1.05 along --pov, the frames "
                        "uniform in its proper time; not with --orbit")
    p.add_argument("--projection", type=str, default="perspective", choices=["perspective", "equirect", "fisheye"],
                   help="the camera's projection.  perspective (default): the pinhole camera of --fov.  equirect: the equirectangular "
                        "panorama, 360 x 180 degrees by default -- the whole sky, the second image of what lies behind the camera "
                        "included; the frame is the resolution's width x width / 2 (fhd: 1920 x 960).  fisheye: the equidistant "
                        "fisheye, 180 degrees by default -- a dome master; the frame is height x height (fhd: 1080 x 1080), blank "
                        "outside the image circle.  Both look along the camera's forward axis (at the hole), are marched by a strict "
                        "kernel of their own whatever --math says, and work with --supersample, --disk_tilt, --lens_flare, the grade, "
                        "HDR, --video [--orbit] and --observer.  A full-sphere equirect --video that this program muxes itself "
                        "(--video_codec mjpeg, or PNG frames in MP4 where no H.264 encoder exists) carries the Spherical Video V1 "
                        "metadata that makes players open it as a 360-degree video; the ffmpeg and pyav routes write none.  The "
                        "bloom does not wrap at the +-180 degree seam.  Not with --fov, --spin, --redshift exact, --anti_alias "
                        "lod_radius, --disk_model v2 / v2_volume, --supersample_threshold, --gpus > 1, --shutter, the ray-map flags, "
                        "--passes or --stars point")
    p.add_argument("--projection_fov", type=float, nargs="+", default=None, metavar=("A", "B"),
                   help="--projection equirect: the horizontal and vertical span in degrees, A in (0, 360] and B in (0, 180] (default: "
                        "360 180); --projection fisheye: the full angle of the image circle, A in (0, 360] (default: 180)")
    p.add_argument("--spin_observer", type=str, default=argparse.SUPPRESS, choices=["static", "circular", "zamo", "infall"], metavar="{static,circular,zamo}",
                   help="--spin / --redshift exact: the camera of the spinning hole moves through --pov -- aberration, the Doppler "
                        "factor in the disk's g and on the sky, in front of the Kerr march.  static: it hovers (the Kerr frame, "
                        "marched by the Kerr camera's kernel); circular: on the equatorial circular geodesic in the disk's sense "
                        "(--pov in the plane z = 0); zamo: the frame-dragged, zero-angular-momentum observer (anywhere outside the "
                        "static limit).  In a --video the velocity is evaluated at every frame's own position, so --orbit with "
                        "circular is the fly-around.  infall is not offered under a spin.  Works with --supersample, --lens_flare, "
                        "the grade, --video [--orbit], --video_codec mjpeg and --video_hdr.  Not with --spin_map, "
                        "--spin_polarization, --observer, --projection, --light_delay, --shutter, --gpus > 1, --passes or --stars point")
    p.add_argument("--spin_observer_velocity", type=float, nargs=3, default=argparse.SUPPRESS, metavar=("BX", "BY", "BZ"),
                   help="the spinning hole's camera velocity given directly, in units of c as the static observer at the camera "
                        "measures it, |beta| <= 0.995; instead of --spin_observer")
    p.add_argument("--spin_observer_sky", type=str, default=argparse.SUPPRESS, choices=["shift", "plain"],
                   help="--spin_observer / --spin_observer_velocity: shift (default) = the sky takes the Doppler factor too; plain = "
                        "the sky is aberrated only")
    p.add_argument("--spin_projection", type=str, default=argparse.SUPPRESS, choices=["equirect", "fisheye"],
                   help="--spin / --redshift exact: --projection's equirectangular or fisheye camera in front of the Kerr march; "
                        "frame sizes follow --projection's rule; combines with --spin_observer")
    p.add_argument("--spin_projection_fov", type=float, nargs="+", default=argparse.SUPPRESS, metavar=("A", "B"),
                   help="--spin_projection: its field of view, as --projection_fov")
    p.add_argument("--light_delay", type=float, nargs="?", const=1.0, default=argparse.SUPPRESS, metavar="SCALE",
                   help="light delay: every disk crossing is shaded at the time its light left the gas, so the far side of the disk "
                        "and the secondary image show the gas earlier than the near side does (tens of r_s / c: radians of orbital "
                        "phase near the inner edge).  SCALE in [0, 16] multiplies the delay: 1 (the default when the flag is given "
                        "bare) is physical, larger values exaggerate it, 0 is the undelayed frame.  Marched by a strict kernel of "
                        "its own whatever --math says; works with --supersample, --disk_tilt, --lens_flare, the grade, HDR and "
                        "--video [--orbit].  Not with --anti_alias lod_radius, --disk_model v2 / v2_volume, "
                        "--supersample_threshold, --gpus > 1, --spin, --redshift exact, the observer flags, --projection, --passes, "
                        "--shutter, the ray-map flags or --stars point")
    p.add_argument("--polarization", type=str, nargs="+", default=argparse.SUPPRESS, metavar="FIELD",
                   help="polarisation: Stokes Q / U maps of the disk's synchrotron light, computed through a ray map of the view by a "
                        "pass behind the shade.  FIELD is the magnetic field in the gas frame: toroidal, radial, vertical, or three "
                        "numbers BR BPHI BZ.  A still image writes --stokes_output (planes, cell grid, field, fraction, convention, "
                        "camera) and --polarization_ticks (the frame with a tick per cell); --video --ray_map collects one cell grid "
                        "per frame into one .npz.  The angle is counted from image-right towards image-up.  Not with --spin, "
                        "--redshift exact, the observer flags, --projection, --light_delay, --orbit_map, --shutter_map, --shutter, "
                        "--map_supersample > 1, --supersample > 1, --disk_model v2 / v2_volume, --gpus > 1, or a video without --ray_map")
    p.add_argument("--spin_polarization", type=str, nargs="+", default=argparse.SUPPRESS, metavar="FIELD",
                   help="--polarization for a spinning hole: the Stokes Q / U maps carried along each Kerr ray by the Walker-Penrose "
                        "constant.  FIELD as for --polarization.  Needs --spin (or --redshift exact); a still image builds a Kerr ray "
                        "map of the view and renders the frame from it; --video needs --spin_map and no --orbit.  Works with both "
                        "--redshift modes, --lens_flare and the grade; --polarization_fraction, --polarization_cell, --stokes_output "
                        "and --polarization_ticks serve it as they serve --polarization (the .npz also holds spin and redshift).  Not "
                        "with --polarization, --supersample > 1 or anything --spin_map refuses")
    p.add_argument("--polarization_fraction", type=float, default=argparse.SUPPRESS, metavar="PI0",
                   help="--polarization: the degree of polarisation of light emitted across the field, in [0, 1] (default: 0.7)")
    p.add_argument("--polarization_cell", type=int, default=argparse.SUPPRESS, metavar="C",
                   help="--polarization: the side of a cell of the tick grid in pixels, 8, 16 or 32 (default: 16)")
    p.add_argument("--stokes_output", type=str, default=argparse.SUPPRESS, metavar="PATH.npz",
                   help="--polarization: where the Stokes .npz goes (a video's default: <output stem>.stokes.npz)")
    p.add_argument("--polarization_ticks", type=str, default=argparse.SUPPRESS, metavar="PATH.png",
                   help="--polarization, still images: the frame with the polarisation ticks drawn over it")
    p.add_argument("--video_stream", type=str, default="auto", choices=["auto", "y4m", "off"],
                   help="--video: also hand the frames to the encoder as a yuv420p stream converted on the device "
                        "(auto: pipe into ffmpeg when it is on PATH; y4m: write <output stem>.y4m; off: PNG frames only)")
    p.add_argument("--png_encoder", type=str, default="device", choices=["device", "host"],
                   help="--video: PNG frames are filtered and Huffman-coded on the GPU (device, default) or by zlib on "
                        "host threads (host: ~10 %% smaller files, ~50 ms of a core per fhd frame)")
    p.add_argument("--video_codec", type=str, default="auto", choices=["auto", "mjpeg"],
                   help="--video: auto = PNG frames, and H.264 where an encoder exists (default); mjpeg = every frame is "
                        "JPEG-coded on the GPU and the frames are muxed into the MP4 as Motion-JPEG (no external encoder needed)")
    p.add_argument("--video_quality", type=int, default=90, help="--video_codec mjpeg: JPEG quality 1..100 (default: 90)")
    p.add_argument("--bit_depth", type=int, default=8, choices=[8, 16],
                   help="bits per sample of the PNG output: 8 (default), or 16 -- (uint16)(clip(x, 0, 1) * 65535), still images and "
                        "--video frames alike (the yuv420p stream stays 8-bit; --video_hdr is the 10-bit stream); not with --dither blue or --video_codec mjpeg")
    p.add_argument("--dither", type=str, default="none", choices=["none", "blue"],
                   help="8-bit quantisation: none = truncation as the reference (default); blue = a 64x64 blue-noise threshold is "
                        "added before the floor, so that smooth dark gradients come out as fine noise instead of bands")
    p.add_argument("--shutter", type=float, default=0.0, metavar="S",
                   help="--video: motion blur -- the share of the frame time the shutter is open, 0..1 (default: 0, an "
                        "instantaneous exposure); every frame is the mean of --shutter_samples marches over the exposure")
    p.add_argument("--shutter_samples", type=int, default=8, metavar="N",
                   help="--shutter: marches per frame, 1..64 (default: 8)")
    p.add_argument("--tonemap", type=str, default=None, choices=["clip", "reinhard", "aces"],
                   help="grade the frame in place of the hard clip at 1 (default: off): clip = exposure and transfer only; "
                        "reinhard = extended Reinhard roll-off, --white maps to 1; aces = Narkowicz's ACES filmic fit")
    p.add_argument("--exposure", type=float, default=None, metavar="STOPS",
                   help="--tonemap: exposure in stops, -16..16, the frame is scaled by 2^STOPS ahead of the operator (default: 0)")
    p.add_argument("--white", type=float, default=None, metavar="W",
                   help="--tonemap reinhard: the scene value that maps to 1, in (0, 65504] (default: 2.5)")
    p.add_argument("--transfer", type=str, default=None, choices=["linear", "srgb"],
                   help="--tonemap: display transfer function: linear = the values as they are, as the reference writes them "
                        "(default); srgb = the sRGB encoding curve")
    p.add_argument("--hdr_output", type=str, default=None, metavar="PATH",
                   help="still images: also write the unclipped scene-linear frame, before exposure, as PATH (.pfm: exact f32; "
                        ".hdr: Radiance RGBE)")
    p.add_argument("--video_hdr", type=str, default=None, choices=["pq", "hlg"],
                   help="--video: the video stream is HDR -- 10-bit BT.2020 frames under the PQ (SMPTE ST 2084) or HLG (BT.2100) "
                        "transfer, made on the device from every frame's unclipped scene-linear plane and piped into ffmpeg "
                        "(libx265) when it is on PATH, else written as <output stem>.y4m; <output stem>.hdr10.json records the "
                        "colour description and the content light levels.  The frame files stay the SDR frames they would be "
                        "without it.  One rank; not with --resume on a run that has frames, --video_codec mjpeg or --video_stream off")
    p.add_argument("--hdr_white", type=float, default=None, metavar="NITS",
                   help="--video_hdr pq: the display level of scene value 1.0 in nits, in (0, 10000] (default: 203, the reference "
                        "white of BT.2408)")
    p.add_argument("--hdr_exposure", type=float, default=None, metavar="STOPS",
                   help="--video_hdr: exposure of the HDR stream in stops, -16..16 (default: 0); the SDR frames take --exposure")
    p.add_argument("--ray_map", action="store_true",
                   help="--video with a camera that stands still: march the view once, before the loop, and shade every frame "
                        "from that ray map under the frame's texture instead of marching it again.  The frames are the strict "
                        "arithmetic's whatever --math says.  Not with --orbit, --shutter, --supersample > 1 (a supersampled map takes "
                        "--map_supersample), --disk_model v2 / v2_volume or --gpus > 1")
    p.add_argument("--orbit_map", action="store_true",
                   help="--video --orbit with --disk_tilt 0: march frame 0's view once and shade every frame of the orbit from "
                        "that one ray map, turned about z to the frame's camera (the orbit is a symmetry of the hole, the untilted "
                        "disk and the escape sphere).  Frame 0 is the strict arithmetic's frame; a later frame is the strict march "
                        "of the symmetric rays, not byte-identical to the marched frame of that view: as far from it as two strict "
                        "marches of symmetric views are from each other.  Not with --ray_map, --shutter, --supersample > 1 (a supersampled "
                        "map takes --map_supersample), --disk_model v2 / v2_volume or --gpus > 1")
    p.add_argument("--shutter_map", action="store_true",
                   help="--video --shutter S: motion blur from ONE ray map.  The view is marched once (frame 0's under --orbit) and "
                        "every sample of every exposure is shaded from that map -- the disk's roll and, under --orbit, the camera's "
                        "turn about z are what a ray map leaves free -- and averaged on the device; no sample is marched.  The bg "
                        "and disk layers are the strict arithmetic's whatever --math says (the bloom follows --math): with a camera "
                        "that stands still and --math strict the frames are byte-identical to the marched --shutter frames, under "
                        "--orbit they are the means of --orbit_map frames.  Not with --ray_map, "
                        "--orbit_map, --orbit together with --disk_tilt, --supersample > 1 (a supersampled map takes --map_supersample), "
                        "--disk_model v2 / v2_volume or --gpus > 1")
    p.add_argument("--spin_map", action="store_true", default=argparse.SUPPRESS,
                   help="--video with --spin or --redshift exact: march the spinning hole's view once with the Kerr march and shade "
                        "every frame from that one Kerr ray map instead of marching it again.  A camera that stands still: the "
                        "frames are byte-identical to the marched ones.  With --orbit: frame 0's view is marched and every frame is "
                        "shaded from the map turned about z, the spin axis, to the frame's camera (an exact symmetry of a Kerr ray's "
                        "path); frame 0 is the marched frame, a later frame the Kerr march of the symmetric rays.  --lens_flare, the "
                        "grade, --video_codec mjpeg, --video_hdr, --bit_depth 16 and --dither work as ever.  Not with --shutter, "
                        "--supersample > 1, --map_supersample > 1, --gpus > 1, --ray_map, --orbit_map, --shutter_map, the observer "
                        "flags, --projection, --light_delay, --stars point or --polarization")
    p.add_argument("--spin_shutter_map", action="store_true", default=argparse.SUPPRESS,
                   help="--video --shutter S with --spin or --redshift exact: motion blur from ONE Kerr ray map.  The spinning hole's "
                        "view is marched once (frame 0's under --orbit) and every sample of every exposure is shaded from that map -- "
                        "the disk's roll and, under --orbit, the camera's turn about z, the spin axis, are what a Kerr ray map leaves "
                        "free -- and averaged on the device; no sample is marched.  --spin_map_supersample K works beside it.  Not "
                        "with --spin_map (the map of an instantaneous exposure), --ray_map, --orbit_map, --shutter_map, --supersample "
                        "> 1, --map_supersample > 1, --spin_polarization, --spin_observer, --spin_projection, the observer flags, "
                        "--projection, --light_delay, --stars point, --polarization or --gpus > 1")
    p.add_argument("--spin_map_supersample", type=int, default=argparse.SUPPRESS, choices=[1, 2, 4, 8], metavar="K",
                   help="--spin_map: the Kerr ray map's own supersampling factor, 1, 2, 4 or 8 (default 1) -- the only anti-aliasing a "
                        "spinning hole has.  The one march of the video marches K x K Kerr rays per pixel and keeps their records; "
                        "every frame shades all of them and resolves each pixel with --supersample's box filter, so with a camera "
                        "that stands still the frames are byte-identical to those of --spin A --supersample K without a march per "
                        "frame.  Needs --spin_map or --spin_shutter_map (whose samples are then resolved one by one, ahead of the mean) and "
                        "takes the map's restrictions (--supersample and --map_supersample stay 1); not with --spin_polarization")
    p.add_argument("--map_supersample", type=int, default=1, choices=[1, 2, 4, 8], metavar="K",
                   help="--ray_map, --orbit_map or --shutter_map: the map's own supersampling factor, 1, 2, 4 or 8 (default 1).  The "
                        "one march of the video marches K x K rays per pixel and keeps their records; every frame shades all of them "
                        "and resolves each pixel with --supersample's box filter, so the frames are those of --supersample K under "
                        "--math strict without a march per frame.  Needs one of the three map flags; --supersample itself stays 1")
    p.add_argument("--passes", type=str, default=None, metavar="PATH.npz",
                   help="still images: also write the view's geometry passes (per pixel: steps, ray fate, escape direction, disk "
                        "crossings and hit points, from a ray map of the view) and the frame's bg / disk / blur layers as a "
                        "compressed .npz; the image itself is unchanged.  One GPU, --supersample 1, --disk_model texture")
    p.add_argument("--stars", type=str, default="texture", choices=["texture", "point"],
                   help="how the procedural sky's stars are drawn.  texture (default): baked into the sky texture as Gaussian blobs, "
                        "as the reference does -- a texture lookup conserves surface brightness, so near the hole a star is smeared "
                        "into a dim arc.  point: a star catalogue rendered through a ray map of the view -- every image of a star "
                        "stays a point and its flux is multiplied by the lensing magnification (the Einstein-ring sparkle); the sky "
                        "texture keeps the nebula and the glow.  The frame is shaded from the map with the strict arithmetic, "
                        "whatever --math says.  --video needs --ray_map or --orbit_map beside it.  Not with --texture, --shutter_map, "
                        "--map_supersample > 1, --supersample > 1, --gpus > 1, --disk_model v2 / v2_volume, --spin, --redshift exact "
                        "or a moving observer")
    p.add_argument("--star_gain", type=float, default=2.0, metavar="G",
                   help="--stars point: an unlensed star of table brightness b deposits G b in total, whatever the resolution "
                        "(default: 2.0, an aesthetic choice)")
    p.add_argument("--star_max_magnification", type=float, default=32.0, metavar="M",
                   help="--stars point: cap of a star image's magnification on the critical curve, 1 .. 1e6 (default: 32)")
    p.add_argument("--spin_stars", type=str, default=argparse.SUPPRESS, choices=["point"],
                   help="--spin or --redshift exact: point -- the procedural sky's stars as a catalogue rendered through a Kerr ray map "
                        "of the view, --stars point for a spinning hole: every image of a star stays a point and its flux is "
                        "multiplied by the lensing magnification, the sparkle along the asymmetric critical curve; the sky texture "
                        "keeps the nebula and the glow.  Reads --star_gain and --star_max_magnification.  A still is shaded from "
                        "the view's Kerr ray map; --video needs --spin_map beside it, and with --orbit every frame gathers the star "
                        "images of its turned view.  Not with --texture, --stars point, --supersample > 1, --spin_map_supersample > "
                        "1, --spin_shutter_map, --shutter, --spin_observer, --spin_projection, --spin_polarization or --gpus > 1")
    p.add_argument("--spin_passes", type=str, default=argparse.SUPPRESS, metavar="PATH.npz",
                   help="still images with --spin or --redshift exact: --passes for a spinning hole -- also build the Kerr ray map of "
                        "the view and write its geometry passes, the frame's bg / disk / blur layers and the hole's spin and "
                        "redshift mode as a compressed .npz; the image itself is unchanged.  Not with --supersample > 1, "
                        "--spin_observer, --spin_projection, --gpus > 1 or --video")
    p.add_argument("--ignore_taichi_cache", action="store_true", help="accepted for compatibility; no effect")
    p.add_argument("--video", action="store_true", help="render frames and assemble a video")
    p.add_argument("--interactive", action="store_true", help="not available in this build (needs ti.GUI)")
    p.add_argument("--orbit", action="store_true", help="video: orbit the camera around the origin")
    p.add_argument("--orbit_degrees", type=float, default=360.0, help="total orbit angle (default: 360)")
    p.add_argument("--n_frames", type=int, default=3600, help="video frames (default: 3600)")
    p.add_argument("--fps", type=int, default=36, help="video frame rate (default: 36)")
    p.add_argument("--resume", action="store_true", help="video: resume from progress.json")
    p.add_argument("--disk_rotation_algorithm", type=str, default="baseline",
                   choices=["baseline", "parametric", "keyframes"], help="[deprecated] ignored")
    p.add_argument("--disk_rotation_speed", type=float, default=0.1, help="disk rotation speed (default: 0.1)")
    p.add_argument("--keyframes_count", type=int, default=10, help="[deprecated] ignored")
    args = p.parse_args(argv)
    fov_given = args.fov is not None                # --projection refuses an explicit --fov; the default is 90 as ever
    args.fov = 90 if args.fov is None else args.fov
    # What does not combine: the rows of rules.FEATURES, feature by feature in this order, so that a line refused without a flag is
    # refused with the same words with it; between them the checks of a flag's own value.  Every refusal is an argparse error.
    from . import drivers, rules
    from .camera import orbit_position
    f = facts_from_args(args, fov_given)

    def refuse(features, surface="cli"):
        try:
            rules.refuse_on(features, f, surface)
        except ValueError as e:
            p.error(str(e))
    # the Kerr anti-aliasing (the drivers' words), ahead of everything else, so that each refusal names --spin_anti_alias
    if hasattr(args, "spin_aa_strength") and not hasattr(args, "spin_anti_alias"):
        p.error("--spin_aa_strength needs --spin_anti_alias lod_radius: it is that anti-aliasing's LOD multiplier")
    try:
        drivers._checked_kerr_anti_alias(kerr_anti_alias_from_args(args).get("kerr_anti_alias"), f)
    except ValueError as e:
        p.error(str(e))
    refuse("kerr_disk_model", "api")              # (the drivers' words, likewise ahead of everything else: each names --spin_disk_model)
    refuse("shutter")
    refuse("spin_shutter_map", "api")             # (the drivers' words: ahead of every other check, so that each names --spin_shutter_map)
    refuse("spin_map_supersample spin_map")       # ahead of a spin's own, so that each names --spin_map
    view = kerr_view_from_args(args)
    if view:
        # the Kerr camera (the drivers' words): ahead of a spin's own refusals, so that each names it
        try:
            checked = drivers.checked("kerr_view", view["kerr_view"], f)
            if fov_given and checked["projection"] is not None:
                raise ValueError(f"--spin_projection {checked['projection']} does not combine with --fov: that is the pinhole camera's "
                                 "field of view (--spin_projection_fov is this one's)")
            # the named velocity where the camera will stand: --pov, or frame 0 of an orbit (which keeps r and the height)
            drivers.kerr_view_beta(checked, orbit_position(args.pov, 0, max(args.n_frames, 1), args.orbit_degrees)
                                   if args.video and args.orbit else args.pov, args.spin)
        except ValueError as e:
            p.error(str(e))
    if rules.FEATURES["spin"]["on"](f):             # the Kerr march: asked for by a spin, or by the exact redshift at spin 0
        from .kerr import SPIN_MAX, camera_f, camera_outside_static_limit
        if not abs(args.spin) <= SPIN_MAX:
            p.error(f"--spin is a/M with |a/M| <= {SPIN_MAX}, got {args.spin}")
        refuse("spin")
        if not camera_outside_static_limit(args.pov, args.spin):
            who = rules.FEATURES["spin"]["words"]["who"](f)
            p.error(f"{who} needs --pov outside the static limit of the hole: at {args.pov} f = r / S = {camera_f(args.pov, args.spin)[0]:.4g} "
                    f"(f < 1 is needed: r > 1 in the disk plane), no static observer and no photon along every pixel direction there")
    if f["observer"]:
        from . import observer as obs
        refuse("observer")
        try:
            if args.observer_velocity is not None:
                obs.check_beta(args.observer_velocity)
            if args.infall_to is not None:
                obs.check_infall_to(args.pov, args.infall_to)
            # the named velocity where the camera will stand: --pov, frame 0 of an orbit (which keeps r and the height), and
            # the end of a fall, where it is largest
            if args.observer is not None:
                obs.velocity(args.observer, orbit_position(args.pov, 0, max(args.n_frames, 1), args.orbit_degrees) if args.video and args.orbit else args.pov)
                if args.infall_to is not None:
                    obs.velocity(args.observer, obs.frame_plan(2, args.pov, "infall", infall_to=args.infall_to)[-1][0])
        except ValueError as e:
            p.error(f"{rules.observer_flag(f)}: {e}")
    args.observer_sky = "shift" if args.observer_sky is None else args.observer_sky
    refuse("map_supersample shutter_map orbit_map ray_map")
    refuse("no_video_hdr video_hdr")
    args.hdr_white = 203.0 if args.hdr_white is None else args.hdr_white
    args.hdr_exposure = 0.0 if args.hdr_exposure is None else args.hdr_exposure
    refuse("passes stars")
    if args.stars == "point":
        if not (args.star_gain > 0 and math.isfinite(args.star_gain)):
            p.error(f"--star_gain must be greater than 0, got {args.star_gain}")
        if not 1.0 <= args.star_max_magnification <= 1e6:
            p.error(f"--star_max_magnification must be between 1 and 1e6, got {args.star_max_magnification}")
    refuse("projection")
    if args.projection != "perspective":
        try:
            from .projection import check
            check(args.projection, args.projection_fov)
        except ValueError as e:
            p.error(f"--projection {args.projection} --projection_fov: {e}")
    # the options from here on have no default in the namespace: they are there only when the flag was given
    if hasattr(args, "light_delay"):
        if not 0.0 <= args.light_delay <= 16.0:               # a NaN fails the comparison too
            p.error(f"--light_delay is a scale in [0, 16], got {args.light_delay}")
        refuse("light_delay")
    pol = getattr(args, "polarization", None)
    spin_pol = getattr(args, "spin_polarization", None)
    for flag in ("polarization_fraction", "polarization_cell", "stokes_output", "polarization_ticks"):
        if pol is None and spin_pol is None and getattr(args, flag, None) is not None:
            p.error(f"--{flag} needs --polarization: it belongs to the Stokes maps")
    for who, field, feature in (("--polarization", pol, "polarization"), ("--spin_polarization", spin_pol, "kerr_polarization")):
        if field is not None:
            from .polarization import DEFAULT_CELL, DEFAULT_FRACTION, check, parse_field
            try:
                check(parse_field(field), getattr(args, "polarization_fraction", DEFAULT_FRACTION), getattr(args, "polarization_cell", DEFAULT_CELL))
            except ValueError as e:
                p.error(f"{who}: {e}")
            refuse(feature)
    # the Kerr point stars and the Kerr passes (the drivers' words), behind every refusal above
    try:
        drivers.checked("kerr_stars", kerr_stars_from_args(args), f, "cli")
    except ValueError as e:
        p.error(str(e))
    refuse("kerr_passes", "api")
    # the Kerr line profile and the redshift map (the drivers' words), likewise
    for flag in ("spin_line_bins", "spin_line_range", "spin_line_index", "spin_line_emissivity", "spin_line_orders", "spin_line_energy"):
        if hasattr(args, flag) and not f["kerr_line"]:
            p.error(f"--{flag} needs --spin_line or --spin_g_map: it belongs to the line profile")
    try:
        drivers._checked_kerr_line(kerr_line_from_args(args).get("kerr_line"), f)
    except ValueError as e:
        p.error(str(e))
    # --exposure, --white, --transfer and --hdr_output without --tonemap mean --tonemap clip
    if args.tonemap is None and any(v is not None for v in (args.exposure, args.white, args.transfer, args.hdr_output)):
        args.tonemap = "clip"
    if args.tonemap is not None:
        args.exposure = 0.0 if args.exposure is None else args.exposure
        args.white = 2.5 if args.white is None else args.white
        args.transfer = "linear" if args.transfer is None else args.transfer
    return args


def facts_from_args(args, fov_given: bool):
    """What the rules look at (rules.FACTS), from the namespace of a command line.  A flag whose companions alone are given counts as
    given, so that the refusal names the combination first: the observer's four, --projection_fov, the Kerr camera's five."""
    from . import rules
    view = kerr_view_from_args(args).get("kerr_view", {})
    spin_projection = view.get("projection") is not None or view.get("projection_fov") is not None
    spin_polarization = hasattr(args, "spin_polarization")
    return rules.Facts(dict(
        video=args.video, orbit=args.orbit, shutter=args.shutter, supersample=args.supersample, supersample_threshold=args.supersample_threshold,
        map_supersample=args.map_supersample, spin_map_supersample=getattr(args, "spin_map_supersample", 1),
        spin_map_supersample_given=hasattr(args, "spin_map_supersample"), gpus=args.gpus, disk_model=args.disk_model,
        disk_tilt=args.disk_tilt, anti_alias=args.anti_alias, spin=args.spin, redshift=args.redshift, skybox_path=args.texture, fov_given=fov_given,
        flag_observer=args.observer, flag_observer_velocity=args.observer_velocity, flag_observer_sky=args.observer_sky, flag_infall_to=args.infall_to,
        observer=any(v is not None for v in (args.observer, args.observer_velocity, args.observer_sky, args.infall_to)),
        projection=args.projection != "perspective" or args.projection_fov is not None, projection_name=args.projection,
        light_delay=hasattr(args, "light_delay"), stars=args.stars == "point", kerr_polarization=spin_polarization,
        # (its four companions count as --polarization's unless --spin_polarization, which they serve too, is there)
        polarization=hasattr(args, "polarization") or (not spin_polarization and any(
            hasattr(args, n) for n in ("polarization_fraction", "polarization_cell", "stokes_output", "polarization_ticks"))),
        stokes_path=getattr(args, "stokes_output", None), ticks_path=getattr(args, "polarization_ticks", None),
        spin_observer=bool(view) and not spin_projection, spin_projection=spin_projection, kerr_stars=hasattr(args, "spin_stars"),
        passes=args.passes is not None, passes_path=args.passes, kerr_passes_path=getattr(args, "spin_passes", None), ray_map=args.ray_map,
        orbit_map=args.orbit_map, shutter_map=args.shutter_map, spin_map=hasattr(args, "spin_map"), spin_shutter_map=hasattr(args, "spin_shutter_map"),
        video_hdr=args.video_hdr, hdr_white_given=args.hdr_white is not None, hdr_exposure_given=args.hdr_exposure is not None, video_codec=args.video_codec,
        video_stream=args.video_stream, kerr_anti_alias=hasattr(args, "spin_anti_alias"), kerr_disk_model=getattr(args, "spin_disk_model", "texture"),
        kerr_line=hasattr(args, "spin_line") or hasattr(args, "spin_g_map"), kerr_line_path=getattr(args, "spin_line", None),
        g_map_path=getattr(args, "spin_g_map", None)))


def kerr_line_from_args(args) -> dict:
    """The Kerr line profile of a command line as drivers.render_image / render_video take it: {} without --spin_line and --spin_g_map."""
    if not (hasattr(args, "spin_line") or hasattr(args, "spin_g_map")):
        return {}
    line = dict(path=getattr(args, "spin_line", None), g_map_path=getattr(args, "spin_g_map", None))
    for flag, key in (("spin_line_bins", "n_bins"), ("spin_line_range", "g_range"), ("spin_line_index", "index"), ("spin_line_emissivity", "emissivity"),
                      ("spin_line_orders", "orders"), ("spin_line_energy", "energy_kev")):
        if hasattr(args, flag):
            line[key] = tuple(getattr(args, flag)) if key == "g_range" else getattr(args, flag)
    return dict(kerr_line=line)


def kerr_anti_alias_from_args(args) -> dict:
    """The Kerr anti-aliasing of a command line as drivers.render_image / render_video take it: {} without --spin_anti_alias."""
    if not hasattr(args, "spin_anti_alias"):
        return {}
    return dict(kerr_anti_alias=float(getattr(args, "spin_aa_strength", 1.0)))


def grade_from_args(args):
    """The grade of a command line as drivers.render_image / render_video take it: None without --tonemap."""
    if getattr(args, "tonemap", None) is None:
        return None
    return dict(tonemap=args.tonemap, exposure=args.exposure, white=args.white, transfer=args.transfer)


def stars_from_args(args):
    """The point stars of a command line as drivers.render_image / render_video take them: None without --stars point."""
    if getattr(args, "stars", "texture") != "point":
        return None
    return dict(gain=args.star_gain, max_magnification=args.star_max_magnification)


def kerr_stars_from_args(args):
    """The Kerr point stars of a command line as drivers.render_image / render_video take them: None without --spin_stars."""
    if not hasattr(args, "spin_stars"):
        return None
    return dict(gain=args.star_gain, max_magnification=args.star_max_magnification)


def projection_from_args(args) -> dict:
    """The projection of a command line as drivers.render_image / render_video take it: {} with the pinhole camera."""
    if getattr(args, "projection", "perspective") == "perspective":
        return {}
    fov = getattr(args, "projection_fov", None)
    return dict(projection=args.projection, projection_fov=None if fov is None else tuple(fov))


def kerr_view_from_args(args) -> dict:
    """The Kerr camera of a command line as drivers.render_image / render_video take it: {} without --spin_observer,
    --spin_observer_velocity, --spin_observer_sky, --spin_projection or --spin_projection_fov."""
    keys = (("observer", "spin_observer"), ("velocity", "spin_observer_velocity"), ("sky", "spin_observer_sky"),
            ("projection", "spin_projection"), ("projection_fov", "spin_projection_fov"))
    if not any(hasattr(args, flag) for _, flag in keys):
        return {}
    view = {k: getattr(args, flag, None) for k, flag in keys}
    for k in ("velocity", "projection_fov"):
        if view[k] is not None:
            view[k] = tuple(view[k])
    return {"kerr_view": view}


def light_delay_from_args(args) -> dict:
    """The light delay of a command line as drivers.render_image / render_video take it: {} without --light_delay."""
    delay = getattr(args, "light_delay", None)
    return {} if delay is None else dict(light_delay=float(delay))


def polarization_from_args(args) -> dict:
    """The polarisation of a command line as drivers.render_image / render_video take it: {} without --polarization or
    --spin_polarization; the latter's goes under ``kerr_polarization``."""
    pol = getattr(args, "polarization", None)
    key = "polarization"
    if pol is None:
        pol, key = getattr(args, "spin_polarization", None), "kerr_polarization"
    if pol is None:
        return {}
    from .polarization import DEFAULT_CELL, DEFAULT_FRACTION, parse_field
    out = {key: dict(field=parse_field(pol), fraction=float(getattr(args, "polarization_fraction", DEFAULT_FRACTION)),
                                 cell=int(getattr(args, "polarization_cell", DEFAULT_CELL)))}
    if getattr(args, "stokes_output", None) is not None:
        out["stokes_path"] = args.stokes_output
    if getattr(args, "polarization_ticks", None) is not None and not getattr(args, "video", False):
        out["ticks_path"] = args.polarization_ticks
    return out


def observer_beta(args):
    """The velocity of a still image's camera: --observer_velocity, or --observer evaluated at --pov; None without either."""
    from . import observer
    if getattr(args, "observer_velocity", None) is not None:
        return observer.check_beta(args.observer_velocity)
    if getattr(args, "observer", None) is not None:
        return tuple(float(v) for v in observer.velocity(args.observer, args.pov))
    return None


def spin_note(args) -> Optional[str]:
    """A note for a disk that reaches inside the innermost stable orbit of its own sense of rotation; None otherwise."""
    from . import kerr
    spin = getattr(args, "spin", 0.0)
    exact = getattr(args, "redshift", "model") == "exact"
    if spin == 0 and not exact:
        return None
    isco = kerr.disk_isco(spin)
    if args.disk_inner_radius >= isco:
        return None
    if exact:
        return (f"Note: --ar1 {args.disk_inner_radius:g} lies inside the ISCO at {isco:.4f} r_s for spin {spin:g}: --redshift exact "
                "shades the matter there as gas that plunges with the ISCO orbit's energy and angular momentum")
    sense = "prograde" if spin > 0 else "retrograde"
    return (f"Note: --ar1 {args.disk_inner_radius:g} lies inside the {sense} ISCO at {isco:.4f} r_s for spin {spin:g}: "
            "matter there plunges, the disk model's circular orbits are a picture only")


def validate_args(args) -> None:
    """Same checks and messages as render.py:4586-4616, plus the backend restrictions."""
    if not (0 < args.fov < 180):
        raise ValueError(f"FOV must be between 0 and 180 degrees, got {args.fov}")
    if args.disk_inner_radius >= args.disk_outer_radius:
        raise ValueError(f"disk_inner_radius ({args.disk_inner_radius}) must be less than "
                         f"disk_outer_radius ({args.disk_outer_radius})")
    if args.step_size <= 0:
        raise ValueError(f"step_size must be positive, got {args.step_size}")
    if not (0.5 <= args.aa_strength <= 2.0):
        raise ValueError(f"aa_strength must be between 0.5 and 2.0, got {args.aa_strength}")
    if args.n_frames <= 0:
        raise ValueError(f"n_frames must be positive, got {args.n_frames}")
    if args.fps <= 0:
        raise ValueError(f"fps must be positive, got {args.fps}")
    if not (1 <= getattr(args, "video_quality", 90) <= 100):
        raise ValueError(f"video_quality must be between 1 and 100, got {args.video_quality}")
    if not math.isfinite(args.orbit_degrees):
        raise ValueError(f"orbit_degrees must be finite, got {args.orbit_degrees}")
    if args.disk_texture and (args.video or args.interactive):
        raise ValueError("--disk_texture only supports still images; video/interactive use the lifecycle system")
    if getattr(args, "disk_model", "texture") != "texture" and (args.video or args.disk_texture):
        raise ValueError("--disk_model v2/v2_volume renders still images and takes no --disk_texture")
    if getattr(args, "device", "hip") == "cpu":
        raise ValueError("--device cpu: this build renders on the MI355X only (no CPU path)")
    if getattr(args, "gpus", 1) < 1:
        raise ValueError(f"gpus must be >= 1, got {args.gpus}")
    if getattr(args, "supersample", 1) > 1 and getattr(args, "gpus", 1) > 1:
        raise ValueError("--supersample renders on one GPU: it does not combine with --gpus > 1")
    thr = getattr(args, "supersample_threshold", None)
    if thr is not None:
        if thr != thr:
            raise ValueError("--supersample_threshold must not be NaN")
        if getattr(args, "supersample", 1) <= 1:
            raise ValueError("--supersample_threshold needs --supersample 2, 4 or 8")
        if getattr(args, "gpus", 1) > 1:
            raise ValueError("--supersample_threshold renders on one GPU: it does not combine with --gpus > 1")
    from . import rules
    rules.refuse_on("bit_depth_16", {name: getattr(args, name) for name in ("bit_depth", "dither", "video_codec") if hasattr(args, name)})
    if getattr(args, "bit_depth", 8) == 16 and not args.video and not args.output.lower().endswith(".png"):
        raise ValueError(f"--bit_depth 16 writes PNG files, got {args.output!r}")
    if not (0.0 <= getattr(args, "shutter", 0.0) <= 1.0):
        raise ValueError(f"shutter must be between 0 and 1, got {args.shutter}")
    if not (1 <= getattr(args, "shutter_samples", 8) <= 64):
        raise ValueError(f"shutter_samples must be between 1 and 64, got {args.shutter_samples}")
    if getattr(args, "tonemap", None) is not None:
        if not (math.isfinite(args.exposure) and -16.0 <= args.exposure <= 16.0):
            raise ValueError(f"exposure must be between -16 and 16 stops, got {args.exposure}")
        if not (math.isfinite(args.white) and 0.0 < args.white <= 65504.0):
            raise ValueError(f"white must be greater than 0 and at most 65504, got {args.white}")
        if getattr(args, "gpus", 1) > 1:
            raise ValueError("--tonemap renders on one GPU: it does not combine with --gpus > 1")
    if getattr(args, "video_hdr", None) is not None:
        if not (math.isfinite(args.hdr_exposure) and -16.0 <= args.hdr_exposure <= 16.0):
            raise ValueError(f"hdr_exposure must be between -16 and 16 stops, got {args.hdr_exposure}")
        if args.video_hdr == "pq" and not (math.isfinite(args.hdr_white) and 0.0 < args.hdr_white <= 10000.0):
            raise ValueError(f"hdr_white must be greater than 0 and at most 10000 nits, got {args.hdr_white}")
        if getattr(args, "gpus", 1) > 1:
            raise ValueError("--video_hdr renders on one GPU: it does not combine with --gpus > 1")
    hdr_output = getattr(args, "hdr_output", None)
    if hdr_output is not None:
        if args.video:
            raise ValueError("--hdr_output writes still images: it does not combine with --video")
        if not hdr_output.lower().endswith((".pfm", ".hdr")):
            raise ValueError(f"--hdr_output writes .pfm or .hdr files, got {hdr_output!r}")
    if getattr(args, "interactive", False):
        raise ValueError("--interactive needs the Taichi GUI and is not part of this build")


def main(argv=None) -> int:
    args = parse_args(argv)
    validate_args(args)
    from . import drivers

    width, height = RESOLUTIONS[args.resolution]
    fov = args.fov % 180
    note = spin_note(args)
    if note:
        print(note)
    spin_kw = {"spin": args.spin} if args.spin != 0 else {}      # without a spin the drivers are called as ever
    if args.redshift != "model":
        spin_kw["redshift"] = args.redshift
    # likewise the moving observer: without one the drivers are called as ever
    moving = args.observer is not None or args.observer_velocity is not None
    sky = args.observer_sky == "shift"
    # ... and the point stars
    stars_kw = {"stars": stars_from_args(args)} if args.stars == "point" else {}
    # ... and a spinning hole's
    kerr_stars_kw = {"kerr_stars": kerr_stars_from_args(args)} if hasattr(args, "spin_stars") else {}
    # ... and a projection, whose frame size follows from the resolution (bhr_amd.projection.frame_size)
    proj_kw = projection_from_args(args)
    if proj_kw:
        from .projection import frame_size
        width, height = frame_size(args.projection, width, height)
    # ... and the Kerr camera, whose projection sizes the frame by the same rule
    view_kw = kerr_view_from_args(args)
    if view_kw and view_kw["kerr_view"]["projection"] is not None:
        from .projection import frame_size
        width, height = frame_size(view_kw["kerr_view"]["projection"], width, height)
    # ... and the light delay
    delay_kw = light_delay_from_args(args)
    # ... and the polarisation
    pol_kw = polarization_from_args(args)
    # ... and the Kerr anti-aliasing
    aa_kw = kerr_anti_alias_from_args(args)
    # ... and the Kerr march's Disk V2 source
    dv2_kw = {"kerr_disk_model": args.spin_disk_model} if hasattr(args, "spin_disk_model") else {}
    # ... and the Kerr line profile
    line_kw = kerr_line_from_args(args)

    if args.video:
        rank = int(os.environ.get("RANK", "0"))
        world = int(os.environ.get("WORLD_SIZE", "1"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        if proj_kw:                                 # several ranks are refused before a device is touched
            drivers.check_projection(world=world, **proj_kw)
        if delay_kw:
            drivers.check_light_delay(delay_kw["light_delay"], world=world)
        if "polarization" in pol_kw:
            drivers.check_polarization(pol_kw["polarization"], video=True, ray_map=args.ray_map, world=world)
        if "kerr_polarization" in pol_kw:
            drivers.check_kerr_polarization(pol_kw["kerr_polarization"], video=True, spin_map=hasattr(args, "spin_map"), orbit=args.orbit,
                                            spin=args.spin, redshift=args.redshift, world=world)
        if hasattr(args, "spin_shutter_map"):
            drivers.check_spin_shutter_map(True, spin=args.spin, redshift=args.redshift, shutter=args.shutter, world=world)
        if kerr_stars_kw:
            drivers.check_kerr_stars(kerr_stars_kw["kerr_stars"], spin=args.spin, redshift=args.redshift, world=world, video=True,
                                     spin_map=hasattr(args, "spin_map"))
        if aa_kw:
            from . import rules
            rules.refuse("kerr_anti_alias", dict(spin=args.spin, redshift=args.redshift, world=world))
        if dv2_kw:
            from . import rules
            rules.refuse("kerr_disk_model", dict(spin=args.spin, redshift=args.redshift, world=world, **dv2_kw))
        if line_kw:
            from . import rules
            rules.refuse("kerr_line", dict(spin=args.spin, redshift=args.redshift, world=world, video=True, spin_map=hasattr(args, "spin_map")))
        if "BHR_FORCE_DEVICE" in os.environ:        # rehearsal: several ranks sharing one card
            local_rank = int(os.environ["BHR_FORCE_DEVICE"])
        elif world > 1:                             # a launcher that shows every rank only its own GPU: ordinal 0
            from . import _lib
            have = int(_lib.load().bhr_device_count())
            if have > 0 and local_rank >= have:
                local_rank %= have
        renderer, _, _, _ = drivers.make_renderer(
            width, height, args.pov, fov, args.step_size, args.texture, args.n_stars, 2048, 1024, args.r_max, None,
            args.disk_inner_radius, args.disk_outer_radius, args.disk_tilt, args.lens_flare, args.anti_alias,
            args.aa_strength, args.disk_rotation_speed, device_index=local_rank, math=args.math, supersample=args.supersample,
            supersample_threshold=args.supersample_threshold, **spin_kw, **stars_kw, **kerr_stars_kw)
        print(f"Rendering video: {args.n_frames} frames at {width}x{height} (rank {rank}/{world})")
        drivers.render_video(renderer, width, height, n_frames=args.n_frames, fps=args.fps,
                             output_path=args.output, fov=fov, static_cam_pos=args.pov, orbit=args.orbit,
                             resume=args.resume, disk_rotation_speed=args.disk_rotation_speed,
                             orbit_degrees=args.orbit_degrees, rank=rank, world=world, video_stream=args.video_stream,
                             png_level=(drivers.DEVICE if args.png_encoder == "device" else drivers.VIDEO_LEVEL),
                             video_codec=args.video_codec, video_quality=args.video_quality, bit_depth=args.bit_depth,
                             dither=args.dither, shutter=args.shutter, shutter_samples=args.shutter_samples,
                             grade=grade_from_args(args), ray_map=args.ray_map, orbit_map=args.orbit_map,
                             shutter_map=args.shutter_map, map_supersample=args.map_supersample, video_hdr=args.video_hdr,
                             hdr_white=args.hdr_white, hdr_exposure=args.hdr_exposure, **stars_kw,
                             **(dict(observer=args.observer, observer_velocity=args.observer_velocity, observer_sky=sky,
                                     infall_to=args.infall_to) if moving else {}), **proj_kw, **delay_kw, **pol_kw, **view_kw,
                             **({"spin_map": True} if hasattr(args, "spin_map") else {}),
                             **({"spin_shutter_map": True} if hasattr(args, "spin_shutter_map") else {}),
                             **({"spin_map_supersample": args.spin_map_supersample} if hasattr(args, "spin_map_supersample") else {}),
                             **kerr_stars_kw, **aa_kw, **dv2_kw, **line_kw)
        if world > 1:
            from . import distributed as D
            dist = D.init("gloo")          # a barrier is all the ranks exchange: frames are independent
            dist.barrier()
            if rank == 0:
                done = D.merge_progress(drivers._frames_dir(args.output), world)
                if len(done) == args.n_frames:
                    drivers.assemble_video(drivers._frames_dir(args.output), args.n_frames, args.fps, args.output,
                                           codec=args.video_codec)
                else:
                    print(f"Warning: only {len(done)}/{args.n_frames} frames completed. Run again with --resume.")
            dist.barrier()
        renderer.close()
        return 0

    img = drivers.render_image(
        width=width, height=height, cam_pos=args.pov, fov=fov, step_size=args.step_size,
        skybox_path=args.texture, n_stars=args.n_stars, r_max=args.r_max, device="hip",
        disk_texture_path=args.disk_texture, r_disk_inner=args.disk_inner_radius,
        r_disk_outer=args.disk_outer_radius, disk_tilt=args.disk_tilt, lens_flare=args.lens_flare,
        anti_alias=args.anti_alias, aa_strength=args.aa_strength, disk_rotation_speed=args.disk_rotation_speed,
        gpus=args.gpus, disk_model=args.disk_model, math=args.math, supersample=args.supersample,
        supersample_threshold=args.supersample_threshold, bit_depth=args.bit_depth, dither=args.dither,
        grade=grade_from_args(args), hdr_path=args.hdr_output, passes_path=args.passes, **spin_kw, **stars_kw,
        **(dict(observer=observer_beta(args), observer_sky=sky) if moving else {}), **proj_kw, **delay_kw, **pol_kw, **view_kw,
        **kerr_stars_kw, **({"kerr_passes_path": args.spin_passes} if hasattr(args, "spin_passes") else {}), **aa_kw, **dv2_kw, **line_kw)
    drivers.save_image(img, args.output, bit_depth=args.bit_depth, dither=args.dither)
    return 0
