"""What may be rendered together: ONE table of feature-combination refusals for the command line (cli.parse_args) and the drivers
(drivers.check_*, render_image, render_video).

FACTS       what the rules look at, with the value that refuses nothing.  A surface builds its facts once (cli.facts_from_args,
            drivers.render_image / render_video); a fact it does not give is the default, and a fact it gives as a function (what
            render_video reads from the renderer) is called when the first rule asks for it, and only then.
CONDITIONS  every predicate over the facts, written once and named.
FEATURES    per feature: when it is on, its words, and ``rows``, the ordered names of the conditions it refuses -- per surface where
            the surfaces differ in order or extent ("cli": the command line, "api": the feature's check_* and through it
            render_image, "video": render_video where it asks more or in another order than "api").  ``say`` has the wording of
            every row, one text or (drivers, command line); braces take the feature's words and the facts.
refusal()   the first row of a feature that the facts violate, as its text; refuse() raises it.  The order of the features is the
            order in which a surface calls refuse(): value checks (a range, a file suffix that is not a row) sit between the calls.

A new feature is one entry of FEATURES (and a condition, where it asks something new), a fact per surface, and one refuse() call
at its place in each surface.
"""
from __future__ import annotations

from collections import ChainMap

FACTS = dict(
    video=False, orbit=False, shutter=0.0, supersample=1, supersample_said=1, supersample_threshold=None, map_supersample=1, spin_map_supersample=1,
    gpus=1, world=1, disk_model="texture", disk_tilt=0.0, anti_alias="disabled", spin=0.0, redshift="model", skybox_path=None, fov_given=False, grade=False,
    # which features are on
    observer=False, projection=False, light_delay=False, stars=False, polarization=False, kerr_polarization=False, spin_observer=False,
    spin_projection=False, kerr_stars=False, passes=False, ray_map=False, orbit_map=False, shutter_map=False, spin_map=False, spin_shutter_map=False,
    kerr_anti_alias=False, kerr_disk_model="texture", kerr_line=False,
    # the paths whose suffix is a row, and what a feature's own validation reads beside its value
    passes_path=None, kerr_passes_path=None, stokes_path=None, ticks_path=None, projection_fov=None, kerr_line_path=None, g_map_path=None,
    # the output side: the HDR stream of a video, the bits per sample
    video_hdr=None, hdr_white_given=False, hdr_exposure_given=False, video_codec="auto", video_stream="auto", width=2, height=2, bit_depth=8, dither="none",
    # the command line's observer flags one by one, and its projection by name
    flag_observer=None, flag_observer_velocity=None, flag_observer_sky=None, flag_infall_to=None, projection_name="perspective",
    # derived, unless a check_* is told them directly
    maps=lambda f: f["ray_map"] or f["orbit_map"] or f["shutter_map"],
    kerr_map=lambda f: f["spin_map"] or f["kerr_polarization"],
    spin_map_supersample_given=lambda f: f["spin_map_supersample"] > 1,      # (the command line: the flag with whatever value)
)


class Facts(dict):
    """The facts of one call: what the surface said, the rest from FACTS; a function is called with the facts once, when a rule asks."""
    def __getitem__(self, name):
        value = dict.__getitem__(self, name) if name in self else FACTS[name]
        if callable(value):
            value = self[name] = value(self)
        return value


def _suffix(path, ext) -> bool:
    return path is not None and not str(path).lower().endswith(ext)


CONDITIONS = {
    "no_spin": lambda f: f["spin"] == 0 and f["redshift"] == "model",
    "spinning": lambda f: f["spin"] != 0 or f["redshift"] != "model",
    "spin": lambda f: f["spin"] != 0,
    "exact": lambda f: f["redshift"] == "exact",
    "video": lambda f: f["video"],
    "no_video": lambda f: not f["video"],
    "orbit": lambda f: f["orbit"],
    "no_orbit": lambda f: not f["orbit"],
    "video_orbit": lambda f: f["video"] and f["orbit"],
    "shutter": lambda f: f["shutter"] > 0,
    "no_shutter": lambda f: not f["shutter"] > 0,
    "marched_shutter": lambda f: f["shutter"] > 0 and not f["spin_shutter_map"],
    "disk_tilt": lambda f: f["disk_tilt"] != 0,
    "orbit_disk_tilt": lambda f: f["orbit"] and f["disk_tilt"] != 0,
    "anti_alias": lambda f: f["anti_alias"] not in ("disabled", 0, False, None),
    "disk_model": lambda f: f["disk_model"] != "texture",
    "supersample_threshold": lambda f: f["supersample_threshold"] is not None,
    # the one real difference between the surfaces: in the drivers supersample=None means "as the renderer is set", which most checks
    # take (supersample); the Kerr maps, the passes and the command line, which always has a number, refuse all but 1 (supersample_set)
    "supersample": lambda f: f["supersample"] not in (None, 1),
    "supersample_set": lambda f: f["supersample"] != 1,
    "supersample_said": lambda f: f["supersample_said"] not in (None, 1),     # render_video's own keyword, before the renderer is asked
    "supersample_or_threshold": lambda f: f["supersample"] != 1 or f["supersample_threshold"] is not None,
    "map_supersample": lambda f: f["map_supersample"] != 1,
    "spin_map_supersample": lambda f: f["spin_map_supersample"] != 1,
    "gpus": lambda f: f["gpus"] != 1,
    "world": lambda f: f["world"] != 1,
    "gpus_or_world": lambda f: f["gpus"] != 1 or f["world"] != 1,
    "grade": lambda f: f["grade"],
    "tiled_spin": lambda f: (f["spin"] != 0 or f["redshift"] != "model") and (f["gpus"] > 1 or f["passes"] or f["disk_model"] != "texture"),
    "not_one_plain_texture_gpu": lambda f: f["gpus"] != 1 or f["supersample"] != 1 or f["disk_model"] != "texture",
    "ray_map": lambda f: f["ray_map"],
    "orbit_map": lambda f: f["orbit_map"],
    "shutter_map": lambda f: f["shutter_map"],
    "spin_map": lambda f: f["spin_map"],
    "spin_shutter_map": lambda f: f["spin_shutter_map"],
    "maps": lambda f: f["maps"],
    "no_maps": lambda f: not f["maps"],
    "video_no_maps": lambda f: f["video"] and not f["maps"],
    "video_no_ray_map": lambda f: f["video"] and not f["ray_map"],
    "video_no_spin_map": lambda f: f["video"] and not f["spin_map"],
    "no_kerr_maps": lambda f: not (f["spin_map"] or f["spin_shutter_map"]),
    "kerr_map": lambda f: f["kerr_map"],
    "passes": lambda f: f["passes"],
    "maps_or_passes": lambda f: f["maps"] or f["passes"],
    "observer": lambda f: f["observer"],
    "projection": lambda f: f["projection"],
    "light_delay": lambda f: f["light_delay"],
    "schwarzschild_marches": lambda f: f["observer"] or f["projection"] or f["light_delay"],
    "stars": lambda f: f["stars"],
    "polarization": lambda f: f["polarization"],
    "kerr_polarization": lambda f: f["kerr_polarization"],
    "spin_observer": lambda f: f["spin_observer"],
    "spin_projection": lambda f: f["spin_projection"],
    "kerr_stars": lambda f: f["kerr_stars"],
    "kerr_passes": lambda f: f["kerr_passes_path"] is not None,
    "kerr_anti_alias": lambda f: f["kerr_anti_alias"],
    "kerr_disk_model": lambda f: f["kerr_disk_model"] != "texture",
    "kerr_line_not_npz": lambda f: _suffix(f["kerr_line_path"], ".npz"),
    "g_map_not_png": lambda f: _suffix(f["g_map_path"], ".png"),
    "g_map_video": lambda f: f["video"] and f["g_map_path"] is not None,
    "kerr_volume_exact": lambda f: f["kerr_disk_model"] == "v2_volume" and f["redshift"] == "exact",
    "sky_texture": lambda f: f["skybox_path"] is not None,
    "fov_given": lambda f: f["fov_given"],
    "video_ticks": lambda f: f["video"] and f["ticks_path"] is not None,
    "passes_not_npz": lambda f: _suffix(f["passes_path"], ".npz"),
    "kerr_passes_not_npz": lambda f: _suffix(f["kerr_passes_path"], ".npz"),
    "stokes_not_npz": lambda f: _suffix(f["stokes_path"], ".npz"),
    "ticks_not_png": lambda f: _suffix(f["ticks_path"], ".png"),
    # the command line's observer flags one by one
    "flag_observer": lambda f: f["flag_observer"] is not None,
    "flag_observer_velocity": lambda f: f["flag_observer_velocity"] is not None,
    "flag_observer_sky": lambda f: f["flag_observer_sky"] is not None,
    "flag_infall_to": lambda f: f["flag_infall_to"] is not None,
    "two_velocities": lambda f: f["flag_observer"] is not None and f["flag_observer_velocity"] is not None,
    "no_velocity": lambda f: f["flag_observer"] is None and f["flag_observer_velocity"] is None,
    "infall_to_other": lambda f: f["flag_infall_to"] is not None and f["flag_observer"] != "infall",
    "infall_to_still": lambda f: f["flag_infall_to"] is not None and not f["video"],
    "infall_to_orbit": lambda f: f["flag_infall_to"] is not None and f["orbit"],
    "no_projection_name": lambda f: f["projection_name"] == "perspective",
    # the output side
    "several_ranks": lambda f: f["world"] > 1,
    "mjpeg": lambda f: f["video_codec"] == "mjpeg",
    "stream_off": lambda f: f["video_stream"] == "off",
    "odd_size": lambda f: f["width"] % 2 or f["height"] % 2,
    "hdr_white_given": lambda f: f["hdr_white_given"],
    "hdr_exposure_given": lambda f: f["hdr_exposure_given"],
    "hlg_white": lambda f: f["video_hdr"] == "hlg" and f["hdr_white_given"],
    "dither": lambda f: f["dither"] != "none",
}

# ---- the wording a family of features shares: one text, or (drivers, command line) -------------------------------------------------------
# a frame marched by a variant of the march: a moving observer, a projection, light delay, the Kerr camera, and on the command line a spin
_MARCH = {
    "no_spin": "{who} needs --spin or --redshift exact: it is the camera of the Kerr march; a hole that does not spin takes --observer and --projection",
    "kerr_map": "{who} does not combine with --spin_map or --spin_polarization: {map}",
    "schwarzschild_marches": "{who} does not combine with --observer, --projection or --light_delay: those marches are Schwarzschild's",
    "disk_tilt": ("{who} does not combine with disk_tilt other than 0: the spin axis is the disk normal",
                  "{who} does not combine with --disk_tilt other than 0: the spin axis is the disk normal"),
    "anti_alias": ("{who} does not combine with anti_alias: {no_diff}", "{who} does not combine with --anti_alias lod_radius: {no_diff}"),
    "disk_model": ("{who} does not combine with disk_model v2 / v2_volume: the {march} march shades the disk texture",
                   "{who} does not combine with --disk_model other than texture: the {march} march shades the disk texture"),
    "supersample_threshold": ("{who} does not combine with supersample_threshold: the {march} march has no refinement kernels (plain supersample works)",
                              "{who} does not combine with --supersample_threshold: the {march} march has no refinement kernels (plain --supersample works)"),
    "gpus_or_world": "{who} renders on one GPU: row-block tiles and frame-sharded ranks march {cam}",
    "gpus": ("{who} renders on one GPU: row-block tiles march {cam}", "{who} does not combine with --gpus other than 1: row-block tiles march {cam}"),
    "world": "{who} renders on one rank: frame-sharded ranks march {cam}",
    "spinning": "{who} does not combine with a spin or the exact redshift: the {march} march is Schwarzschild's, {no_exact}",
    "spin": "{who} does not combine with --spin: the {march} march is Schwarzschild's",
    "exact": "{who} does not combine with --redshift exact: {exact_is}",
    "observer": ("{who} does not combine with a moving observer: the {march} march is the camera's that stands still",
                 "{who} does not combine with --observer, --observer_velocity, --observer_sky or --infall_to: the {march} march is the camera's that stands still"),
    "projection": ("{who} does not combine with a projection: the {march} march is the pinhole camera's",
                   "{who} does not combine with --projection {projection_name}: the {march} march is the pinhole camera's"),
    "passes": ("{who} writes no passes: {map}", "{who} does not combine with --passes: {map}"),
    "shutter": ("{who} does not combine with shutter: shutter frames march {cam}", "{who} does not combine with --shutter: shutter frames march {cam}"),
    "marched_shutter": "{who} does not combine with --shutter: shutter frames march {cam}",
    "maps": "{who} does not combine with ray_map, orbit_map or shutter_map: {map}",
    "maps_or_passes": "{who} does not combine with --ray_map, --orbit_map, --shutter_map or --passes: {map}",
    "ray_map": "{who} does not combine with --ray_map: {map}",
    "orbit_map": "{who} does not combine with --orbit_map: {map}",
    "shutter_map": "{who} does not combine with --shutter_map: {map}",
    "stars": ("{who} does not combine with point stars: they are rendered through a ray map{of_map}",
              "{who} does not combine with --stars point: point stars are rendered through a ray map{of_map}"),
    "fov_given": "{who} does not combine with --fov: that is the pinhole camera's field of view (--projection_fov is this one's)",
}
# a video from ONE ray map
_MAP = {
    "no_spin": "{who} needs --spin or --redshift exact: it is the ray map of the Kerr march; a hole that does not spin takes {plain}",
    "no_video": "{who} needs --video: it is the ray map of {video}",
    "no_orbit": "{who} needs --orbit: a camera that stands still takes --ray_map",
    "no_shutter": "{who} needs --shutter > 0: an instantaneous exposure takes {instant}",
    "orbit": ("a ray map is one view: {who} does not combine with --orbit", "{who} does not combine with --orbit: a ray map is one view"),
    "ray_map": "{who} does not combine with --ray_map: that is {other_map}",
    "orbit_map": "{who} does not combine with --orbit_map: that is {other_map}",
    "shutter_map": "{who} does not combine with --shutter_map: that is {other_map}",
    "spin_map": "{who} does not combine with --spin_map: that is the map of an instantaneous exposure",
    "disk_tilt": ("the orbit is a symmetry of an untilted disk only: {who} needs --disk_tilt 0",
                  "{who} needs --disk_tilt 0: the orbit is a symmetry of an untilted disk only"),
    "orbit_disk_tilt": ("the orbit is a symmetry of an untilted disk only: {who} with --orbit needs --disk_tilt 0",
                        "{who} with --orbit needs --disk_tilt 0: the orbit is a symmetry of an untilted disk only"),
    "shutter": ("shutter frames are marched: {who} does not combine with --shutter", "{who} does not combine with --shutter: shutter frames are marched"),
    "supersample": "{a_map} holds one ray per pixel: {who} does not combine with --supersample > 1",
    "supersample_set": ("{a_map} holds one ray per pixel: {who} does not combine with --supersample > 1",
                        "{who} does not combine with --supersample other than 1: {a_map} holds one ray per pixel"),
    "supersample_said": "{a_map} holds one ray per pixel: {who} does not combine with --supersample > 1",
    "map_supersample": ("{a_map} has no supersampled form: {who} does not combine with --map_supersample > 1",
                        "{who} does not combine with --map_supersample other than 1: {a_map} has no supersampled form"),
    "disk_model": ("a ray map shades the disk texture: {who} does not combine with --disk_model v2 / v2_volume",
                   "{who} does not combine with --disk_model other than texture: a ray map shades the disk texture"),
    "gpus_or_world": "a ray map lives on one GPU: {who} does not combine with --gpus > 1 or several ranks",
    "gpus": "{who} does not combine with --gpus other than 1: a ray map lives on one GPU",
    "observer": "{who} does not combine with --observer: the observer march is Schwarzschild's",
    "projection": ("{who} does not combine with --projection: the projected march is Schwarzschild's", "{who} does not combine with --projection: {schwarzschild}"),
    "light_delay": ("{who} does not combine with --light_delay: the delayed march is Schwarzschild's", "{who} does not combine with --light_delay: {schwarzschild}"),
    "stars": ("{who} does not combine with --stars point: point stars are rendered through the map of Schwarzschild rays",
              "{who} does not combine with --stars point: {schwarzschild}"),
    "polarization": ("{who} does not combine with --polarization: the transport rule is Schwarzschild's", "{who} does not combine with --polarization: {schwarzschild}"),
    "flag_observer": "{who} does not combine with --observer: {schwarzschild}",
    "flag_observer_velocity": "{who} does not combine with --observer_velocity: {schwarzschild}",
    "flag_observer_sky": "{who} does not combine with --observer_sky: {schwarzschild}",
    "flag_infall_to": "{who} does not combine with --infall_to: {schwarzschild}",
    "kerr_polarization": "{who} does not combine with --spin_polarization: shutter frames from the Kerr map have no Stokes planes",
    "spin_observer": "{who} does not combine with --spin_observer: a Kerr ray map holds the rays of the camera at rest",
    "spin_projection": "{who} does not combine with --spin_projection: a Kerr ray map holds the rays of the pinhole camera",
}
# what is rendered THROUGH a ray map: point stars, the Stokes planes, the passes -- of the Schwarzschild map and of the Kerr map
_THROUGH = {
    "no_spin": "{who} needs --spin or --redshift exact: {kerr_own}; a hole that does not spin takes {plain}",
    "sky_texture": ("{who} {does} not combine with a sky texture: a sky image has no catalogue", "{who} does not combine with --texture: a sky image has no catalogue"),
    "spinning": ("{who} {does} not combine with a spin or the exact redshift: {no_spin}", "{who} does not combine with --spin or --redshift exact: {no_spin}"),
    "spin": "{who} does not combine with --spin: {no_spin}",
    "exact": "{who} does not combine with --redshift exact: that is the Kerr march's",
    "observer": ("{who} {does} not combine with a moving observer: {no_observer}",
                 "{who} does not combine with --observer, --observer_velocity, --observer_sky or --infall_to: {no_observer}"),
    "projection": ("{who} does not combine with a projection: {no_projection}", "{who} does not combine with --projection {projection_name}: {no_projection}"),
    "light_delay": ("{who} does not combine with light_delay: {no_delay}", "{who} does not combine with --light_delay: {no_delay}"),
    "stars": "{who} does not combine with --stars point: {no_stars}",
    "polarization": "{who} does not combine with --polarization: that is the hole that does not spin",
    "orbit_map": ("{who} does not combine with orbit_map: {turned}", "{who} does not combine with --orbit_map: {turned}"),
    "video_orbit": "{who} does not combine with --orbit: {turned}",
    "shutter_map": ("{who} {does} not combine with shutter_map: shutter frames from the map have no {planes}",
                    "{who} does not combine with --shutter_map: shutter frames from the map have no {planes}"),
    "spin_shutter_map": "{who} does not combine with --spin_shutter_map: shutter frames from the Kerr map have no {planes}",
    "shutter": ("{who} does not combine with shutter: {no_shutter}", "{who} does not combine with --shutter: {no_shutter}"),
    "map_supersample": ("{who} {does} not combine with map_supersample > 1: {one_ray}", "{who} does not combine with --map_supersample other than 1: {one_ray_cli}"),
    "spin_map_supersample": "{who} does not combine with --spin_map_supersample other than 1: point stars need a Kerr ray map with one ray per pixel",
    "supersample": ("{who} {does} not combine with supersample > 1: {one_ray}", "{who} does not combine with --supersample other than 1: {one_ray_cli}"),
    "supersample_set": ("{who} {does} not combine with supersample > 1: {one_ray}", "{who} does not combine with --supersample other than 1: {one_ray_cli}"),
    "supersample_or_threshold": "{who} does not combine with --supersample other than 1: a Kerr ray map holds one ray per pixel",
    "disk_model": ("{who} {does} not combine with disk_model v2 / v2_volume: a ray map shades the disk texture",
                   "{who} does not combine with --disk_model other than texture: a ray map shades the disk texture"),
    "gpus": ("{who} {render} on one GPU: a ray map lives on one GPU", "{who} does not combine with --gpus other than 1: a ray map lives on one GPU"),
    "world": "{who} {render} on one GPU: a ray map lives on one GPU",
    "gpus_or_world": ("{who} {render} on one GPU: a ray map lives on one GPU", "{who} does not combine with --gpus other than 1: a ray map lives on one GPU"),
    "video_no_maps": ("{who} in a video need ray_map or orbit_map: they are rendered through a ray map",
                      "{who} with --video needs --ray_map or --orbit_map: point stars are rendered through a ray map"),
    "video_no_ray_map": ("{who} in a video needs ray_map: the Stokes planes come from the ray map of a camera that stands still",
                         "{who} with --video needs --ray_map: the Stokes planes come from the ray map of a camera that stands still"),
    "video_no_spin_map": "{who} with --video needs --spin_map: {from_kerr_map}",
    "video": "{who} writes the passes of a still image: it does not combine with --video",
    "video_ticks": ("polarization_ticks is a still image's overlay: a video writes its cell grids to stokes_output",
                    "--polarization_ticks is a still image's overlay: it does not combine with --video (the cell grids go to --stokes_output)"),
    "stokes_not_npz": ("stokes_output is written as a .npz file, got {stokes_path!r}", "--stokes_output writes a .npz file, got {stokes_path!r}"),
    "ticks_not_png": ("polarization_ticks is written as a .png file, got {ticks_path!r}", "--polarization_ticks writes a .png file, got {ticks_path!r}"),
    "spin_observer": "{who} does not combine with --spin_observer: a Kerr ray map holds the rays of the camera at rest",
    "spin_projection": "{who} does not combine with --spin_projection: a Kerr ray map holds the rays of the pinhole camera",
    "ray_map": "{who} does not combine with --ray_map: that is a map of Schwarzschild rays",
    "passes": "{who} does not combine with --passes: that is a map of Schwarzschild rays",
}
_KERR_MAP = dict(a_map="a Kerr ray map", other_map="a map of Schwarzschild rays", schwarzschild="it is a Schwarzschild march's or the Schwarzschild ray map's")
_STILL_CAMERA = "a ray map holds the rays of the camera that stands still"
_PINHOLE = "a ray map holds the rays of the pinhole camera"


def observer_flag(f) -> str:
    """The first of the command line's observer flags that was given: the one its refusals name."""
    return next("--" + n[5:] for n in ("flag_observer", "flag_observer_velocity", "flag_observer_sky", "flag_infall_to") if f[n] is not None)


# ---- the features ------------------------------------------------------------------------------------------------------------------------
FEATURES = {
    "shutter": dict(on=lambda f: f["shutter"] > 0, rows=dict(cli="no_video", api=""),
                    say={"no_video": "--shutter needs --video: a still image is an instantaneous exposure"}),
    # motion blur from the Kerr ray map.  render_video first refuses what the call itself says and asks the renderer (its spin and redshift,
    # its supersampling where the call names none) last
    "spin_shutter_map": dict(
        on=lambda f: f["spin_shutter_map"], say=_MAP,
        words=dict(_KERR_MAP, who="--spin_shutter_map", video="a motion-blurred video", plain="--shutter_map", instant="--spin_map"),
        rows=dict(api="no_spin no_video no_shutter spin_map ray_map orbit_map shutter_map supersample_set map_supersample kerr_polarization spin_observer "
                      "spin_projection observer projection light_delay stars polarization gpus_or_world",
                  video="no_video no_shutter spin_map ray_map orbit_map shutter_map supersample_said map_supersample kerr_polarization spin_observer "
                        "spin_projection observer projection light_delay stars polarization gpus_or_world no_spin supersample_set")),
    "spin_map_supersample": dict(
        on=lambda f: f["spin_map_supersample_given"], rows="no_kerr_maps kerr_polarization",
        say={"no_kerr_maps": ("--spin_map_supersample is the Kerr ray map's factor: it needs --spin_map (marched frames take --supersample)",
                              "--spin_map_supersample needs --spin_map: it is the Kerr ray map's factor (marched frames take --supersample)"),
             "kerr_polarization": "--spin_map_supersample does not combine with --spin_polarization: the Stokes planes need a Kerr ray map with one ray per pixel"}),
    "spin_map": dict(
        on=lambda f: f["spin_map"], say=_MAP, words=dict(_KERR_MAP, who="--spin_map", video="a video", plain="--ray_map or --orbit_map"),
        rows=dict(api="no_spin no_video shutter supersample_set map_supersample gpus_or_world ray_map orbit_map shutter_map observer projection light_delay stars polarization",
                  cli="no_spin no_video shutter supersample_set map_supersample gpus ray_map orbit_map shutter_map flag_observer flag_observer_velocity "
                      "flag_observer_sky flag_infall_to projection light_delay stars polarization")),
    # the Kerr camera (--spin_observer, --spin_projection and their companions; HipRenderer.render_async(kerr_observer=, kerr_projection=))
    "kerr_view": dict(
        on=lambda f: f["spin_observer"] or f["spin_projection"], say=_MARCH,
        words=dict(who="--spin_observer / --spin_projection", march="Kerr", cam="Schwarzschild rays", of_map=" of Schwarzschild rays",
                   no_diff="ray differentials around a spinning hole need Kerr's variational equations", map="a ray map holds the rays of the pinhole camera at rest"),
        rows="no_spin kerr_map schwarzschild_marches disk_tilt anti_alias disk_model supersample_threshold gpus passes shutter maps stars"),
    # the Kerr march on the command line: asked for by a spin, or by the exact redshift at spin 0
    "spin": dict(
        on=lambda f: f["spin"] != 0 or f["redshift"] != "model",
        say={**_MARCH, "tiled_spin": "a spin renders on one GPU with the texture disk source and writes no passes: row-block tiles, ray maps and Disk V2 are Schwarzschild's"},
        words=dict(who=lambda f: "--spin" if f["spin"] != 0 else "--redshift exact (the Kerr march, as with --spin)", march="Kerr", cam="Schwarzschild rays",
                   no_diff="ray differentials around a spinning hole need Kerr's variational equations", map="a ray map holds Schwarzschild rays"),
        rows=dict(cli="disk_tilt anti_alias disk_model supersample_threshold maps_or_passes marched_shutter gpus", api="tiled_spin")),
    "observer": dict(
        on=lambda f: f["observer"], words=dict(who=("a moving observer", observer_flag), march="observer", cam="the camera that stands still", map=_STILL_CAMERA,
                                               no_diff="the differential seeds under aberration are not implemented", no_exact="the exact redshift's observer static",
                                               exact_is="its observer is static"),
        say={**_MARCH, "two_velocities": "--observer names a velocity and --observer_velocity gives one: take one of the two",
             "no_velocity": "{who} needs --observer or --observer_velocity: it belongs to a camera that moves",
             "infall_to_other": "--infall_to needs --observer infall: it is the path of the falling camera",
             "infall_to_still": "--infall_to needs --video: a still image stays at --pov", "infall_to_orbit": "--infall_to does not combine with --orbit: the camera falls radially"},
        rows=dict(api="anti_alias disk_model supersample_threshold gpus spinning passes shutter maps",
                  cli="two_velocities no_velocity spin exact anti_alias disk_model supersample_threshold gpus shutter maps_or_passes infall_to_other infall_to_still infall_to_orbit")),
    "map_supersample": dict(
        on=lambda f: f["map_supersample"] > 1, rows="no_maps",
        say={"no_maps": ("--map_supersample is a ray map's factor: it needs --ray_map, --orbit_map or --shutter_map (marched frames take --supersample)",
                         "--map_supersample needs --ray_map, --orbit_map or --shutter_map: it is a ray map's factor (marched frames take --supersample)")}),
    "shutter_map": dict(
        on=lambda f: f["shutter_map"], say=_MAP,
        words=dict(who="--shutter_map", a_map="a ray map", video="a motion-blurred video", other_map="the map of an instantaneous exposure", instant="--ray_map or --orbit_map"),
        rows=dict(api="no_shutter ray_map orbit_map orbit_disk_tilt supersample disk_model gpus_or_world",
                  cli="no_video no_shutter ray_map orbit_map orbit_disk_tilt supersample_set disk_model gpus")),
    "orbit_map": dict(
        on=lambda f: f["orbit_map"], say=_MAP, words=dict(who="--orbit_map", a_map="a ray map", video="an orbit video", other_map="the map of a camera that stands still"),
        rows=dict(api="no_video no_orbit ray_map disk_tilt shutter supersample disk_model gpus_or_world",
                  cli="no_video no_orbit ray_map disk_tilt shutter supersample_set disk_model gpus")),
    "ray_map": dict(
        on=lambda f: f["ray_map"], words=dict(who="--ray_map", a_map="a ray map"),
        say={**_MAP, "no_video": "--ray_map needs --video: a still image is marched once anyway (--passes writes its ray map's passes)"},
        rows=dict(api="orbit shutter supersample disk_model gpus_or_world", cli="no_video orbit shutter supersample_set disk_model gpus")),
    "passes": dict(
        on=lambda f: f["passes"], words=dict(who="--passes"),
        say={"video": _THROUGH["video"], "passes_not_npz": ("the passes are written as a .npz file, got {passes_path!r}", "--passes writes a .npz file, got {passes_path!r}"),
             "not_one_plain_texture_gpu": "--passes needs one GPU, --supersample 1 and --disk_model texture: the passes come from a ray map",
             "gpus": "the passes come from a ray map, which lives on one GPU: --passes does not combine with --gpus > 1",
             "supersample_set": "a ray map holds one ray per pixel: --passes does not combine with --supersample > 1",
             "disk_model": "a ray map shades the disk texture: --passes does not combine with --disk_model v2 / v2_volume"},
        rows=dict(api="passes_not_npz gpus supersample_set disk_model", cli="video passes_not_npz not_one_plain_texture_gpu")),
    # point stars; in a video the frames that show them are the map's
    "stars": dict(
        on=lambda f: f["stars"], say=_THROUGH,
        words=dict(who=("point stars", "--stars point"), does="do", render="render", no_spin="a ray map holds Schwarzschild rays", no_observer=_STILL_CAMERA,
                   planes="point stars", one_ray="they need a ray map with one ray per pixel", one_ray_cli="point stars need a map with one ray per pixel"),
        rows=dict(api="sky_texture supersample gpus disk_model spinning observer",
                  video="sky_texture supersample gpus disk_model spinning observer shutter_map video_no_maps map_supersample world",
                  cli="sky_texture spinning observer video_no_maps shutter_map map_supersample supersample_set gpus disk_model")),
    "projection": dict(
        on=lambda f: f["projection"], words=dict(who=("a projection", "--projection {projection_name}"), march="projected", cam="the pinhole camera", map=_PINHOLE,
                                                 no_diff="the projected march has no ray differentials", no_exact="with the model redshift",
                                                 exact_is="that is the Kerr march's", of_map=" of the pinhole camera"),
        say={**_MARCH, "no_projection_name": "--projection_fov needs --projection equirect or fisheye: it is the field of view of that camera (the pinhole takes --fov)"},
        rows=dict(api="anti_alias disk_model supersample_threshold gpus_or_world spinning passes shutter maps stars",
                  cli="no_projection_name fov_given spin exact anti_alias disk_model supersample_threshold gpus shutter ray_map orbit_map shutter_map passes stars")),
    "light_delay": dict(
        on=lambda f: f["light_delay"], say=_MARCH,
        words=dict(who=("light_delay", "--light_delay"), march="delayed", cam="without the light's travel time", map="a ray map's records hold no travel time",
                   no_diff="the delayed march has no ray differentials", no_exact="with the model redshift", exact_is="that is the Kerr march's",
                   of_map=", whose records hold no travel time"),
        rows=dict(api="anti_alias disk_model supersample_threshold gpus world spinning observer projection passes shutter maps stars",
                  cli="anti_alias disk_model supersample_threshold gpus spin exact observer projection shutter ray_map orbit_map shutter_map passes stars")),
    "polarization": dict(
        on=lambda f: f["polarization"], say=_THROUGH,
        words=dict(who=("polarization", "--polarization"), does="does", render="renders", no_observer=_STILL_CAMERA, no_projection=_PINHOLE,
                   no_spin="the transport rule is Schwarzschild's and a ray map holds Schwarzschild rays", no_delay="a ray map's records hold no travel time",
                   turned="the Stokes planes are the build view's, turned views have none", planes="Stokes planes",
                   no_shutter="shutter frames are marched, the Stokes planes come from a ray map", one_ray="the Stokes planes need a map with one ray per pixel",
                   one_ray_cli="the Stokes planes need a map with one ray per pixel"),
        rows=dict(api="spinning observer projection light_delay orbit_map shutter_map shutter map_supersample supersample disk_model gpus_or_world video_no_ray_map "
                      "video_ticks stokes_not_npz ticks_not_png",
                  cli="spin exact observer projection light_delay orbit_map shutter_map shutter map_supersample supersample_set disk_model gpus video_no_ray_map "
                      "video_ticks stokes_not_npz ticks_not_png")),
    "kerr_polarization": dict(
        on=lambda f: f["kerr_polarization"],
        say={**_THROUGH, "orbit_map": _THROUGH["ray_map"].replace("ray_map", "orbit_map"), "shutter_map": _THROUGH["ray_map"].replace("ray_map", "shutter_map"),
             "map_supersample": "{who} does not combine with --map_supersample other than 1: a Kerr ray map has no supersampled form",
             "gpus_or_world": _THROUGH["gpus"][1], "gpus": _THROUGH["gpus"][1], "disk_model": "{who} does not combine with --disk_model other than texture: a ray map shades the disk texture",
             "observer": ("{who} does not combine with --observer: {no_observer}", _THROUGH["observer"][1]), "projection": "{who} does not combine with --projection: {no_observer}",
             "light_delay": "{who} does not combine with --light_delay: {no_observer}", "shutter": "{who} does not combine with --shutter: shutter frames are marched",
             "supersample_set": _THROUGH["supersample_or_threshold"]},
        words=dict(who="--spin_polarization", kerr_own="it is the polarisation of the Kerr march", plain="--polarization", turned="the Stokes planes are the build view's, turned views have none",
                   from_kerr_map="the Stokes planes come from the Kerr ray map", no_observer=_KERR_MAP["schwarzschild"], no_stars=_KERR_MAP["schwarzschild"]),
        rows=dict(api="polarization no_spin video_no_spin_map video_orbit video_ticks shutter supersample_or_threshold map_supersample gpus_or_world ray_map orbit_map "
                      "shutter_map passes observer projection light_delay stars disk_model stokes_not_npz ticks_not_png",
                  # (render_video has never refused a supersample_threshold here: the frames come from the map, which has no refinement pass)
                  video="polarization no_spin video_no_spin_map video_orbit video_ticks shutter supersample_set map_supersample gpus_or_world ray_map orbit_map "
                        "shutter_map passes observer projection light_delay stars disk_model stokes_not_npz ticks_not_png",
                  cli="polarization no_spin video_no_spin_map video_orbit shutter supersample_or_threshold map_supersample gpus ray_map orbit_map shutter_map passes "
                      "observer projection light_delay stars disk_model video_ticks stokes_not_npz ticks_not_png")),
    # the Kerr point stars and the Kerr passes: each names its flag and the other one, on both surfaces alike
    "kerr_stars": dict(
        on=lambda f: f["kerr_stars"],
        say={**_THROUGH, "sky_texture": _THROUGH["sky_texture"][1], "supersample": "{who} does not combine with --supersample other than 1: a Kerr ray map holds one ray per pixel",
             "shutter": "{who} does not combine with --shutter: shutter frames are marched, point stars are rendered through the Kerr ray map",
             "gpus_or_world": "{who} does not combine with --gpus other than 1 or several ranks: a ray map lives on one GPU",
             "kerr_polarization": "--spin_stars does not combine with --spin_polarization on one command line: take one of the two"},
        words=dict(who="--spin_stars", kerr_own="they are the point stars of the Kerr ray map", plain="--stars point", planes="point stars",
                   no_stars="that is the catalogue of the map of Schwarzschild rays", from_kerr_map="point stars are rendered through the Kerr ray map"),
        rows=dict(api="no_spin sky_texture stars supersample spin_map_supersample spin_shutter_map shutter spin_observer spin_projection gpus_or_world video_no_spin_map",
                  cli="no_spin sky_texture stars supersample spin_map_supersample spin_shutter_map shutter spin_observer spin_projection gpus_or_world video_no_spin_map "
                      "kerr_polarization")),
    "kerr_passes": dict(
        on=lambda f: f["kerr_passes_path"] is not None,
        say={**_THROUGH, "kerr_passes_not_npz": "{who} writes a .npz file, got {kerr_passes_path!r}", "gpus": "{who} does not combine with --gpus other than 1: a ray map lives on one GPU",
             "supersample": "{who} does not combine with --supersample other than 1: a Kerr ray map holds one ray per pixel"},
        words=dict(who="--spin_passes", kerr_own="the passes come from the Kerr ray map", plain="--passes"),
        rows="no_spin video kerr_passes_not_npz supersample spin_observer spin_projection gpus"),
    # anti-aliasing of the Kerr march (--spin_anti_alias lod_radius; HipRenderer.set_kerr_anti_alias): marched frames of the pinhole
    # camera at rest, on one GPU -- the same words on both surfaces, each naming both flags
    "kerr_anti_alias": dict(
        on=lambda f: f["kerr_anti_alias"],
        words=dict(who="--spin_anti_alias", no_words="a Kerr ray map's record has no differential words"),
        say={"no_spin": "{who} needs --spin or --redshift exact: it is the anti-aliasing of the Kerr march; a hole that does not spin takes --anti_alias lod_radius",
             "spin_map": "{who} does not combine with --spin_map: {no_words}",
             "spin_shutter_map": "{who} does not combine with --spin_shutter_map: {no_words}",
             "kerr_polarization": "{who} does not combine with --spin_polarization: {no_words}",
             "kerr_stars": "{who} does not combine with --spin_stars: {no_words}",
             "kerr_passes": "{who} does not combine with --spin_passes: {no_words}",
             "spin_observer": "{who} does not combine with --spin_observer: the differential seeds would need the aberration's Jacobian",
             "spin_projection": "{who} does not combine with --spin_projection: the differential seeds are the pinhole camera's",
             "gpus_or_world": "{who} does not combine with --gpus other than 1 or several ranks: row-block tiles and frame-sharded ranks march Schwarzschild rays"},
        rows="no_spin spin_map spin_shutter_map kerr_polarization kerr_stars kerr_passes spin_observer spin_projection gpus_or_world"),
    # the Kerr march's own Disk V2 sources (--spin_disk_model v2 | v2_volume; HipRenderer.use_kerr_disk_v2): marched frames of the pinhole
    # camera at rest, on one GPU, stills and videos -- the same words on both surfaces, each naming both flags
    "kerr_disk_model": dict(
        on=lambda f: f["kerr_disk_model"] != "texture",
        words=dict(who="--spin_disk_model", texture="shades the disk texture"),
        say={"no_spin": "{who} needs --spin or --redshift exact: it is the Disk V2 source of the Kerr march; a hole that does not spin takes --disk_model",
             "disk_model": "{who} does not combine with --disk_model other than texture: that is the Schwarzschild march's source, which a spin refuses",
             "spin_map": "{who} does not combine with --spin_map: a frame from the Kerr ray map {texture}",
             "spin_shutter_map": "{who} does not combine with --spin_shutter_map: a frame from the Kerr ray map {texture}",
             "kerr_polarization": "{who} does not combine with --spin_polarization: a frame from the Kerr ray map {texture}",
             "kerr_stars": "{who} does not combine with --spin_stars: a frame from the Kerr ray map {texture}",
             "kerr_passes": "{who} does not combine with --spin_passes: a frame from the Kerr ray map {texture}",
             "spin_observer": "{who} does not combine with --spin_observer: the Kerr camera's march {texture}",
             "spin_projection": "{who} does not combine with --spin_projection: the Kerr camera's march {texture}",
             "kerr_anti_alias": "{who} does not combine with --spin_anti_alias: the analytic source has no mip chain",
             "gpus_or_world": "{who} does not combine with --gpus other than 1 or several ranks: row-block tiles and frame-sharded ranks march Schwarzschild rays",
             "kerr_volume_exact": "{who} v2_volume does not combine with --redshift exact: gas off the equatorial plane has no four-velocity in this model (v2 takes it)"},
        rows="no_spin disk_model spin_map spin_shutter_map kerr_polarization kerr_stars kerr_passes spin_observer spin_projection kerr_anti_alias gpus_or_world "
             "kerr_volume_exact"),
    # the Kerr line profile and the redshift map (--spin_line, --spin_g_map; HipRenderer.set_kerr_line): a pass over the k = 1 Kerr ray
    # map of the camera at rest, on one GPU -- the same words on both surfaces; --spin_polarization, --spin_stars and --spin_passes may
    # stand beside it
    "kerr_line": dict(
        on=lambda f: f["kerr_line"],
        words=dict(who="--spin_line / --spin_g_map", one_ray="the line pass needs a Kerr ray map with one ray per pixel"),
        say={"no_spin": "{who} needs --spin or --redshift exact: the line profile is a pass over the Kerr ray map",
             "video_no_spin_map": "{who} with --video needs --spin_map: the line profile comes from the Kerr ray map",
             "video_orbit": "{who} does not combine with --orbit: the line pass walks the build view's records, turned views have none",
             "shutter": "{who} does not combine with --shutter: a mean of frames has no line profile",
             "supersample_or_threshold": "{who} does not combine with --supersample other than 1: a Kerr ray map holds one ray per pixel",
             "spin_map_supersample": "{who} does not combine with --spin_map_supersample other than 1: {one_ray}",
             "spin_shutter_map": "{who} does not combine with --spin_shutter_map: a mean of frames has no line profile",
             "spin_observer": "{who} does not combine with --spin_observer: a Kerr ray map holds the rays of the camera at rest",
             "spin_projection": "{who} does not combine with --spin_projection: the solid angle of a pixel is the pinhole camera's",
             "kerr_anti_alias": "{who} does not combine with --spin_anti_alias: a Kerr ray map's record has no differential words",
             "kerr_disk_model": "{who} does not combine with --spin_disk_model other than texture: a frame from the Kerr ray map shades the disk texture",
             "gpus_or_world": "{who} does not combine with --gpus other than 1 or several ranks: a ray map lives on one GPU",
             "kerr_line_not_npz": "--spin_line writes a .npz file, got {kerr_line_path!r}",
             "g_map_not_png": "--spin_g_map writes a .png file, got {g_map_path!r}",
             "g_map_video": "--spin_g_map is a still image's map: it does not combine with --video (the spectra go to --spin_line)"},
        rows="no_spin video_no_spin_map video_orbit shutter supersample_or_threshold spin_map_supersample spin_shutter_map spin_observer spin_projection "
             "kerr_anti_alias kerr_disk_model gpus_or_world kerr_line_not_npz g_map_not_png g_map_video"),
    # a still image tiled in row blocks over several GPUs (render_image)
    "tiles": dict(on=lambda f: f["gpus"] > 1, rows=dict(api="grade supersample_set", cli=""),
                  say={"grade": "a grade renders on one GPU: row-block tiles store their rows from inside the V pass",
                       "supersample_set": "supersample > 1 renders on one GPU: row-block tiles march one ray per pixel"}),
    # the output side: the HDR stream of a video (and its two companions without it), 16-bit output
    "video_hdr": dict(on=lambda f: f["video_hdr"] is not None, rows=dict(api="several_ranks mjpeg stream_off odd_size", cli="no_video hlg_white mjpeg stream_off"),
                      say={"several_ranks": "the HDR stream is written by one rank in frame order: --video_hdr does not combine with several ranks",
                           "mjpeg": "--video_hdr does not combine with --video_codec mjpeg: that mode writes no stream",
                           "stream_off": "--video_hdr is a video stream: it does not combine with --video_stream off",
                           "odd_size": "the HDR stream is 4:2:0 and needs even frame sizes, got {width}x{height}",
                           "no_video": "--video_hdr needs --video: it is the HDR stream of a video (still images take --hdr_output)",
                           "hlg_white": "--hdr_white is PQ's: HLG is scene-referred and places scene value 1.0 at its 75 % reference white"}),
    "no_video_hdr": dict(on=lambda f: f["video_hdr"] is None, rows=dict(api="", cli="hdr_white_given hdr_exposure_given"),
                         say={"hdr_white_given": "--hdr_white needs --video_hdr pq: it is the display level of the PQ stream's scene value 1.0",
                              "hdr_exposure_given": "--hdr_exposure needs --video_hdr: it is the exposure of the HDR stream"}),
    "bit_depth_16": dict(on=lambda f: f["bit_depth"] == 16, rows="dither mjpeg",
                         say={"dither": "--bit_depth 16 is not dithered: --dither blue applies to 8-bit output",
                              "mjpeg": "--bit_depth 16 does not combine with --video_codec mjpeg: JPEG frames are 8-bit"}),
}


def refusal(feature: str, facts, surface: str = "api"):
    """The text of the first row of ``feature`` that ``facts`` (a dict, or Facts) violate on ``surface``, or None.  Whether the feature
    is on is the caller's matter (refuse_on asks)."""
    f = facts if isinstance(facts, Facts) else Facts(facts)
    entry = FEATURES[feature]
    rows = entry["rows"]
    if isinstance(rows, dict):
        rows = rows.get(surface, rows["api"])          # "video": as "api" where the feature has no rows of its own for it
    cli = surface == "cli"
    for name in rows.split():
        if CONDITIONS[name](f):
            text = entry["say"][name]
            words = {k: v[cli] if isinstance(v, tuple) else v for k, v in entry.get("words", {}).items()}
            words = {k: v(f) if callable(v) else v.format_map(f) for k, v in words.items()}
            return (text if isinstance(text, str) else text[cli]).format_map(ChainMap(words, f))
    return None


def refuse(feature: str, facts, surface: str = "api") -> None:
    """Raises ValueError with refusal()'s text, if there is one."""
    text = refusal(feature, facts, surface)
    if text is not None:
        raise ValueError(text)


def refuse_on(features, facts, surface: str = "api") -> None:
    """refuse() for every one of ``features`` (names separated by blanks) that is on, in that order."""
    f = facts if isinstance(facts, Facts) else Facts(facts)
    for feature in features.split():
        if FEATURES[feature]["on"](f):
            refuse(feature, f, surface)
