"""--projection on the command line and in the drivers: it parses, the frame size follows the resolution, its refusals fire before
any device is touched, the defaults change nothing, the keyword reaches the drivers and the progress record only when it is set,
and the project's own muxer marks a full-sphere equirect video as spherical -- and nothing else.  No GPU."""
import json
import struct
import zlib

import numpy as np
import pytest

from bhr_amd import cli, drivers, mp4, projection

# the default namespace before the projections existed (vars(cli.parse_args([])))
BEFORE = json.loads("""{"aa_strength": 1.0, "anti_alias": "disabled", "bit_depth": 8, "device": "hip", "disk_generation_scale": 2,
"disk_inner_radius": 2.0, "disk_model": "texture", "disk_outer_radius": 15.0, "disk_rotation_algorithm": "baseline", "disk_rotation_speed": 0.1,
"disk_texture": null, "disk_tilt": 0.0, "dither": "none", "exposure": null, "force_regenerate_disk_texture": false, "fov": 90, "fps": 36,
"gpus": 1, "hdr_exposure": 0.0, "hdr_output": null, "hdr_white": 203.0, "ignore_taichi_cache": false, "infall_to": null, "interactive": false,
"keyframes_count": 10, "lens_flare": false, "map_supersample": 1, "math": "hybrid", "n_frames": 3600, "n_stars": 6000, "observer": null,
"observer_sky": "shift", "observer_velocity": null, "orbit": false, "orbit_degrees": 360.0, "orbit_map": false, "output": "output/blackhole.png",
"passes": null, "png_encoder": "device", "pov": [6, 0, 0.5], "r_max": 10, "ray_map": false, "redshift": "model", "resolution": "fhd",
"resume": false, "shutter": 0.0, "shutter_map": false, "shutter_samples": 8, "spin": 0.0, "star_gain": 2.0, "star_max_magnification": 32.0,
"stars": "texture", "step_size": 0.1, "supersample": 1, "supersample_threshold": null, "texture": null, "tonemap": null, "transfer": null,
"video": false, "video_codec": "auto", "video_hdr": null, "video_quality": 90, "video_stream": "auto", "white": null}""")
NEW = {"projection": "perspective", "projection_fov": None}


# ---- parsing, defaults, the frame size ----------------------------------------------------------------------------------------------
def test_projection_parses():
    a = cli.parse_args(["--projection", "equirect"])
    assert (a.projection, a.projection_fov, a.fov) == ("equirect", None, 90)
    cli.validate_args(a)
    assert cli.projection_from_args(a) == {"projection": "equirect", "projection_fov": None}
    a = cli.parse_args(["--projection", "equirect", "--projection_fov", "120", "60"])
    assert cli.projection_from_args(a) == {"projection": "equirect", "projection_fov": (120.0, 60.0)}
    a = cli.parse_args(["--projection", "fisheye", "--projection_fov", "220"])
    assert cli.projection_from_args(a) == {"projection": "fisheye", "projection_fov": (220.0,)}
    assert cli.projection_from_args(cli.parse_args([])) == {} == cli.projection_from_args(cli.parse_args(["--projection", "perspective"]))
    # what works with a projection: plain supersampling, a tilted disk, the lens flare, grading, HDR, video, an orbit, an observer
    for kind in projection.KINDS:
        cli.parse_args(["--projection", kind, "--supersample", "2", "--disk_tilt", "20", "--lens_flare", "--tonemap", "aces", "--video", "--orbit",
                        "--video_hdr", "pq", "--math", "fast", "--observer", "circular"])
        cli.parse_args(["--projection", kind, "--observer", "infall", "--video", "--infall_to", "2", "--video_codec", "mjpeg"])
        cli.parse_args(["--projection", kind, "--observer_velocity", "0.1", "0.2", "0.3", "--observer_sky", "plain", "--hdr_output", "x.pfm"])


def test_projection_defaults():
    assert projection.check("equirect") == ("equirect", 360.0, 180.0)
    assert projection.check("fisheye") == ("fisheye", 180.0, 0.0)
    assert projection.check("equirect", (120, 60)) == ("equirect", 120.0, 60.0)
    assert projection.check("fisheye", (360,)) == ("fisheye", 360.0, 0.0) == projection.check("fisheye", 360)
    assert projection.full_sphere("equirect") and projection.full_sphere("equirect", (360.0, 180.0))
    assert not projection.full_sphere("equirect", (360.0, 90.0)) and not projection.full_sphere("equirect", (180.0, 180.0))
    assert not projection.full_sphere("fisheye") and not projection.full_sphere("fisheye", (360.0,)) and not projection.full_sphere(None)
    for kind, fov in (("cube", None), (None, None), ("perspective", None), ("equirect", (360.0,)), ("equirect", (360.0, 180.0, 1.0)), ("fisheye", (180.0, 90.0)),
                      ("equirect", (0.0, 90.0)), ("equirect", (360.5, 90.0)), ("equirect", (360.0, 180.5)), ("equirect", (360.0, -1.0)),
                      ("equirect", (float("nan"), 90.0)), ("equirect", (90.0, float("nan"))), ("fisheye", (0.0,)), ("fisheye", (360.5,)),
                      ("fisheye", (float("nan"),)), ("fisheye", (float("inf"),)), ("fisheye", ("wide",))):
        with pytest.raises(ValueError):
            projection.check(kind, fov)


def test_frame_size_rule():
    sizes = {"8k": ((7680, 3840), (4320, 4320)), "4k": ((3840, 1920), (2160, 2160)), "fhd": ((1920, 960), (1080, 1080)),
             "hd": ((1280, 640), (720, 720)), "sd": ((640, 320), (360, 360))}
    assert set(sizes) == set(cli.RESOLUTIONS)
    for name, (eq, fish) in sizes.items():
        w, h = cli.RESOLUTIONS[name]
        assert projection.frame_size("equirect", w, h) == eq and projection.frame_size("fisheye", w, h) == fish
        assert projection.frame_size("perspective", w, h) == (w, h) == projection.frame_size(None, w, h)
    with pytest.raises(ValueError):
        projection.frame_size("cube", 1920, 1080)


def test_defaults_change_nothing():
    ns = vars(cli.parse_args([]))
    assert ns == {**BEFORE, **NEW}                           # today's namespace and the two new keys
    for line in (["--video", "--orbit", "--supersample", "2"], ["--disk_tilt", "20", "--anti_alias", "lod_radius", "--gpus", "2"], ["--spin", "0.5"],
                 ["--video", "--shutter", "0.5", "--shutter_map"], ["--fov", "60"], ["--observer", "circular"], ["--stars", "point"]):
        ns = vars(cli.parse_args(line))
        assert {k: ns[k] for k in NEW} == NEW and set(ns) == set(BEFORE) | set(NEW)
        assert ns == vars(cli.parse_args(line + ["--projection", "perspective"]))
    assert cli.parse_args(["--fov", "60"]).fov == 60.0 and cli.parse_args(["--fov", "90"]).fov == 90.0
    with_proj = vars(cli.parse_args(["--video", "--orbit", "--supersample", "2", "--projection", "fisheye"]))
    plain = vars(cli.parse_args(["--video", "--orbit", "--supersample", "2"]))
    assert {k: v for k, v in with_proj.items() if k != "projection"} == {k: v for k, v in plain.items() if k != "projection"}


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
FLAGS = (["--projection", "equirect"], ["--projection", "fisheye"], ["--projection", "fisheye", "--projection_fov", "200"])


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "_".join(f[1:]))
@pytest.mark.parametrize("extra, word", [
    (["--spin", "0.7"], "--spin"),
    (["--redshift", "exact"], "--redshift exact"),
    (["--anti_alias", "lod_radius"], "--anti_alias"),
    (["--disk_model", "v2"], "--disk_model"),
    (["--disk_model", "v2_volume"], "--disk_model"),
    (["--supersample", "2", "--supersample_threshold", "0.1"], "--supersample_threshold"),
    (["--gpus", "2"], "--gpus"),
    (["--video", "--shutter", "0.5"], "--shutter"),
    (["--video", "--shutter", "0.5", "--shutter_samples", "4"], "--shutter"),
    (["--video", "--ray_map"], "--ray_map"),
    (["--video", "--orbit", "--orbit_map"], "--orbit_map"),
    (["--video", "--shutter", "0.5", "--shutter_map"], "--shutter"),
    (["--passes", "x.npz"], "--passes"),
    (["--stars", "point"], "--stars point"),
    (["--fov", "90"], "--fov"),
    (["--fov", "60"], "--fov"),
])
def test_projection_refusals_are_argparse_errors(flags, extra, word, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(flags + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--projection" in err and word in err
    cli.parse_args(extra)                                         # the same line with the pinhole camera parses
    cli.parse_args(flags)


@pytest.mark.parametrize("line, word", [
    (["--projection_fov", "180"], "needs --projection"),
    (["--projection", "perspective", "--projection_fov", "180"], "needs --projection"),
    (["--projection", "equirect", "--projection_fov", "180"], "(h, v)"),
    (["--projection", "fisheye", "--projection_fov", "180", "90"], "(full_angle,)"),
    (["--projection", "equirect", "--projection_fov", "361", "90"], "360"),
    (["--projection", "equirect", "--projection_fov", "360", "181"], "180"),
    (["--projection", "equirect", "--projection_fov", "0", "90"], "outside"),
    (["--projection", "fisheye", "--projection_fov", "nan"], "outside"),
    (["--projection", "fisheye", "--projection_fov", "400"], "360"),
    (["--projection", "cube"], "invalid choice"),
])
def test_projection_argument_errors(line, word, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(line)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--projection" in err and word in err


def test_driver_checks_need_no_device():
    assert drivers.check_projection(None, anti_alias="lod_radius", gpus=4, spin=0.9) is None      # the pinhole camera: nothing to check
    assert drivers.check_projection("equirect") == ("equirect", 360.0, 180.0)
    assert drivers.check_projection("fisheye", (200.0,)) == ("fisheye", 200.0, 0.0)
    for kw, word in ((dict(anti_alias="lod_radius"), "anti_alias"), (dict(disk_model="v2"), "disk_model"), (dict(disk_model="v2_volume"), "disk_model"),
                     (dict(supersample_threshold=0.1), "supersample_threshold"), (dict(gpus=2), "one GPU"), (dict(world=2), "one GPU"),
                     (dict(spin=0.5), "spin"), (dict(redshift="exact"), "exact redshift"), (dict(passes=True), "passes"), (dict(shutter=0.5), "shutter"),
                     (dict(maps=True), "ray_map"), (dict(stars=True), "point stars")):
        for kind in projection.KINDS:
            with pytest.raises(ValueError, match="projection") as e:
                drivers.check_projection(kind, **kw)
            assert word in str(e.value)
    with pytest.raises(ValueError, match="needs a projection"):
        drivers.check_projection(None, (180.0,))
    with pytest.raises(ValueError):
        drivers.check_projection("fisheye", (400.0,))
    with pytest.raises(ValueError):
        drivers.check_projection("cube")
    with pytest.raises(ValueError, match="projection"):           # the drivers refuse before any device work
        drivers.render_image(64, 32, [6, 0, 0.5], 90.0, 0.1, projection="equirect", spin=0.5)
    with pytest.raises(ValueError, match="projection"):
        drivers.render_image(64, 32, [6, 0, 0.5], 90.0, 0.1, projection="fisheye", gpus=2)
    with pytest.raises(ValueError, match="projection_fov"):
        drivers.render_image(64, 32, [6, 0, 0.5], 90.0, 0.1, projection_fov=(180.0,))


# ---- the keyword reaches the drivers and the progress record only when it is set -------------------------------------------------------
def _run_main(monkeypatch, argv):
    seen = {}

    def render_image(**kw):
        seen["image"] = kw
        return np.zeros((2, 2, 3), dtype=np.float32)

    class Renderer:
        def close(self):
            pass

    def make_renderer(*a, **kw):
        seen["renderer"] = (a, kw)
        return Renderer(), None, None, None

    def render_video(renderer, width, height, **kw):
        seen["video"] = dict(kw, width=width, height=height)

    monkeypatch.setattr(drivers, "render_image", render_image)
    monkeypatch.setattr(drivers, "make_renderer", make_renderer)
    monkeypatch.setattr(drivers, "render_video", render_video)
    monkeypatch.setattr(drivers, "save_image", lambda *a, **kw: None)
    assert cli.main(argv) == 0
    return seen


def test_the_default_passes_no_keyword(monkeypatch):
    for argv in ([], ["--projection", "perspective"], ["--observer", "circular"], ["--supersample", "2"]):
        kw = _run_main(monkeypatch, argv)["image"]
        assert "projection" not in kw and "projection_fov" not in kw and (kw["width"], kw["height"]) == (1920, 1080), argv
        seen = _run_main(monkeypatch, argv + ["--video"])
        assert "projection" not in seen["video"] and "projection_fov" not in seen["video"], argv
        assert (seen["video"]["width"], seen["video"]["height"]) == (1920, 1080) == seen["renderer"][0][:2]


def test_the_projection_reaches_the_drivers(monkeypatch):
    kw = _run_main(monkeypatch, ["--projection", "equirect"])["image"]
    assert (kw["projection"], kw["projection_fov"], kw["width"], kw["height"]) == ("equirect", None, 1920, 960) and "observer" not in kw
    kw = _run_main(monkeypatch, ["--projection", "fisheye", "--projection_fov", "220", "-r", "hd", "--observer", "circular"])["image"]
    assert (kw["projection"], kw["projection_fov"], kw["width"], kw["height"]) == ("fisheye", (220.0,), 720, 720) and len(kw["observer"]) == 3
    seen = _run_main(monkeypatch, ["--projection", "equirect", "--projection_fov", "180", "90", "-r", "sd", "--video", "--orbit", "--observer", "circular"])
    kw = seen["video"]
    assert (kw["projection"], kw["projection_fov"], kw["width"], kw["height"]) == ("equirect", (180.0, 90.0), 640, 320)
    assert kw["observer"] == "circular" and kw["orbit"] is True and seen["renderer"][0][:2] == (640, 320)


def test_several_ranks_are_refused_before_a_renderer_exists(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setattr(drivers, "make_renderer", lambda *a, **kw: pytest.fail("a renderer was made"))
    with pytest.raises(ValueError, match="one GPU"):
        cli.main(["--projection", "equirect", "--video"])


def test_progress_params_carry_the_projection_only_when_set():
    base = drivers.progress_params(4, 90.0, True, 0.1, 360.0)
    assert "projection" not in base
    p = drivers.progress_params(4, 90.0, True, 0.1, 360.0, projection={"kind": "equirect", "fov": [360.0, 180.0]})
    assert p == {**base, "projection": {"kind": "equirect", "fov": [360.0, 180.0]}}
    other = drivers.progress_params(4, 90.0, True, 0.1, 360.0, projection={"kind": "fisheye", "fov": [180.0, 0.0]})
    assert other != p and other != base                           # a resume under another projection starts over


# ---- the spherical box ------------------------------------------------------------------------------------------------------------------
def _png(path, w, h, seed):
    """A small valid RGB PNG."""
    rng = np.random.default_rng(seed)
    rows = b"".join(b"\0" + rng.integers(0, 256, w * 3, dtype=np.uint8).tobytes() for _ in range(h))

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    path.write_bytes(mp4.PNG_MAGIC + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows)) + chunk(b"IEND", b""))
    return str(path)


def _boxes(buf, start, end, path=()):
    """[(path of box kinds, payload start, payload end)] of every box under [start, end), containers walked."""
    out, at = [], start
    while at + 8 <= end:
        size, kind = struct.unpack_from(">I4s", buf, at)
        head = 8
        if size == 1:
            size, head = struct.unpack_from(">Q", buf, at + 8)[0], 16
        assert size >= head and at + size <= end, (kind, at, size)
        out.append((path + (kind,), at + head, at + size))
        if kind in (b"moov", b"trak", b"mdia", b"minf", b"stbl", b"dinf"):
            out += _boxes(buf, at + head, at + size, path + (kind,))
        at += size
    return out


def _frames(tmp_path, w, h, n=3):
    return [_png(tmp_path / f"frame_{k:04d}.png", w, h, k) for k in range(n)]


def test_spherical_box_marks_the_full_sphere_equirect_video_only(tmp_path):
    paths = _frames(tmp_path, 16, 8)
    plain, sph = str(tmp_path / "plain.mp4"), str(tmp_path / "sph.mp4")
    n_plain, n_sph = mp4.write_png_mp4(paths, 30, plain, 16, 8), mp4.write_png_mp4(paths, 30, sph, 16, 8, spherical=True)
    a, b = open(plain, "rb").read(), open(sph, "rb").read()
    assert len(a) == n_plain and len(b) == n_sph
    assert not [x for x in _boxes(a, 0, len(a)) if x[0][-1] == b"uuid"]
    found = [x for x in _boxes(b, 0, len(b)) if x[0][-1] == b"uuid"]
    assert len(found) == 1 and found[0][0] == (b"moov", b"trak", b"uuid")          # in the video trak, nowhere else
    _, s, e = found[0]
    assert b[s:s + 16] == bytes.fromhex("ffcc8263f8554a938814587a02521fdd") == mp4.SPHERICAL_UUID
    import xml.etree.ElementTree as ET
    root = ET.fromstring(b[s + 16:e].decode("utf-8"))
    ns = "{http://ns.google.com/videos/1.0/spherical/}"
    assert root.tag == "{http://www.w3.org/1999/02/22-rdf-syntax-ns#}SphericalVideo"
    assert (root.findtext(ns + "Spherical"), root.findtext(ns + "Stitched"), root.findtext(ns + "ProjectionType")) == ("true", "true", "equirectangular")
    assert len(b) - len(a) == 8 + (e - s)
    # the samples are where the table says, in both files, and are the frame files
    for path in (plain, sph):
        info = mp4.read_samples(path)
        buf = open(path, "rb").read()
        assert [buf[o:o + n] for o, n in info["samples"]] == [open(p, "rb").read() for p in paths]
    # Motion-JPEG likewise (the writer checks the magic only)
    jpgs = []
    for k in range(2):
        p = tmp_path / f"frame_{k:04d}.jpg"
        p.write_bytes(mp4.JPEG_MAGIC + bytes([0xE0]) + bytes(20 + k))
        jpgs.append(str(p))
    mp4.write_jpeg_mp4(jpgs, 24, str(tmp_path / "j.mp4"), 16, 8)
    mp4.write_jpeg_mp4(jpgs, 24, str(tmp_path / "js.mp4"), 16, 8, spherical=True)
    j, js = open(tmp_path / "j.mp4", "rb").read(), open(tmp_path / "js.mp4", "rb").read()
    assert not [x for x in _boxes(j, 0, len(j)) if x[0][-1] == b"uuid"]
    assert [x[0] for x in _boxes(js, 0, len(js)) if x[0][-1] == b"uuid"] == [(b"moov", b"trak", b"uuid")]


def test_other_videos_are_byte_for_byte_what_they_were(tmp_path, monkeypatch):
    """assemble_video without the argument, and with spherical=False, writes the bytes of a mux of the same frames without it."""
    import builtins
    import shutil
    paths = _frames(tmp_path, 16, 8)
    want = str(tmp_path / "want.mp4")
    mp4.write_png_mp4(paths, 30, want, 16, 8)
    real_import = builtins.__import__

    def no_encoders(name, *a, **kw):                              # the last-resort route: no imageio + pyav, no ffmpeg
        if name.split(".")[0] in ("imageio", "av"):
            raise ImportError(name)
        return real_import(name, *a, **kw)
    monkeypatch.setattr(builtins, "__import__", no_encoders)
    monkeypatch.setattr(shutil, "which", lambda name: None)
    for kw, same in (({}, True), ({"spherical": False}, True), ({"spherical": True}, False)):
        out = str(tmp_path / "out.mp4")
        assert drivers.assemble_video(str(tmp_path), len(paths), 30, out, **kw)
        assert (open(out, "rb").read() == open(want, "rb").read()) == same
    sph = open(str(tmp_path / "out.mp4"), "rb").read()
    assert [x[0] for x in _boxes(sph, 0, len(sph)) if x[0][-1] == b"uuid"] == [(b"moov", b"trak", b"uuid")]
