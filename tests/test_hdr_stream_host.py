"""The host side of the HDR video stream (--video_hdr, render_video(video_hdr=...), output.Y4MStream(hdr=...)): command-line
parsing and every refusal, the encoder's argument list, the reader of 10-bit YUV4MPEG2 files, the progress record, the sidecar
and the two new entry points in the binding.  No device is touched."""
import contextlib
import io
import json
import os

import numpy as np
import pytest


# ---- command line ----------------------------------------------------------------------------------------------------------
def test_cli_accepts_video_hdr():
    from bhr_amd import cli
    a = cli.parse_args(["--video", "--video_hdr", "pq"])
    assert (a.video_hdr, a.hdr_white, a.hdr_exposure) == ("pq", 203.0, 0.0)
    cli.validate_args(a)
    a = cli.parse_args(["--video", "--video_hdr", "pq", "--hdr_white", "1000", "--hdr_exposure", "-1.5", "--lens_flare"])
    assert (a.video_hdr, a.hdr_white, a.hdr_exposure) == ("pq", 1000.0, -1.5)
    cli.validate_args(a)
    a = cli.parse_args(["--video", "--video_hdr", "hlg", "--hdr_exposure", "2", "--video_stream", "y4m"])
    assert (a.video_hdr, a.hdr_exposure) == ("hlg", 2.0)
    cli.validate_args(a)
    # beside a grade of the SDR frames, and with every frame producer of the loop
    for extra in (["--tonemap", "aces", "--transfer", "srgb", "--exposure", "1"], ["--shutter", "0.5"], ["--ray_map"],
                  ["--orbit", "--orbit_map"], ["--shutter", "0.5", "--shutter_map"], ["--bit_depth", "16"], ["--dither", "blue"]):
        a = cli.parse_args(["--video", "--video_hdr", "pq"] + extra)
        cli.validate_args(a)
        assert a.video_hdr == "pq"
    assert cli.parse_args([]).video_hdr is None and cli.parse_args(["--video"]).video_hdr is None       # off by default


@pytest.mark.parametrize("argv,word", [
    (["--video_hdr", "pq"], "--video_hdr needs --video"),
    (["--video", "--video_hdr", "hlg", "--hdr_white", "203"], "--hdr_white"),
    (["--video", "--hdr_white", "203"], "--hdr_white needs --video_hdr"),
    (["--video", "--hdr_exposure", "1"], "--hdr_exposure needs --video_hdr"),
    (["--hdr_white", "100"], "--hdr_white needs --video_hdr"),
    (["--video", "--video_hdr", "pq", "--video_codec", "mjpeg"], "mjpeg"),
    (["--video", "--video_hdr", "pq", "--video_stream", "off"], "--video_stream off"),
    (["--video", "--video_hdr", "srgb"], "--video_hdr"),
    (["--video", "--video_hdr", "pq", "--hdr_white", "bright"], "--hdr_white"),
])
def test_cli_refuses_in_argument_parsing(argv, word, capsys):
    from bhr_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


@pytest.mark.parametrize("spelling", [["--transfer", "pq"], ["--transfer", "hlg"], ["--tonemap", "pq"]])
def test_the_grade_still_refuses_an_hdr_transfer(spelling):
    """The HDR stream is a consumer of the HDR plane beside the grade, not a transfer inside it."""
    from bhr_amd import cli
    from bhr_amd.renderer import check_grade
    with contextlib.redirect_stderr(io.StringIO()), pytest.raises(SystemExit):
        cli.parse_args(["--video"] + spelling)
    with pytest.raises(ValueError):
        check_grade(dict(tonemap="clip", transfer="pq"))


@pytest.mark.parametrize("argv,word", [
    (["--video", "--video_hdr", "pq", "--hdr_white", "0"], "hdr_white"),
    (["--video", "--video_hdr", "pq", "--hdr_white", "10001"], "hdr_white"),
    (["--video", "--video_hdr", "pq", "--hdr_white", "nan"], "hdr_white"),
    (["--video", "--video_hdr", "pq", "--hdr_white", "inf"], "hdr_white"),
    (["--video", "--video_hdr", "pq", "--hdr_exposure", "16.5"], "hdr_exposure"),
    (["--video", "--video_hdr", "hlg", "--hdr_exposure", "-17"], "hdr_exposure"),
    (["--video", "--video_hdr", "hlg", "--hdr_exposure", "nan"], "hdr_exposure"),
    (["--video", "--video_hdr", "pq", "--gpus", "2"], "--gpus"),
])
def test_cli_refuses_values_in_validation(argv, word):
    from bhr_amd import cli
    with pytest.raises(ValueError, match=word):
        cli.validate_args(cli.parse_args(argv))


def test_help_says_what_the_hdr_stream_is():
    from bhr_amd import cli
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        cli.parse_args(["--help"])
    text = " ".join(buf.getvalue().split())
    for word in ("--video_hdr", "--hdr_white", "--hdr_exposure", "BT.2020", "hdr10.json"):
        assert word in text


# ---- the driver's checks -----------------------------------------------------------------------------------------------------
def test_check_video_hdr_accepts_and_refuses():
    from bhr_amd import drivers
    assert drivers.check_video_hdr(None, hdr_white=-1, hdr_exposure=99, width=3, height=3, world=4, video_codec="mjpeg",
                                   video_stream="off") is None                      # off: nothing to check
    assert drivers.check_video_hdr("pq") == dict(transfer="pq", exposure=0.0, white_nits=203.0)
    assert drivers.check_video_hdr("hlg", 203.0, 1.5, 64, 36) == dict(transfer="hlg", exposure=1.5, white_nits=203.0)
    assert drivers.check_video_hdr("pq", 1000, -2, 1920, 1080, 1, "auto", "y4m") == dict(transfer="pq", exposure=-2.0, white_nits=1000.0)
    assert drivers.check_video_hdr("hlg", hdr_white=-5.0)["transfer"] == "hlg"      # HLG has no white level to check
    for kw in (dict(video_hdr="srgb"), dict(video_hdr="PQ"), dict(video_hdr=True), dict(hdr_white=0.0), dict(hdr_white=-1.0),
               dict(hdr_white=10000.5), dict(hdr_white=float("nan")), dict(hdr_white=float("inf")), dict(hdr_white="203"),
               dict(hdr_exposure=16.01), dict(hdr_exposure=-16.01), dict(hdr_exposure=float("nan")), dict(hdr_exposure=None),
               dict(world=2), dict(video_codec="mjpeg"), dict(video_stream="off"), dict(width=65), dict(height=35)):
        with pytest.raises(ValueError):
            drivers.check_video_hdr(**dict(dict(video_hdr="pq"), **kw))


def test_check_hdr_of_the_stream():
    from bhr_amd.output import check_hdr
    assert check_hdr(None) is None
    assert check_hdr(dict(transfer="pq")) == dict(transfer="pq", exposure=0.0, white_nits=203.0)
    assert check_hdr(dict(transfer="hlg", exposure=-16, white_nits=7)) == dict(transfer="hlg", exposure=-16.0, white_nits=7.0)
    for bad in ("pq", dict(), dict(transfer="linear"), dict(transfer="pq", white=203.0), dict(transfer="pq", exposure=17),
                dict(transfer="pq", white_nits=0), dict(transfer="pq", white_nits=20000.0), dict(transfer="pq", exposure=False)):
        with pytest.raises(ValueError):
            check_hdr(bad)


class NoDevice:                                               # anything but the settings the checks read is device work
    supersample = 1
    disk_tilt = 0.0
    _dv2 = None

    def __getattr__(self, name):
        raise RuntimeError(f"device work: {name}")


def test_render_video_refuses_before_touching_the_renderer(tmp_path):
    from bhr_amd import drivers
    args = (48, 28, 6, 24, "never/v.mp4", 90, [6, 0, 0.5])
    for kw, word in ((dict(world=2), "ranks"), (dict(video_codec="mjpeg"), "mjpeg"), (dict(video_stream="off"), "--video_stream off"),
                     (dict(video_hdr="rec709"), "video_hdr"), (dict(hdr_white=0.0), "white_nits"), (dict(hdr_exposure=20.0), "exposure")):
        with pytest.raises(ValueError) as e:
            drivers.render_video(NoDevice(), *args, **dict(dict(video_hdr="pq"), **kw))
        assert word in str(e.value), (kw, str(e.value))
    for w, h in ((49, 28), (48, 27)):
        with pytest.raises(ValueError, match="even frame sizes"):
            drivers.render_video(NoDevice(), w, h, 6, 24, "never/v.mp4", 90, [6, 0, 0.5], video_hdr="hlg")
    assert not os.path.exists("never")
    # a resume that finds completed frames: refused; one that finds none goes on to the renderer
    out = str(tmp_path / "v.mp4")
    d = drivers._frames_dir(out)
    os.makedirs(d)
    params = drivers.progress_params(6, 90, False, 0.1, 360.0, video_hdr="pq", hdr_white=203.0, hdr_exposure=0.0)
    with open(os.path.join(d, "progress.json"), "w") as f:
        json.dump({"params": params, "completed": [0, 1]}, f)
    for k in (0, 1):
        open(os.path.join(d, f"frame_{k:04d}.png"), "wb").close()
    with pytest.raises(ValueError, match="does not resume"):
        drivers.render_video(NoDevice(), 48, 28, 6, 24, out, 90, [6, 0, 0.5], resume=True, video_hdr="pq")
    with pytest.raises(RuntimeError, match="device work"):
        drivers.render_video(NoDevice(), 48, 28, 6, 24, str(tmp_path / "w.mp4"), 90, [6, 0, 0.5], resume=True, video_hdr="pq")
    with pytest.raises(RuntimeError, match="device work"):        # and without resume the good call reaches the renderer
        drivers.render_video(NoDevice(), 48, 28, 6, 24, str(tmp_path / "x.mp4"), 90, [6, 0, 0.5], video_hdr="hlg", video_stream="y4m")


# ---- the encoder's arguments, the sidecar, the progress record ----------------------------------------------------------------
def test_ffmpeg_arguments():
    from bhr_amd.drivers import hdr_ffmpeg_args
    for transfer, trc in (("pq", "smpte2084"), ("hlg", "arib-std-b67")):
        a = hdr_ffmpeg_args(transfer, "out/v.mp4")
        assert a[0] == "ffmpeg" and a[-1] == "out/v.mp4"
        text = " ".join(a)
        assert (f"-f yuv4mpegpipe -i - -c:v libx265 -pix_fmt yuv420p10le -color_primaries bt2020 -color_trc {trc} "
                "-colorspace bt2020nc -color_range tv") in text
        assert a.index("-i") < a.index("-c:v") and "libx264" not in a          # input options first, output options behind the input
    with pytest.raises(ValueError):
        hdr_ffmpeg_args("srgb", "v.mp4")


def test_sidecar_record():
    from bhr_amd.drivers import hdr_sidecar
    rec = hdr_sidecar(dict(transfer="pq", exposure=0.5, white_nits=203.0), 1234.5, 87.25, 3)
    assert rec == {"transfer": "pq", "white_nits": 203.0, "exposure": 0.5, "primaries": "bt2020", "matrix": "bt2020nc",
                   "range": "limited", "max_cll": 1234.5, "max_fall": 87.25, "frames": 3}
    assert json.loads(json.dumps(rec)) == rec


def test_progress_params_carry_the_hdr_settings_only_when_set():
    from bhr_amd.drivers import progress_params
    base = progress_params(6, 90, True, 0.1, 360.0)
    assert set(base) == {"n_frames", "fov", "orbit", "disk_rotation_speed", "orbit_degrees"}
    assert progress_params(6, 90, True, 0.1, 360.0, video_hdr=None, hdr_white=1000.0, hdr_exposure=2.0) == base
    assert progress_params(6, 90, True, 0.1, 360.0, video_hdr="pq") == dict(base, video_hdr="pq", hdr_white=203.0, hdr_exposure=0.0)
    assert progress_params(6, 90, True, 0.1, 360.0, video_hdr="hlg", hdr_white=203.0, hdr_exposure=-1.0) == \
        dict(base, video_hdr="hlg", hdr_white=203.0, hdr_exposure=-1.0)
    # the stream's own grade (clip, keep_hdr) is not the caller's: the record of an ungraded HDR run carries no grade
    assert "tonemap" not in progress_params(6, 90, True, 0.1, 360.0, video_hdr="pq")
    graded = progress_params(6, 90, True, 0.1, 360.0, grade=dict(tonemap="aces", exposure=1.0, white=2.5, transfer="srgb"), video_hdr="pq")
    assert graded["tonemap"] == "aces" and graded["video_hdr"] == "pq"


# ---- read_y4m ----------------------------------------------------------------------------------------------------------------
def test_read_y4m_reads_ten_bit_and_eight_bit_files(tmp_path):
    from bhr_amd.output import read_y4m
    rng = np.random.default_rng(5)
    w, h = 6, 4
    frames10 = [(rng.integers(64, 941, (h, w)).astype("<u2"), rng.integers(64, 961, (h // 2, w // 2)).astype("<u2"),
                 rng.integers(64, 961, (h // 2, w // 2)).astype("<u2")) for _ in range(3)]
    p10 = tmp_path / "hdr.y4m"
    with open(p10, "wb") as f:
        f.write(b"YUV4MPEG2 W6 H4 F24:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n")
        for planes in frames10:
            f.write(b"FRAME\n" + b"".join(p.tobytes() for p in planes))
    head, planes = read_y4m(str(p10))
    assert (head["width"], head["height"], head["fps"], head["chroma"]) == (6, 4, "24:1", "C420p10")
    assert "XCOLORRANGE=LIMITED" in head["tags"] and len(planes) == 3
    for got, want in zip(planes, frames10):
        for g, x in zip(got, want):
            assert g.dtype == np.uint16 and g.shape == x.shape
            np.testing.assert_array_equal(g, x)
    # little endian in the file: 0x0340 is the bytes 40 03
    assert open(p10, "rb").read().split(b"FRAME\n")[1][:2] == int(frames10[0][0][0, 0]).to_bytes(2, "little")
    frames8 = [(rng.integers(16, 236, (h, w)).astype(np.uint8), rng.integers(16, 241, (h // 2, w // 2)).astype(np.uint8),
                rng.integers(16, 241, (h // 2, w // 2)).astype(np.uint8)) for _ in range(2)]
    p8 = tmp_path / "sdr.y4m"
    with open(p8, "wb") as f:
        f.write(b"YUV4MPEG2 W6 H4 F30:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n")
        for planes in frames8:
            f.write(b"FRAME\n" + b"".join(p.tobytes() for p in planes))
    head, planes = read_y4m(str(p8))
    assert (head["width"], head["height"], head["fps"], head["chroma"]) == (6, 4, "30:1", "C420jpeg") and len(planes) == 2
    for got, want in zip(planes, frames8):
        for g, x in zip(got, want):
            assert g.dtype == np.uint8
            np.testing.assert_array_equal(g, x)
    with open(p10, "ab") as f:
        f.write(b"FRAME\n" + b"\0" * 10)
    with pytest.raises(AssertionError, match="truncated"):
        read_y4m(str(p10))


# ---- the binding ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_entry_points(hip_lib):
    import ctypes as C
    from bhr_amd import _lib
    for name in ("bhr_y4m_open_hdr", "bhr_y4m_light_levels"):
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name)
    assert (_lib.HDR_PQ, _lib.HDR_HLG) == (1, 2) and C.sizeof(_lib.HdrStream) == 16
    assert [f[0] for f in _lib.HdrStream._fields_] == ["transfer", "exposure_stops", "white_nits", "reserved"]
    assert hip_lib.bhr_abi_version() == 1
    # argument checks that need no device
    s = C.c_void_p(1)
    assert hip_lib.bhr_y4m_open_hdr(None, b"x.y4m", 24, 1, 2, None, C.byref(s)) == _lib.BHR_ERR_INVALID and not s.value
    cfg = _lib.HdrStream(_lib.HDR_PQ, 0.0, 203.0, 0)
    assert hip_lib.bhr_y4m_open_hdr(None, b"x.y4m", 24, 1, 2, C.byref(cfg), C.byref(s)) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_y4m_light_levels(None, None) == _lib.BHR_ERR_INVALID
    assert b"bhr_y4m_light_levels" in hip_lib.bhr_last_error()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bhr_output.h")).read()
    text = " ".join(header.split())
    assert "#define BHR_HDR_PQ 1" in text and "#define BHR_HDR_HLG 2" in text
    assert "typedef struct { int32_t transfer; float exposure_stops; float white_nits; int32_t reserved; } bhr_hdr_stream;" in text
    assert "bhr_y4m_light_levels(bhr_y4m *stream, double out[2]);" in text
