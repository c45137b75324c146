"""The HDR video stream on the device (bhr_y4m_open_hdr, csrc/hdr_stream.hip) against its NumPy restatement (tests/hdr_ref.py):
every plane of every frame within one code of the binary64 formulas, in at most 1 % of its samples (hdr_ref.Tally), the light
levels, the ring, two frame slots, the refusals, and render_video end to end."""
import ctypes as C
import json
import os
import stat

import numpy as np
import pytest

import hdr_ref as H
from hdr_cases import CONFIGS, SIZES, layer_sets
from test_gpu_grade import _assert_bits, _default, _inject
from test_gpu_quantisers import _renderer

pytestmark = pytest.mark.gpu
F32 = np.float32

# MaxCLL: the device's per-pixel value is white_nits * max over the rows of M . (h * gain), at most eight f32 roundings (the
# constants', the products', the sums') of 2^-24 each from the binary64 value: 1e-6 relative covers them twice over.  It is also
# the f32 restatement's value bit for bit, since that follows the kernel operation by operation and a maximum has no rounding.
CLL_RTOL = 1e-6
FALL_RTOL = 1e-6


def _check_frame(tally, planes, plane_hdr, cfg, tag):
    want = H.encode(plane_hdr, **cfg)
    tally.add(cfg["transfer"], planes, want, tag)
    y, cb, cr = planes
    assert 64 <= y.min() and y.max() <= 940 and 64 <= min(cb.min(), cr.min()) and max(cb.max(), cr.max()) <= 960, tag
    return want


# ---- 1. injected layers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
def test_injected_layers_stream_as_the_restatement(size, tmp_path, hip_lib):
    from bhr_amd.output import Y4MStream, read_y4m
    w, h = size
    r = _renderer(w, h)
    r.set_grade("clip", keep_hdr=True)
    sets = layer_sets(w, h)
    # the sets that saturate the light levels go last: the levels are running maxima, read after every frame
    sets = {k: sets[k] for k in sorted(sets, key=lambda k: (k in ("non-finite", "1e4", "65504"), k))}
    streams = [Y4MStream(r, str(tmp_path / f"s{k}.y4m"), fps=24, slots=2, hdr=cfg) for k, cfg in enumerate(CONFIGS)]
    planes_hdr, seen = [], []
    for name, layers in sets.items():
        _inject(r, layers)
        r.grade_frame()
        for st in streams:                                       # every configuration converts the same frame
            st.submit()
        planes_hdr.append(r.read_hdr())
        seen.append([(st.drain(), st.light_levels())[1] for st in streams])
    tally = H.Tally()
    for k, (st, cfg) in enumerate(zip(streams, CONFIGS)):
        frames, nbytes = st.drain()
        assert frames == len(sets) and nbytes == len(sets) * (6 + 3 * w * h)
        st.close()
        head, planes = read_y4m(str(tmp_path / f"s{k}.y4m"))
        assert (head["width"], head["height"], head["fps"], head["chroma"]) == (w, h, "24:1", "C420p10")
        assert "XCOLORRANGE=LIMITED" in head["tags"] and "Ip" in head["tags"] and "A1:1" in head["tags"] and len(planes) == len(sets)
        levels, levels32 = [], []
        for i, (name, got, plane) in enumerate(zip(sets, planes, planes_hdr)):
            want = _check_frame(tally, got, plane, cfg, f"{w}x{h} {name} {cfg}")
            levels.append((want["max_nits"], want["mean_nits"]))
            levels32.append(H.encode(plane, dtype=np.float32, **cfg)["max_nits"])
            cll, fall = seen[i][k]                               # the stream's levels once frame i was written
            want_cll, want_fall = H.light_levels(levels)
            if size == SIZES[-1]:
                print(f"[hdr] {w}x{h} {cfg} after {name!r}: MaxCLL {cll!r} (restatement {want_cll!r}), MaxFALL {fall!r} ({want_fall!r})")
            if cfg["transfer"] == "hlg":
                assert (cll, fall) == (0.0, 0.0)
                continue
            assert abs(cll - want_cll) <= CLL_RTOL * want_cll, (cfg, name, cll, want_cll)
            assert cll == max(levels32), (cfg, name, cll, max(levels32))
            assert abs(fall - want_fall) <= FALL_RTOL * want_fall, (cfg, name, fall, want_fall)
    print(f"[hdr] {w}x{h}: one code off in " + tally.check())
    r.close()


def test_the_cases_cover_what_the_issue_names():
    assert {c["transfer"] for c in CONFIGS} == {"pq", "hlg"} and {c["exposure"] for c in CONFIGS} == {-2.0, 0.0, 1.5}
    assert {c["white_nits"] for c in CONFIGS if c["transfer"] == "pq"} == {100.0, 203.0, 1000.0}
    assert SIZES == [(2, 2), (6, 4), (66, 18), (130, 34)]
    assert {"zeros", "toe ramp", "noise", "1e4", "65504", "non-finite"} <= set(layer_sets(6, 4))


# ---- 2. ring order -----------------------------------------------------------------------------------------------------------
def test_five_frames_leave_a_two_slot_ring_in_submission_order(tmp_path, hip_lib):
    from bhr_amd.output import Y4MStream, read_y4m
    w, h = 66, 18
    r = _renderer(w, h)
    r.set_grade("reinhard", exposure=0.5, keep_hdr=True)          # the SDR grade does not reach the stream
    cfg = dict(transfer="pq", exposure=0.0, white_nits=203.0)
    rng = np.random.default_rng(77)
    zero = np.zeros((h, w, 3), F32)
    frames = [(rng.random((h, w, 3), dtype=F32) * F32(0.4 * (k + 1)), zero, zero) for k in range(5)]
    path = str(tmp_path / "ring.y4m")
    planes_hdr = []
    with Y4MStream(r, path, fps=30, slots=2, hdr=cfg) as st:       # fewer slots than frames: submit has to wait
        for layers in frames:
            _inject(r, layers)
            r.grade_frame()
            st.submit()
        assert st.drain() == (5, 5 * (6 + 3 * w * h))
        cll, fall = st.light_levels()
    _, planes = read_y4m(path)
    assert len(planes) == 5
    tally = H.Tally()
    wants = [_check_frame(tally, got, layers[0], cfg, f"ring frame {k}") for k, (got, layers) in enumerate(zip(planes, frames))]
    tally.check()
    means = [float(p[0].mean()) for p in planes]
    assert means == sorted(means) and means[0] < means[-1] - 50    # the frames differ, and frame k is the k-th brightest
    assert abs(fall - max(x["mean_nits"] for x in wants)) <= FALL_RTOL * fall and abs(cll - max(x["max_nits"] for x in wants)) <= CLL_RTOL * cll
    r.close()


# ---- 3. two frame slots --------------------------------------------------------------------------------------------------------
def test_a_stream_over_two_frame_slots_gives_each_frame_its_own_plane(tmp_path, hip_lib):
    from bhr_amd.output import Y4MStream, read_y4m
    positions = [[6.0 + 0.3 * i, 0.2 * i, 0.5] for i in range(4)]
    g = dict(tonemap="reinhard", white=1.5, keep_hdr=True)
    one, s = _default("strict", frame_slots=1)
    one.set_grade(**g)
    want = []
    for pos in positions:
        one.render_async(pos, s["fov"])
        want.append(one.read_hdr())
    one.close()
    assert (want[0] != want[1]).any()
    print(f"[hdr] two slots: the planes reach {max(float(a.max()) for a in want):.3f}")
    two, _ = _default("strict", frame_slots=2)
    assert two.frame_slots == 2
    two.set_grade(**g)
    cfg = dict(transfer="hlg", exposure=0.0, white_nits=203.0)
    path = str(tmp_path / "two.y4m")
    with Y4MStream(two, path, fps=24, slots=3, hdr=cfg) as st:
        for pos in positions:                                    # nothing is read back: frame i is in flight when i + 1 is launched
            two.render_async(pos, s["fov"])
            st.submit()
        assert st.drain()[0] == 4
    _assert_bits(two.read_hdr(), want[-1], "the last frame's plane")
    _, planes = read_y4m(path)
    tally = H.Tally()
    for k, (got, plane) in enumerate(zip(planes, want)):
        _check_frame(tally, got, plane, cfg, f"two slots, frame {k}")
    tally.check()
    two.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
BAD_CONFIGS = [(0, 0.0, 203.0, 0), (3, 0.0, 203.0, 0), (-1, 0.0, 203.0, 0), (1, np.nan, 203.0, 0), (1, np.inf, 203.0, 0),
               (2, -np.inf, 203.0, 0), (1, 16.5, 203.0, 0), (2, -16.5, 203.0, 0), (1, 0.0, 0.0, 0), (1, 0.0, -1.0, 0),
               (1, 0.0, np.nan, 0), (1, 0.0, np.inf, 0), (1, 0.0, 10000.5, 0), (1, 0.0, 203.0, 1), (2, 0.0, 203.0, -1)]


def test_refusals_and_an_eight_bit_stream_afterwards(tmp_path, hip_lib):
    from bhr_amd import _lib
    from bhr_amd.output import Y4MStream, read_y4m, rgb_to_yuv420
    r, s = _default("strict")
    cfg = dict(transfer="pq", exposure=0.0, white_nits=203.0)
    path = str(tmp_path / "r.y4m")
    st = Y4MStream(r, path, fps=24, slots=2, hdr=cfg)
    r.render_async(s["cam_pos"], s["fov"])                        # no grade: the frame has no HDR plane
    with pytest.raises(AssertionError, match="HDR plane"):
        st.submit()
    assert hip_lib.bhr_y4m_submit(st._s) == _lib.BHR_ERR_STATE
    r.set_grade("aces", transfer="srgb")
    r.render_async(s["cam_pos"], s["fov"])                        # graded without keep_hdr
    assert hip_lib.bhr_y4m_submit(st._s) == _lib.BHR_ERR_STATE
    r.set_grade("aces", transfer="srgb", keep_hdr=True)
    r.render_async(s["cam_pos"], s["fov"])
    st.submit()                                                   # the stream is as good as new
    plane = r.read_hdr()
    assert st.drain() == (1, 6 + 3 * 64 * 36)
    st.close()
    tally = H.Tally()
    _check_frame(tally, read_y4m(path)[1][0], plane, cfg, "after the refusals")
    tally.check()
    # every configuration bhr_y4m_open_hdr refuses, with nothing opened and no file made
    out = C.c_void_p()
    for k, (transfer, stops, white, reserved) in enumerate(BAD_CONFIGS):
        bad = _lib.HdrStream(transfer, stops, white, reserved)
        p = tmp_path / f"bad{k}.y4m"
        assert hip_lib.bhr_y4m_open_hdr(r._ctx, os.fsencode(str(p)), 24, 1, 2, C.byref(bad), C.byref(out)) == _lib.BHR_ERR_INVALID, BAD_CONFIGS[k]
        assert b"bhr_y4m_open_hdr" in hip_lib.bhr_last_error() and not out.value and not p.exists()
    assert hip_lib.bhr_y4m_open_hdr(r._ctx, os.fsencode(str(tmp_path / "n.y4m")), 24, 1, 2, None, C.byref(out)) == _lib.BHR_ERR_INVALID
    for bad in (dict(transfer="srgb"), dict(transfer="pq", white_nits=0.0), dict(transfer="hlg", exposure=17.0)):
        with pytest.raises(ValueError):
            Y4MStream(r, str(tmp_path / "v.y4m"), fps=24, hdr=bad)
    hlg = Y4MStream(r, str(tmp_path / "h.y4m"), fps=24, slots=1, hdr=dict(transfer="hlg", white_nits=-3.0))     # HLG has no white level
    hlg.close()
    for w, h in ((7, 4), (6, 5)):
        odd = _renderer(w, h)
        with pytest.raises(ValueError, match="even"):
            Y4MStream(odd, str(tmp_path / "odd.y4m"), fps=24, hdr=cfg)
        odd.close()
    # an 8-bit stream on the same context: what it always was
    r.set_grade(None)
    r.render_async(s["cam_pos"], s["fov"])
    u8 = r.read_final_u8()
    path8 = str(tmp_path / "sdr.y4m")
    with Y4MStream(r, path8, fps=24, slots=2) as st8:
        st8.submit()
        assert st8.drain() == (1, 6 + 64 * 36 * 3 // 2)
        assert st8.light_levels() == (0.0, 0.0)
    head, planes = read_y4m(path8)
    assert head["chroma"] == "C420jpeg" and planes[0][0].dtype == np.uint8
    for got, want in zip(planes[0], rgb_to_yuv420(u8)):
        np.testing.assert_array_equal(got, want)
    r.close()


# ---- 5. render_video end to end -------------------------------------------------------------------------------------------------
def _video(tmp_path, name, monkeypatch=None, capture=None, **kw):
    """One 64x36 video of 3 frames into tmp_path/name; capture: a list that receives every submitted frame's HDR plane and, last,
    the stream's light levels."""
    from bhr_amd import drivers, output
    if capture is not None:
        class Spy(output.Y4MStream):
            def submit(self):
                super().submit()
                capture.append(self._renderer.read_hdr())

            def light_levels(self):
                capture.append(super().light_levels())
                return capture[-1]
        monkeypatch.setattr(drivers, "Y4MStream", Spy)
    out = str(tmp_path / name / "v.mp4")
    r, _, _, _ = drivers.make_renderer(64, 36, [6, 0, 0.5], 90, n_stars=50, tex_w=256, tex_h=128, lens_flare=kw.pop("lens_flare", False),
                                       math="strict")
    before = r.grade
    drivers.render_video(r, 64, 36, n_frames=3, fps=12, output_path=out, fov=90, static_cam_pos=[6, 0, 0.5], assemble=kw.pop("assemble", False),
                         **kw)
    assert r.grade == before                                      # the renderer's grade is restored on return
    r.close()
    d = drivers._frames_dir(out)
    return out, [open(os.path.join(d, f"frame_{k:04d}.png"), "rb").read() for k in range(3)], json.load(open(os.path.join(d, "progress.json")))


@pytest.mark.parametrize("how", ["marched, lens flare", "ray map"])
def test_render_video_writes_the_hdr_stream_beside_unchanged_frames(how, tmp_path, monkeypatch, hip_lib):
    from bhr_amd.output import read_y4m
    kw = dict(lens_flare=True) if how.startswith("marched") else dict(ray_map=True)
    captured = []
    out, pngs, record = _video(tmp_path, "hdr", monkeypatch, captured, video_hdr="pq", video_stream="y4m", **kw)
    monkeypatch.undo()
    _, plain, plain_record = _video(tmp_path, "plain", video_stream="off", **kw)
    assert pngs == plain and len(set(pngs)) == 3                  # the frame files are what they are without the stream
    assert record["params"] == dict(plain_record["params"], video_hdr="pq", hdr_white=203.0, hdr_exposure=0.0)
    assert "video_hdr" not in plain_record["params"] and "tonemap" not in record["params"]
    planes_hdr, levels = captured[:3], captured[3]
    assert len(captured) == 4 and all(p.shape == (36, 64, 3) for p in planes_hdr)
    print(f"[hdr] render_video, {how}: the planes reach {max(float(p.max()) for p in planes_hdr):.3f}")
    cfg = dict(transfer="pq", exposure=0.0, white_nits=203.0)
    head, planes = read_y4m(os.path.splitext(out)[0] + ".y4m")
    assert (head["width"], head["height"], head["fps"], head["chroma"]) == (64, 36, "12:1", "C420p10") and len(planes) == 3
    tally = H.Tally()
    wants = [_check_frame(tally, got, plane, cfg, f"{how}, frame {k}") for k, (got, plane) in enumerate(zip(planes, planes_hdr))]
    print(f"[hdr] render_video, {how}: one code off in " + tally.check())
    side = json.load(open(os.path.splitext(out)[0] + ".hdr10.json"))
    assert side == {"transfer": "pq", "white_nits": 203.0, "exposure": 0.0, "primaries": "bt2020", "matrix": "bt2020nc", "range": "limited",
                    "max_cll": levels[0], "max_fall": levels[1], "frames": 3}
    want_cll, want_fall = H.light_levels((x["max_nits"], x["mean_nits"]) for x in wants)
    assert abs(side["max_cll"] - want_cll) <= CLL_RTOL * want_cll and abs(side["max_fall"] - want_fall) <= FALL_RTOL * want_fall


# ---- 6. the pipe into ffmpeg ------------------------------------------------------------------------------------------------------
def test_render_video_pipes_the_hdr_stream_into_ffmpeg(tmp_path, monkeypatch, hip_lib):
    """video_stream="auto" with an `ffmpeg` on PATH: a stand-in that stores its arguments and its standard input plays the encoder
    (what is under test is the argument list and the pipe, not libx265).  It gets hdr_ffmpeg_args and the bytes of the .y4m file."""
    from bhr_amd import drivers
    file_out, _, _ = _video(tmp_path, "file", video_hdr="hlg", hdr_exposure=1.0, video_stream="y4m")
    want = open(os.path.splitext(file_out)[0] + ".y4m", "rb").read()
    fake = tmp_path / "bin" / "ffmpeg"
    fake.parent.mkdir()
    fake.write_text('#!/bin/sh\nprintf "%s\\n" "$@" > "$0.args"\nfor a in "$@"; do out="$a"; done\ncat > "$out"\n')
    fake.chmod(fake.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", str(fake.parent) + os.pathsep + os.environ["PATH"])
    out, _, _ = _video(tmp_path, "pipe", video_hdr="hlg", hdr_exposure=1.0, video_stream="auto", assemble=True)
    assert open(str(fake) + ".args").read().split("\n")[:-1] == drivers.hdr_ffmpeg_args("hlg", out)[1:]
    got = open(out, "rb").read()
    assert got.startswith(b"YUV4MPEG2 W64 H36 F12:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n") and got == want
    assert not os.path.exists(os.path.splitext(out)[0] + ".y4m")
    side = json.load(open(os.path.splitext(out)[0] + ".hdr10.json"))
    assert (side["transfer"], side["exposure"], side["max_cll"], side["max_fall"], side["frames"]) == ("hlg", 1.0, 0.0, 0.0, 3)
