"""render_video(video_codec="mjpeg"): JPEG frames coded on the device, muxed into a Motion-JPEG MP4; resume and sharding."""
import io
import json
import os

import numpy as np
import pytest

import jpeg_ref

W, H, N, Q = 320, 180, 24, 90


def _run(out, rank=0, world=1, resume=False, assemble=True, **kw):
    from bhr_amd import drivers
    r, _, _, _ = drivers.make_renderer(W, H, [6, 0, 0.5], 90, n_stars=50, tex_w=256, tex_h=128)
    before = r.outputs
    drivers.render_video(r, W, H, n_frames=N, fps=24, output_path=out, fov=90, static_cam_pos=[6, 0, 0.5], orbit=True,
                         resume=resume, disk_rotation_speed=0.1, orbit_degrees=90.0, rank=rank, world=world, assemble=assemble, **kw)
    after = r.outputs
    r.close()
    return drivers._frames_dir(out), before, after


def _jpgs(d):
    return [open(os.path.join(d, f"frame_{k:04d}.jpg"), "rb").read() for k in range(N)]


@pytest.mark.gpu
def test_mjpeg_video_frames_mux_resume_and_sharding(tmp_path):
    from PIL import Image
    from bhr_amd import mp4
    # the untouched default: PNG frames only, a 0x6D MP4 (no H.264 encoder in this environment), outputs left at "u8"
    out_png = str(tmp_path / "png" / "v.mp4")
    d_png, _, after = _run(out_png, video_stream="off")
    assert after == "u8"
    assert sorted(f for f in os.listdir(d_png) if f.startswith("frame_")) == [f"frame_{k:04d}.png" for k in range(N)]
    prog = json.load(open(os.path.join(d_png, "progress.json")))
    assert prog["params"] == {"n_frames": N, "fov": 90, "orbit": True, "disk_rotation_speed": 0.1, "orbit_degrees": 90.0}
    try:
        import imageio.v3  # noqa: F401
        import av  # noqa: F401
        have_h264 = True
    except ImportError:
        import shutil
        have_h264 = bool(shutil.which("ffmpeg"))
    if not have_h264:
        assert mp4.read_samples(out_png)["object_type"] == 0x6D

    out = str(tmp_path / "mjpeg" / "v.mp4")
    d, before, after = _run(out, video_codec="mjpeg", video_quality=Q)
    assert before == after == "f32"                                       # this mode restores the outputs selection
    assert sorted(f for f in os.listdir(d) if f.startswith("frame_")) == [f"frame_{k:04d}.jpg" for k in range(N)]
    assert not [f for f in os.listdir(d) if f.endswith((".tmp", ".png"))]
    frames = _jpgs(d)
    # the two loops render identical frames and differ only in the coder
    R = jpeg_ref.restart_interval(W)
    for k in range(N):
        u8 = np.asarray(Image.open(os.path.join(d_png, f"frame_{k:04d}.png")).convert("RGB"))
        assert frames[k] == jpeg_ref.encode(u8, Q, R), f"frame {k}"
    assert frames[0] != frames[N - 1]                                     # the camera moved
    info = mp4.read_samples(out)
    assert info["codec"] == "mp4v" and info["object_type"] == 0x6C and (info["width"], info["height"]) == (W, H)
    assert (info["timescale"], info["duration"]) == (24, N)
    video = open(out, "rb").read()
    for k, (o, s) in enumerate(info["samples"]):
        assert video[o:o + s] == frames[k]
        assert Image.open(io.BytesIO(video[o:o + s])).size == (W, H)
    prog = json.load(open(os.path.join(d, "progress.json")))
    assert sorted(prog["completed"]) == list(range(N))
    assert prog["params"] == {"n_frames": N, "fov": 90, "orbit": True, "disk_rotation_speed": 0.1, "orbit_degrees": 90.0,
                              "video_codec": "mjpeg", "video_quality": Q}
    print(f"[mjpeg] {W}x{H} x {N}: {sum(map(len, frames)) / N:.0f} B per JPEG frame, "
          f"{sum(os.path.getsize(os.path.join(d_png, f)) for f in os.listdir(d_png) if f.endswith('.png')) / N:.0f} B per PNG frame")

    # resume: two frames gone -> exactly those are rendered again, and the MP4 comes out the same
    for k in (7, 19):
        os.remove(os.path.join(d, f"frame_{k:04d}.jpg"))
    mtimes = {k: os.path.getmtime(os.path.join(d, f"frame_{k:04d}.jpg")) for k in range(N) if k not in (7, 19)}
    os.remove(out)
    _run(out, resume=True, video_codec="mjpeg", video_quality=Q)
    assert {k: os.path.getmtime(os.path.join(d, f"frame_{k:04d}.jpg")) for k in mtimes} == mtimes
    assert _jpgs(d) == frames and open(out, "rb").read() == video

    # another quality: the record's params differ, the run starts over
    _run(out, resume=True, video_codec="mjpeg", video_quality=75)
    again = _jpgs(d)
    assert all(a != b for a, b in zip(again, frames))                     # other tables in every header
    u8 = np.asarray(Image.open(os.path.join(d_png, "frame_0003.png")).convert("RGB"))
    assert again[3] == jpeg_ref.encode(u8, 75, R)
    assert json.load(open(os.path.join(d, "progress.json")))["params"]["video_quality"] == 75

    # two ranks, one after the other on the one device: the same files as one rank
    out2 = str(tmp_path / "two" / "v.mp4")
    d2, _, _ = _run(out2, rank=0, world=2, assemble=False, video_codec="mjpeg", video_quality=Q)
    _run(out2, rank=1, world=2, assemble=False, video_codec="mjpeg", video_quality=Q)
    assert sorted(f for f in os.listdir(d2) if f.startswith("frame_")) == [f"frame_{k:04d}.jpg" for k in range(N)]
    assert _jpgs(d2) == frames
    assert not os.path.exists(out2)                                       # rank 0 muxes after the barrier (cli.py)
