"""render_video under a projection: the frame files of --video --orbit --projection equirect --observer circular are the frames
of the same cameras and velocities rendered one at a time, the Motion-JPEG file of a full-sphere equirect video carries the
spherical box, a fisheye video's does not, and a resume under another projection starts over."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, N, POV = 64, 32, 3, [6, 0, 0.5]


def _renderer(frame_slots, w=W, h=H):
    from bhr_amd import drivers
    r, _, _, _ = drivers.make_renderer(w, h, POV, 90, n_stars=600, tex_w=512, tex_h=256, frame_slots=frame_slots, math="strict")
    return r


def _alone(plan, **proj):
    from bhr_amd import drivers
    r = _renderer(1)
    try:
        factories = drivers.init_lifecycle_system(r, r.dtex_h, r.dtex_w, seed=42)
        frames = []
        for f, (pos, beta) in enumerate(plan):
            drivers.advance_lifecycle_frame(r, factories, f * 0.1, 0.1, recompute_stats=(f % 60 == 0), compose=True)
            r.render(pos, 90, frame=0, observer=beta, **proj)
            frames.append(r.read_final_u8())
        return frames
    finally:
        r.close()


def _uuid_boxes(path):
    from bhr_amd import mp4
    buf = open(path, "rb").read()
    info = mp4.read_samples(path)
    moov = next((a, b) for k, a, b in mp4._walk(buf, 0, len(buf)) if k == b"moov")
    trak = next((a, b) for k, a, b in mp4._walk(buf, *moov) if k == b"trak")
    return [buf[a:b] for k, a, b in mp4._walk(buf, *trak) if k == b"uuid"], info


def test_video_frames_are_the_frames_rendered_alone(tmp_path, hip_lib):
    from PIL import Image
    from bhr_amd import drivers, observer
    out = os.path.join(str(tmp_path), "eq", "v.mp4")
    proj = dict(projection="equirect", projection_fov=(360.0, 180.0))
    r = _renderer(2)
    try:
        drivers.render_video(r, W, H, n_frames=N, fps=12, output_path=out, fov=90, static_cam_pos=POV, assemble=False, video_stream="off",
                             observer="circular", orbit=True, **proj)
    finally:
        r.close()
    with open(os.path.join(drivers._frames_dir(out), "progress.json")) as f:
        assert json.load(f)["params"]["projection"] == {"kind": "equirect", "fov": [360.0, 180.0]}
    plan = observer.frame_plan(N, POV, "circular", None, True, 360.0, None)
    want = _alone(plan, **proj)
    frames = [np.asarray(Image.open(os.path.join(drivers._frames_dir(out), f"frame_{f:04d}.png")).convert("RGB")) for f in range(N)]
    for f in range(N):
        assert frames[f].shape == (H, W, 3)
        assert np.array_equal(frames[f], want[f]), f"frame {f}: {int((frames[f] != want[f]).any(axis=2).sum())} pixels differ"
    assert frames[0].max() > 100 and (frames[0] != frames[-1]).mean() > 0.01       # the frames are real and the camera moves
    pinhole = _alone(plan)                                                         # the projection is in the files
    assert (pinhole[0] != want[0]).mean() > 0.1


def test_mjpeg_video_carries_the_spherical_box_for_the_full_sphere_only(tmp_path, hip_lib):
    from bhr_amd import drivers, mp4
    found = {}
    for name, size, proj in (("equirect", (64, 32), dict(projection="equirect")), ("partial", (64, 32), dict(projection="equirect", projection_fov=(180.0, 90.0))),
                             ("fisheye", (32, 32), dict(projection="fisheye")), ("pinhole", (64, 32), {})):
        out = os.path.join(str(tmp_path), name, "v.mp4")
        r = _renderer(2, *size)
        try:
            drivers.render_video(r, *size, n_frames=2, fps=12, output_path=out, fov=90, static_cam_pos=POV, video_codec="mjpeg", video_stream="off", **proj)
        finally:
            r.close()
        boxes, info = _uuid_boxes(out)
        assert (info["width"], info["height"]) == size and len(info["samples"]) == 2 and info["object_type"] == mp4.JPEG_OBJECT_TYPE
        found[name] = boxes
    assert found["partial"] == found["fisheye"] == found["pinhole"] == []
    assert found["equirect"] == [mp4.SPHERICAL_UUID + mp4.SPHERICAL_XML]


def test_resume_under_another_projection_starts_over(tmp_path, hip_lib, capsys):
    from bhr_amd import drivers
    out = os.path.join(str(tmp_path), "v.mp4")
    r = _renderer(2)
    try:
        kw = dict(n_frames=2, fps=12, output_path=out, fov=90, static_cam_pos=POV, assemble=False, video_stream="off")
        drivers.render_video(r, W, H, projection="equirect", **kw)
        capsys.readouterr()
        drivers.render_video(r, W, H, projection="equirect", resume=True, **kw)
        assert "Resuming: 2/2" in capsys.readouterr().out
        drivers.render_video(r, W, H, projection="fisheye", resume=True, **kw)
        assert "starting over" in capsys.readouterr().out
        drivers.render_video(r, W, H, resume=True, **kw)                          # ... and so does the pinhole camera
        assert "starting over" in capsys.readouterr().out
    finally:
        r.close()
