"""render_video with a moving observer: the frame files of --video --orbit --observer circular and of --observer infall
--infall_to 2 are the frames of the same cameras and velocities rendered one at a time."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, N, FOV, POV = 64, 36, 4, 90, [6, 0, 0.5]


def _renderer(frame_slots):
    from bhr_amd import drivers
    r, _, _, _ = drivers.make_renderer(W, H, POV, FOV, n_stars=600, tex_w=512, tex_h=256, frame_slots=frame_slots, math="strict")
    return r


def _alone(plan):
    """The frames of the plan rendered one at a time: the video loop's scene updates, then render() of the frame's camera and
    velocity on a context that holds one frame, read back before the next."""
    from bhr_amd import drivers
    r = _renderer(1)
    try:
        factories = drivers.init_lifecycle_system(r, r.dtex_h, r.dtex_w, seed=42)
        frames = []
        for f, (pos, beta) in enumerate(plan):
            drivers.advance_lifecycle_frame(r, factories, f * 0.1, 0.1, recompute_stats=(f % 60 == 0), compose=True)
            r.render(pos, FOV, frame=0, observer=beta)
            frames.append(r.read_final_u8())
        return frames
    finally:
        r.close()


@pytest.mark.parametrize("mode", ("orbit_circular", "infall_to"))
def test_video_frames_are_the_frames_rendered_alone(mode, tmp_path, hip_lib):
    from PIL import Image
    from bhr_amd import drivers, observer
    kw = dict(observer="circular", orbit=True) if mode == "orbit_circular" else dict(observer="infall", infall_to=2.0)
    out = os.path.join(str(tmp_path), mode, "v.mp4")
    r = _renderer(2)
    try:
        drivers.render_video(r, W, H, n_frames=N, fps=12, output_path=out, fov=FOV, static_cam_pos=POV, assemble=False, video_stream="off", **kw)
    finally:
        r.close()
    plan = observer.frame_plan(N, POV, kw["observer"], None, kw.get("orbit", False), 360.0, kw.get("infall_to"))
    if mode == "infall_to":
        assert np.linalg.norm(plan[-1][0]) == pytest.approx(2.0) and plan[0][0] == pytest.approx(POV)
    want = _alone(plan)
    frames = [np.asarray(Image.open(os.path.join(drivers._frames_dir(out), f"frame_{f:04d}.png")).convert("RGB")) for f in range(N)]
    for f in range(N):
        assert frames[f].shape == (H, W, 3)
        assert np.array_equal(frames[f], want[f]), f"frame {f}: {int((frames[f] != want[f]).any(axis=2).sum())} pixels differ"
    assert frames[0].max() > 100 and (frames[0] != frames[-1]).mean() > 0.01       # the frames are real and the camera moves
    # the camera's motion is in the files: the same loop with a camera at rest writes other frames
    rest = _alone([(pos, (0.0, 0.0, 0.0)) for pos, _ in plan])
    assert (rest[-1] != want[-1]).mean() > 0.01
