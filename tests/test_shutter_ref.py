"""Motion blur, the host side (no GPU): the NumPy statement of a shutter frame's layers (tests/shutter_ref.py), the sample
times of drivers.shutter_times, the driver's and the CLI's refusals, and the progress record of a video without a shutter."""
import numpy as np
import pytest

from shutter_ref import resolve


def test_resolve_is_the_sequential_f32_sum_times_the_f32_reciprocal():
    rng = np.random.default_rng(5)
    layers = [rng.random((13, 21, 3), dtype=np.float32) for _ in range(5)]
    np.testing.assert_array_equal(resolve(layers[:1]), layers[0])
    got = resolve(layers)
    assert got.dtype == np.float32 and got.shape == (13, 21, 3)
    # element by element with Python-level f32 scalars
    inv = np.float32(1) / np.float32(5)
    for idx in [(0, 0, 0), (12, 20, 2), (6, 11, 1)]:
        acc = layers[0][idx]
        for l in layers[1:]:
            acc = np.float32(acc + l[idx])
        assert got[idx] == np.float32(acc * inv)
    # it is NOT the binary64 mean rounded once, nor a division: the order and the roundings are part of the definition
    third = np.float32(1) / np.float32(3)
    one = [np.full((1, 1, 3), v, dtype=np.float32) for v in (0.1, 0.2, 0.7)]
    assert resolve(one)[0, 0, 0] == np.float32(np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.7)) * third)
    with pytest.raises(ValueError):
        resolve([])
    with pytest.raises(ValueError):
        resolve([layers[0], layers[1].astype(np.float64)])


@pytest.mark.parametrize("frame", [0, 7, 3599])
@pytest.mark.parametrize("shutter", [0.25, 0.5, 1.0])
@pytest.mark.parametrize("n", [1, 2, 3, 8, 64])
def test_shutter_times(frame, shutter, n):
    from bhr_amd.drivers import shutter_times
    u = shutter_times(frame, shutter, n)
    assert len(u) == n and all(isinstance(v, float) for v in u)
    if n == 1:
        assert u == [float(frame)]                                   # the frame itself
    for j in range(n):                                               # symmetric about the frame
        assert abs((u[j] - frame) + (u[n - 1 - j] - frame)) <= 4 * np.spacing(float(max(frame, 1)))
    assert all(b > a for a, b in zip(u, u[1:]))                      # strictly increasing
    assert u[-1] - u[0] < shutter                                    # inside the exposure
    assert frame - shutter / 2 < u[0] and u[-1] < frame + shutter / 2
    # the definition, in binary64
    assert u == [frame + shutter * ((j + 0.5) / n - 0.5) for j in range(n)]


def test_shutter_times_without_a_shutter_are_the_frame():
    from bhr_amd.drivers import shutter_times
    assert shutter_times(12, 0.0, 4) == [12.0] * 4


@pytest.mark.parametrize("kw", [dict(shutter=-0.1), dict(shutter=1.5), dict(shutter=float("nan")), dict(shutter="0.5"),
                                dict(shutter=0.5, shutter_samples=0), dict(shutter=0.5, shutter_samples=65),
                                dict(shutter=0.5, shutter_samples=2.5), dict(shutter_samples=0), dict(shutter=0.5, shutter_samples=True)])
def test_render_video_refuses_bad_shutter_arguments(kw, tmp_path):
    """Before anything is touched: no renderer is needed to be refused."""
    from bhr_amd import drivers
    with pytest.raises(ValueError, match="shutter"):
        drivers.render_video(None, 64, 36, n_frames=3, fps=24, output_path=str(tmp_path / "v.mp4"), fov=90,
                             static_cam_pos=[6, 0, 0.5], **kw)
    assert not list(tmp_path.iterdir())


def test_cli_shutter_arguments(capsys):
    from bhr_amd import cli
    a = cli.parse_args(["--video"])
    assert (a.shutter, a.shutter_samples) == (0.0, 8)
    a = cli.parse_args(["--video", "--shutter", "0.5", "--shutter_samples", "4"])
    assert (a.shutter, a.shutter_samples) == (0.5, 4)
    cli.validate_args(a)
    assert cli.parse_args(["--shutter_samples", "4"]).shutter == 0.0        # without a shutter the count means nothing
    with pytest.raises(SystemExit):                                           # parser.error
        cli.parse_args(["--shutter", "0.5"])
    assert "--shutter needs --video" in capsys.readouterr().err
    for bad in (["--shutter", "1.5"], ["--shutter", "-0.5"], ["--shutter", "0.5", "--shutter_samples", "0"],
                ["--shutter", "0.5", "--shutter_samples", "65"]):
        with pytest.raises(ValueError, match="shutter"):
            cli.validate_args(cli.parse_args(["--video"] + bad))


def test_progress_params_carry_the_shutter_only_when_it_is_open():
    from bhr_amd.drivers import progress_params
    base = {"n_frames": 24, "fov": 90, "orbit": True, "disk_rotation_speed": 0.1, "orbit_degrees": 90.0}
    assert progress_params(24, 90, True, 0.1, 90.0) == base
    assert progress_params(24, 90, True, 0.1, 90.0, shutter=0.0, shutter_samples=8) == base
    assert progress_params(24, 90, True, 0.1, 90.0, shutter=0, shutter_samples=3) == base      # the count alone changes nothing
    assert progress_params(24, 90, True, 0.1, 90.0, shutter=0.5, shutter_samples=4) == dict(base, shutter=0.5, shutter_samples=4)
    assert progress_params(24, 90, True, 0.1, 90.0, "mjpeg", 80, 8, "blue", 0.25, 8) == dict(
        base, video_codec="mjpeg", video_quality=80, dither="blue", shutter=0.25, shutter_samples=8)
