"""CPU side of adaptive supersampling: the NumPy statement of the criterion (tests/adaptive_ref.py) against a plain loop, the
CLI option and the Python-level refusals that need no GPU."""
import numpy as np
import pytest

from adaptive_ref import contrast, refined_mask


def _loop(bg, disk):
    H, W, _ = bg.shape
    c = np.zeros((H, W), np.float32)
    for j in range(H):
        for i in range(W):
            for nj, ni in ((j, i - 1), (j, i + 1), (j - 1, i), (j + 1, i)):
                if 0 <= nj < H and 0 <= ni < W:
                    for layer in (bg, disk):
                        for ch in range(3):
                            c[j, i] = max(c[j, i], abs(np.float32(layer[j, i, ch] - layer[nj, ni, ch])))
    return c


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (4, 1), (7, 9)])
def test_contrast_is_the_loop_over_edge_neighbours(shape):
    rng = np.random.default_rng(3)
    bg = rng.random(shape + (3,)).astype(np.float32)
    disk = (rng.random(shape + (3,)) ** 4).astype(np.float32)
    c = contrast(bg, disk)
    assert c.dtype == np.float32 and np.array_equal(c, _loop(bg, disk))
    if shape == (1, 1):
        assert c[0, 0] == 0


def test_thresholds():
    rng = np.random.default_rng(4)
    bg = rng.random((6, 8, 3)).astype(np.float32)
    disk = np.zeros_like(bg)
    bg[1:5, 1:6] = 0.5                                     # a flat patch: c == 0 in its interior (rows 2-3, columns 2-4)
    assert not refined_mask(bg, disk, np.inf).any()
    assert refined_mask(bg, disk, -1.0).all()
    m0 = refined_mask(bg, disk, 0.0)
    assert not m0[2, 3] and not m0[3, 3] and m0[0, 0]
    c = contrast(bg, disk)
    t = float(np.sort(c.ravel())[c.size // 2])
    assert np.array_equal(refined_mask(bg, disk, t), c > np.float32(t))    # strict inequality: a pixel AT the threshold stays
    with pytest.raises(AssertionError):
        refined_mask(bg, disk, float("nan"))


def test_cli_option():
    from bhr_amd import cli
    assert cli.parse_args([]).supersample_threshold is None
    a = cli.parse_args(["--supersample", "4", "--supersample_threshold", "0.03"])
    assert a.supersample == 4 and a.supersample_threshold == pytest.approx(0.03)
    cli.validate_args(a)
    cli.validate_args(cli.parse_args(["--supersample", "2", "--supersample_threshold", "inf"]))
    for bad in (["--supersample_threshold", "0.1"], ["--supersample", "1", "--supersample_threshold", "0.1"],
                ["--supersample", "2", "--supersample_threshold", "nan"],
                ["--supersample", "2", "--supersample_threshold", "0.1", "--gpus", "2"]):
        with pytest.raises(ValueError):
            cli.validate_args(cli.parse_args(bad))


def test_python_refusals_without_a_device(hip_lib):
    from bhr_amd import HipRenderer, _lib
    sky, tex = np.zeros((4, 8, 3), np.float32), np.zeros((4, 8, 4), np.float32)
    for thr in (float("nan"), "0.1", True):
        with pytest.raises(ValueError):
            HipRenderer(8, 8, sky, tex, supersample=2, supersample_threshold=thr)
    assert hip_lib.bhr_set_adaptive_supersample(None, 2, 0.1) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_adaptive_info(None, None) == _lib.BHR_ERR_INVALID
