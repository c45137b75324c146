"""Supersampling without a device: the CLI flag, the binding's and the drivers' refusals, the C entry point's argument
check, and the NumPy box filter (tests/supersample_ref.py) the GPU tests hold the march to."""
import numpy as np
import pytest

from supersample_ref import box_resolve


def test_cli_flag_default_choices_and_gpus():
    from bhr_amd import cli
    assert cli.parse_args([]).supersample == 1
    assert cli.parse_args(["--supersample", "4"]).supersample == 4
    with pytest.raises(SystemExit):
        cli.parse_args(["--supersample", "3"])
    with pytest.raises(ValueError):
        cli.validate_args(cli.parse_args(["--gpus", "2", "--supersample", "2"]))
    cli.validate_args(cli.parse_args(["--gpus", "2"]))
    cli.validate_args(cli.parse_args(["--supersample", "8"]))


def test_binding_refuses_a_bad_factor_before_any_device(hip_lib):
    from bhr_amd import HipRenderer, drivers, scenes
    sky, tex = scenes.analytic_skybox(8, 16), scenes.noisy_disk(8, 16)
    for k in (3, 0, 16, True):
        with pytest.raises(ValueError):
            HipRenderer(8, 8, sky, tex, supersample=k)
    with pytest.raises(ValueError):
        drivers.render_image(64, 36, [6, 0, 0.5], 90, 0.1, gpus=2, supersample=2)


def test_c_entry_point_checks_its_context(hip_lib):
    from bhr_amd import _lib
    assert hip_lib.bhr_set_supersample(None, 2) == _lib.BHR_ERR_INVALID
    assert hip_lib.bhr_set_supersample(None, 1) == _lib.BHR_ERR_INVALID


def test_box_resolve_sums_rows_first_as_pairwise_trees():
    e = np.float32(2.0 ** -24)
    # k = 2: (1 + e) + (0 + e) rounds to 1 twice; the column-first order, (1 + 0) + (e + e) = 1 + 2^-23, does not
    fine = np.zeros((2, 2, 3), np.float32)
    fine[0, 0], fine[0, 1], fine[1, 1] = 1.0, e, e
    out = box_resolve(fine, 2)
    assert out.shape == (1, 1, 3) and out.dtype == np.float32
    assert out[0, 0, 0] == np.float32(0.25)
    # k = 4: the row [1, 0, e, e] is (1 + 0) + (e + e) = 1 + 2^-23 as a pairwise tree, 1 summed left to right
    fine = np.zeros((4, 4, 3), np.float32)
    fine[2, :, 1] = [1.0, 0.0, e, e]
    out = box_resolve(fine, 4)
    assert out[0, 0, 1] == np.float32((1.0 + 2.0 ** -23) / 16) and out[0, 0, 0] == 0.0
    # k = 8 over several output pixels: the mean of exactly representable values, pixel by pixel
    rng = np.random.default_rng(1)
    fine = (rng.integers(0, 256, (16, 24, 3)) / 256.0).astype(np.float32)
    want = fine.reshape(2, 8, 3, 8, 3).astype(np.float64).mean(axis=(1, 3))
    np.testing.assert_array_equal(box_resolve(fine, 8), want.astype(np.float32))
    np.testing.assert_array_equal(box_resolve(fine, 1), fine)
