"""The restatement of the HDR video stream (tests/hdr_ref.py) against the standards' fixed points, and its f32 version -- the
kernel's operations in the kernel's order -- against the binary64 truth on the inputs of tests/test_gpu_hdr_stream.py.  No GPU.

The quoted values of PQ at 203 nits (0.5807) and of HLG at scene 1.0 (0.7500) are the standards' four-decimal roundings of
0.5806888810 and 0.7500277525; they are checked to the digits quoted (half a unit of the fourth decimal) and the restatement to
1e-6 of the full values, which are the formulas evaluated in Python's own binary64 arithmetic.  Every other fixed point is exact
and holds to 1e-6."""
import math

import numpy as np
import pytest

import grade_ref as G
import hdr_ref as H
from hdr_cases import CONFIGS, SIZES, layer_sets

F32 = np.float32


def test_pq_fixed_points():
    assert abs(float(H.pq_oetf(1.0)) - 1.0) <= 1e-6                            # 10000 nits
    assert H.code_y(H.pq_oetf(1.0)) == 940
    assert H.code_y(H.pq_oetf(0.0)) == 64 and float(H.pq_oetf(0.0)) < 1e-6
    e203 = float(H.pq_oetf(203.0 / 10000.0))
    assert abs(e203 - 0.5807) <= 5e-5 and abs(e203 - 0.5806888810) <= 1e-6
    # the same through the whole chain: grey of scene value 1.0 at white_nits 203 and at 10000
    one = np.ones((2, 2, 3), F32)
    assert abs(float(H.transfer_of(H.linear_2020(one, 0.0), "pq", 203.0)[0, 0, 1]) - 0.5806888810) <= 1e-6
    assert H.encode(one, "pq", 0.0, 10000.0)["y"].tolist() == [[940, 940], [940, 940]]
    assert H.encode(np.zeros((2, 2, 3), F32), "pq")["y"].tolist() == [[64, 64], [64, 64]]


def test_hlg_fixed_points():
    assert abs(float(H.hlg_oetf(1.0 / 12.0)) - 0.5) <= 1e-6
    assert abs(float(H.hlg_oetf(1.0)) - 1.0) <= 1e-6
    scene1 = float(H.transfer_of(np.float64(1.0), "hlg", 0.0))
    assert abs(scene1 - 0.7500) <= 5e-5 and abs(scene1 - 0.7500277525) <= 1e-6
    # both branches meet at E = 1/12
    below, above = float(H.hlg_oetf(1.0 / 12.0 - 1e-9)), float(H.hlg_oetf(1.0 / 12.0 + 1e-9))
    assert abs(below - above) <= 1e-6
    assert float(H.hlg_oetf(0.0)) == 0.0


def test_constants_are_the_standards():
    assert (H.PQ_M1, H.PQ_M2, H.PQ_C1, H.PQ_C2, H.PQ_C3) == (0.1593017578125, 78.84375, 0.8359375, 18.8515625, 18.6875)
    assert abs(H.PQ_C1 - (H.PQ_C3 - H.PQ_C2 + 1.0)) <= 1e-15                   # ST 2084: c1 = c3 - c2 + 1
    for row in H.M_709_TO_2020:
        assert abs(sum(row) - 1.0) <= 1e-12                                      # white stays white
    assert abs(sum(H.LUMA) - 1.0) <= 1e-12
    assert abs(H.CB_DIV - 2.0 * (1.0 - H.LUMA[2])) <= 1e-12 and abs(H.CR_DIV - 2.0 * (1.0 - H.LUMA[0])) <= 1e-12
    assert abs(H.HLG_A * math.log(12.0 - H.HLG_B) + H.HLG_C - 1.0) <= 1e-6


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("transfer", H.TRANSFERS)
def test_grey_has_neutral_chroma(transfer, dtype):
    for v in (0.0, 1e-4, 0.18, 1.0, 2.1, 50.0, 65504.0):
        for stops in (-2.0, 0.0, 1.5):
            out = H.encode(np.full((4, 6, 3), v, F32), transfer, stops, 203.0, dtype)
            assert (out["cb"] == 512).all() and (out["cr"] == 512).all(), (v, stops)
            assert (out["y"] == out["y"][0, 0]).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("transfer", H.TRANSFERS)
def test_codes_are_monotone_in_the_input(transfer, dtype):
    ramp = np.concatenate([[0.0], np.geomspace(1e-7, 65504.0, 4093), [65504.0, 65504.0]]).astype(F32)       # 4096 grey values
    plane = np.repeat(ramp.reshape(64, 64, 1), 3, axis=2)
    for stops in (-2.0, 0.0, 1.5):
        y = H.encode(plane, transfer, stops, 203.0, dtype)["y"].reshape(-1).astype(np.int32)
        assert (np.diff(y) >= 0).all() and y[0] == 64 and y[-1] == 940
    # one primary rising, the others fixed: the luma code never falls (the colour differences may, once the primary has clipped).
    # In binary64 only: where the luma moves by less than an f32 rounding per step, an f32 power function need not be monotone
    for ch in range(3 if dtype is np.float64 else 0):
        plane = np.full((64, 64, 3), 0.25, F32)
        plane[..., ch] = ramp.reshape(64, 64)
        y = H.encode(plane, transfer, 0.0, 203.0, dtype)["y"].reshape(-1).astype(np.int32)
        assert (np.diff(y) >= 0).all()


def test_light_levels_of_the_restatement():
    h = np.zeros((2, 4, 3), F32)
    h[0, 1] = (1.0, 1.0, 1.0)
    h[1, 2] = (100.0, 0.0, 0.0)
    out = H.encode(h, "pq", 0.0, 203.0)
    assert abs(out["max_nits"] - 10000.0) <= 1e-9                                 # 203 * 62.74, capped
    assert abs(out["mean_nits"] - (203.0 + 10000.0) / 8.0) <= 1e-6
    out = H.encode(h, "pq", -2.0, 100.0)
    assert abs(out["max_nits"] - 100.0 * 25.0 * 0.6274) <= 1e-9
    assert (H.encode(h, "hlg")["max_nits"], H.encode(h, "hlg")["mean_nits"]) == (0.0, 0.0)
    assert H.light_levels([(5.0, 1.0), (3.0, 2.0)]) == (5.0, 2.0) and H.light_levels([]) == (0.0, 0.0)


@pytest.mark.parametrize("size", SIZES)
def test_f32_version_is_within_one_code_of_binary64_on_the_gpu_inputs(size):
    """The kernel's arithmetic, restated in f32, against the truth on exactly the planes of the GPU test: every sample within one
    code, and at most 1 % of the samples of each plane -- Y, Cb, Cr -- different at all (hdr_ref.Tally: per frame where a frame's
    plane has a hundred samples, and over the frames of a transfer at this size).  The cap is a condition, not a measurement: a
    wrong constant moves nearly every sample."""
    w, h = size
    tally = H.Tally()
    for name, layers in layer_sets(w, h).items():
        plane = G.hdr_plane(*layers)
        for cfg in CONFIGS:
            want = H.encode(plane, **cfg)
            got = H.encode(plane, dtype=np.float32, **cfg)
            tally.add(cfg["transfer"], (got["y"], got["cb"], got["cr"]), want, f"{w}x{h} {name} {cfg}")
            if cfg["transfer"] == "pq":
                assert abs(got["max_nits"] - want["max_nits"]) <= 1e-6 * want["max_nits"]
                assert abs(got["mean_nits"] - want["mean_nits"]) <= 1e-6 * want["mean_nits"] + 1e-12
    print(f"[hdr ref] {w}x{h}: f32 one code off in " + tally.check())
