"""The lens-flare edge cases without a device: oracle/flare_np.py is held to the reference's own output on the stored subset
(tests/golden/flare_cases.npz, made by tests/golden/make_flare_golden.py) bit for bit, and every case of tests/flare_cases.py is
shown to be what it was chosen for, so that tests/test_gpu_flare_cases.py cannot quietly stop testing it."""
import os

import numpy as np
import pytest

import flare_cases as FC

F = FC.F
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ids = lambda c: c.name
FLARED = tuple(c for c in FC.CASES if c.flared)
UNTOUCHED = tuple(c for c in FC.CASES if not c.flared)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.fixture(scope="module")
def stored():
    return np.load(os.path.join(GOLD, "flare_cases.npz"))


# ---- the pin ---------------------------------------------------------------------------------------------------------------
def test_the_stored_subset_is_the_table_s(stored):
    assert sorted(stored.files) == sorted(c.name for c in FC.GOLDEN)
    shapes = {(c.w, c.h) for c in FC.GOLDEN}
    assert any(w > h >= FC.WHOLE_SHAPES_FROM for w, h in shapes) and any(h > w for w, h in shapes) and any(w * h < 8 for w, h in shapes)
    for w, h in FC.GOLDEN_SHAPES:
        assert {c.plane for c in FC.GOLDEN if (c.w, c.h) == (w, h)} >= set(FC.PLANES)
    assert {c.plane for c in FC.GOLDEN} >= set(FC.TRIO)


@pytest.mark.parametrize("case", FC.GOLDEN, ids=ids)
def test_the_restatement_is_the_reference_bit_for_bit(case, stored):
    want = stored[case.name]
    assert want.dtype == F and want.shape == (case.h, case.w, 3)
    np.testing.assert_array_equal(_bits(FC.restated(case)), _bits(want))


def test_the_restatement_still_gives_the_first_vector():
    """apply_lens_flare is built on flare_term now: tests/golden/misc.npz, the vector it has always been held to."""
    from oracle.flare_np import apply_lens_flare, flare_term
    d = np.load(os.path.join(GOLD, "misc.npz"))
    final, disk, want = (d[k].transpose(1, 0, 2) for k in ("flare_final", "flare_disk", "flare_out"))
    np.testing.assert_array_equal(_bits(apply_lens_flare(final, disk)), _bits(want))
    np.testing.assert_array_equal(_bits(apply_lens_flare(final, np.zeros_like(disk))), _bits(d["flare_dark_out"].transpose(1, 0, 2)))
    assert flare_term(np.zeros_like(disk)) is None
    term = flare_term(disk)
    assert term.dtype == F
    np.testing.assert_array_equal(_bits(np.clip(final + term, 0, 1)), _bits(want))


# ---- the premises ----------------------------------------------------------------------------------------------------------
def test_the_table_has_every_plane_on_every_shape():
    assert len({c.name for c in FC.CASES}) == len(FC.CASES) == len(FC.SHAPES) * (len(FC.PLANES) + 2) + len(FC.TRIO)
    for w, h in FC.SHAPES:
        mine = [c for c in FC.CASES if (c.w, c.h) == (w, h)]
        assert {c.plane for c in mine} >= set(FC.PLANES)
        assert sorted(c.final for c in mine if c.final != "rand") == ["one", "zero"]
    assert any(w < h and min(w, h) >= FC.WHOLE_SHAPES_FROM for w, h in FC.SHAPES) and (640, 360) in FC.SHAPES
    assert [c.name for c in UNTOUCHED] == ["1x1-dim", "3x2-dim", "64x36-thr_below"]
    below, exact, above = (FC.TRIO[k] for k in ("thr_below", "thr_exact", "thr_above"))
    assert below < exact < above and exact == F(0.01) and F(np.nextafter(below, F(1))) == exact == F(np.nextafter(above, F(0)))


@pytest.mark.parametrize("case", UNTOUCHED, ids=ids)
def test_untouched_cases_return_the_frame(case):
    final, disk = FC.inputs(case)
    total = np.sum(np.max(disk, axis=2).T.copy())
    assert total.dtype == F and 0 < total < FC.THRESHOLD
    assert FC.term(case) is None
    np.testing.assert_array_equal(_bits(FC.restated(case)), _bits(final))


@pytest.mark.parametrize("case", FLARED, ids=ids)
def test_flared_cases_are_what_they_were_chosen_for(case):
    final, disk = FC.inputs(case)
    probe = {}
    term = FC.term(case, probe)
    out = FC.restated(case)
    assert term is not None and term.dtype == F and term.min() >= 0
    assert probe["total"].dtype == F and probe["total"] >= FC.THRESHOLD
    np.testing.assert_array_equal(_bits(out), _bits(np.clip(final + term, 0, 1)))
    moved = float(np.abs(out - final).max())
    print(f"[flare cases] {case.name}: total {probe['total']!r} ratio {probe['ratio']!r} src {probe['src']} term <= {term.max():.4g} moved {moved:.4g}")

    # how far the frame moves
    if case.plane == "dim":
        # strength = 0.0015.  The lit pixel itself is on the first streak with falloff 1: f32(0.0015 * 0.3) = 4.5e-4 at the least;
        # all 13 shapes at their peaks on one pixel would give 0.0015 (5.76 + 1.125 + 0.3 + 2 * 0.3) = 0.0117 at the most
        assert 4.4e-4 <= term.max() <= 0.0117 and 0 < moved <= 0.0118
    elif case.faint:
        # total = 0.01 on 64 x 36: strength = 1.5 * 0.01 / 691.2 = 2.17e-5, by the same sums 6.5e-6 .. 1.7e-4; most of the frame
        # is inside the larger ghosts and every value there changes (a value of 0.15 has an ulp of 1.5e-8)
        assert 6.4e-6 <= term.max() <= 1.7e-4 and 0 < moved <= 1.7e-4
        assert (out != final).mean() > 0.5
    elif case.final == "one":
        assert term.max() > 0.01 and (out == 1).all()              # the clip is active on every value
    else:
        assert moved > 0.01
    if case.final == "zero":
        np.testing.assert_array_equal(_bits(out), _bits(np.minimum(term, F(1))))

    # the strength
    ratio = probe["ratio"]
    assert ratio.dtype == F
    assert bool(1 < ratio) == case.saturated
    if case.plane == "const03":
        assert bool(ratio == 1.0) == ((case.w, case.h) in FC.CONST03_RATIO_IS_ONE)
    elif case.plane in ("corner00", "cornerWH"):
        assert ratio == 0.5
    elif case.plane == "centre":
        assert ratio == 2.0

    # where the source lies
    sx, sy = probe["src"]
    if case.plane == "corner00":
        assert (sx, sy) == (0.0, 0.0)
    elif case.plane == "cornerWH":
        assert (sx, sy) == (case.w - 1.0, case.h - 1.0)
    elif case.plane == "centre":
        assert (sx, sy) == (float(case.w // 2), float(case.h // 2))
        if case.w % 2 == 0 and case.h % 2 == 0:
            assert (sx, sy) == (case.w / 2, case.h / 2)             # src == mid: all 13 shapes are concentric
    elif case.plane == "two_blobs" and min(case.w, case.h) >= FC.WHOLE_SHAPES_FROM:
        glow = np.max(disk, axis=2)
        assert glow[int(round(sy)), int(round(sx))] < 1e-3 * glow.max()         # the centroid lies on no light

    # every shape is there and ends inside the frame: the device's skip tests go both ways
    if min(case.w, case.h) >= FC.WHOLE_SHAPES_FROM:
        for name in FC.SHAPE_NAMES:
            plane = probe[name]
            assert (plane != 0).any() and (plane == 0).any(), f"{case.name}: {name} has {(plane != 0).sum()} of {plane.size} pixels"
    if min(case.w, case.h) <= 7:
        assert 25 * min(case.w, case.h) / 360.0 < 0.5                # the first ghost is thinner than a pixel

    # the one discontinuous edge: a pixel whose delta is a last bit from 0.05 could change sides with another libm
    for delta in probe["delta"]:
        assert np.abs(delta - 0.05).min() > 1e-9


def test_a_source_on_a_pixel_meets_atan2_of_zero_and_a_row_of_zero_dy():
    case = FC.BY_NAME["64x36-corner00"]
    probe = {}
    FC.term(case, probe)
    sx, sy = probe["src"]
    assert sx == int(sx) and sy == int(sy)
    on = probe["streaks"]                                            # (W, H)
    assert on[int(sx), int(sy)] == 1                                 # atan2(0, 0) = 0: on the first axis only
    assert (on[int(sx) + 1:, int(sy)] == 1).all() and (on[int(sx), int(sy) + 1:] == 1).all()


# ---- the sum planes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", FC.SUM_SHAPES_LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_sum_planes_tell_numpy_s_order_from_others(size):
    """A device sum that equals np.sum on these planes took NumPy's order: an accurate sum, a sequential one and the pairwise
    sum over the other memory order all give another f32."""
    w, h = size
    planes = FC.sum_planes(w, h)
    assert list(planes) == ["rand4", "loguniform", "sparse", "const03"]
    n = w * h
    assert n // FC.CHUNK > 256 or (n // FC.CHUNK == 256 and n % FC.CHUNK)          # the fold's second batch, or exactly one full batch
    for name in ("rand4", "loguniform"):
        glow_hw = planes[name]
        glow = np.ascontiguousarray(glow_hw.T)
        s0 = np.sum(glow)
        assert s0.dtype == F and FC.numpy_sums(glow_hw)[0] == s0
        others = {"f64 rounded": F(np.sum(glow.astype(np.float64))),
                  "sequential f32": np.cumsum(glow.ravel(), dtype=F)[-1],
                  "(H, W) order": np.sum(np.ascontiguousarray(glow_hw))}
        print(f"[flare sums] {w}x{h} {name}: np.sum {s0!r}; " + ", ".join(f"{k} {v!r}" for k, v in others.items()))
        for k, v in others.items():
            assert v.dtype == F and v != s0, f"{w}x{h} {name}: the {k} sum equals np.sum"


@pytest.mark.parametrize("size", FC.SUM_SHAPES_TINY + FC.SUM_SHAPES_LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_sum_shapes_reach_their_branches(size):
    w, h = size
    n = w * h
    chunks, tail = divmod(n, FC.CHUNK)
    want = {(1, 1): (0, 1), (3, 2): (0, 6), (9, 1): (0, 9), (7, 5): (0, 35), (2056, 1024): (257, 0), (2053, 1031): (258, 3107),
            (1031, 2053): (258, 3107), (1450, 1450): (256, 5348)}
    assert (chunks, tail) == want[size]
    sparse = FC.sum_planes(w, h)["sparse"]
    assert (sparse == 0).any() or n < 8
    if n > 1000:
        assert 0.0005 < (sparse != 0).mean() <= 0.001
