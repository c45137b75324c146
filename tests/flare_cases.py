"""The cases of the lens-flare edge tests: one table for tests/golden/make_flare_golden.py (the reference's own output on a
subset), tests/test_flare_ref.py (the restatement pinned to it, and every case's premise, without a device) and
tests/test_gpu_flare_cases.py (csrc/flare.hip against the restatement).

A case is a name, a frame size and two recipes -- the disk layer's and the frame's; the table holds no arrays.  Everything is
float32 and seeded, so the three users build the same inputs.  Arrays are (H, W, 3) as the library takes them; the restatement
(oracle/flare_np.py) moves them into the reference's (W, H, 3) order itself.

What the flare does with a disk layer hangs on total = np.sum(max(r, g, b)) in f32: under 0.01 the frame is returned untouched,
ratio = total / (0.3 w h) is the strength, capped at 1 ("saturated": Python's min() then hands back the float 1.0 and the
promotions change), and the total's centroid is the source every shape is placed from.  A = 0.3 w h below."""
import functools
import typing

import numpy as np

from oracle.flare_np import apply_lens_flare, flare_term

F = np.float32
THRESHOLD = F(0.01)
SHAPE_NAMES = tuple(f"ghost{g}" for g in range(8)) + tuple(f"ring{k}" for k in range(3)) + ("hex", "streaks")     # the 13 shapes

# w x h.  640 x 360: scale exactly 1; 200 x 360, 36 x 64, 33 x 97, 5 x 7: min(w, h) is the width; 45 x 45: both
SHAPES = ((1, 1), (3, 2), (7, 5), (5, 7), (64, 36), (36, 64), (97, 33), (33, 97), (45, 45), (160, 90), (517, 131), (200, 360),
          (640, 360))
WHOLE_SHAPES_FROM = 33               # min(w, h) from which every one of the 13 shapes has pixels inside and outside it
PLANES = ("corner00", "cornerWH", "centre", "dim", "rand_unsat", "rand_sat", "const03", "const09", "two_blobs")
TRIO_SHAPE, TRIO_AT = (64, 36), (20, 10, 1)          # the threshold trio: channel 1 of pixel x = 20, y = 10
TRIO = {"thr_below": np.nextafter(THRESHOLD, F(0)), "thr_exact": THRESHOLD, "thr_above": np.nextafter(THRESHOLD, F(1))}
# ratio > 1 ("saturated") by plane kind, and where a frame is too small for the kind's long-run mean.  rand ** 4: the mean of the
# largest of three draws is 3 / 7, so ratio 0.43 and 1.43 -- of one and of six pixels it is what the draws give.  The two blobs
# share their pixels on the two smallest frames.
SATURATED_PLANES = ("centre", "rand_sat", "const09")
SATURATED_EXCEPT = {("rand_sat", (1, 1)): False, ("rand_sat", (3, 2)): False, ("two_blobs", (1, 1)): True, ("two_blobs", (3, 2)): True}
# const03: the f32 np.sum of the plane against f32(0.3 w h).  Equal, so ratio == 1.0 exactly and 1 < ratio is False, on five
# frames; an ulp or more above on three (saturated); below on the rest.
CONST03_RATIO_IS_ONE = ((1, 1), (3, 2), (45, 45), (160, 90), (517, 131))
CONST03_SATURATED = ((7, 5), (5, 7), (640, 360))


class Case(typing.NamedTuple):
    name: str
    w: int
    h: int
    plane: str                       # one of PLANES or of TRIO
    final: str = "rand"              # "rand": rand 0.3; "zero"; "one": the upper clip is active on every value

    @property
    def area(self):
        return 0.3 * self.w * self.h

    @property
    def flared(self):
        """False: the total is under the threshold and the frame must come back bit for bit."""
        if self.plane == "dim":
            return 0.001 * self.area >= 0.01          # 1 x 1 and 3 x 2 only are under it (7 x 5: 0.0105)
        return self.plane != "thr_below"

    @property
    def saturated(self):
        """1 < f32 ratio, for a flared case."""
        if self.plane == "const03":
            return (self.w, self.h) in CONST03_SATURATED
        return SATURATED_EXCEPT.get((self.plane, (self.w, self.h)), self.plane in SATURATED_PLANES)

    @property
    def faint(self):
        """Flared, but by far less than 0.01: the premise is the flare's expected size instead."""
        return self.flared and self.plane in ("dim", "thr_exact", "thr_above")


def _lit_pixel(w, h, x, y, value):
    disk = np.zeros((h, w, 3), F)
    disk[y, x] = F(value)
    return disk


def _two_blobs(w, h):
    """Gaussians around the points 1/8 and 7/8 along the diagonal: their centroid is the frame's middle, where neither shines."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    sigma = max(min(w, h) / 10.0, 0.6)
    blob = sum(np.exp(-((xx - (w - 1) * t) ** 2 + (yy - (h - 1) * t) ** 2) / (2 * sigma * sigma)) for t in (0.125, 0.875))
    return (blob[..., None] * np.array([1.0, 0.8, 0.5])).astype(F)


def disk_plane(case):
    w, h, a = case.w, case.h, case.area
    rng = np.random.default_rng([w, h, (PLANES + tuple(TRIO)).index(case.plane)])
    if case.plane == "corner00":                     # ratio 0.5, strength 0.75, the source exactly on pixel (0, 0)
        return _lit_pixel(w, h, 0, 0, 0.5 * a)
    if case.plane == "cornerWH":
        return _lit_pixel(w, h, w - 1, h - 1, 0.5 * a)
    if case.plane == "centre":                       # ratio 2: saturated; on an even frame src == mid, all 13 shapes concentric
        return _lit_pixel(w, h, w // 2, h // 2, 2.0 * a)
    if case.plane == "dim":
        return _lit_pixel(w, h, w // 4, h // 3, 0.001 * a)
    if case.plane == "rand_unsat":
        return (rng.random((h, w, 3), dtype=F) ** 4 * F(0.3)).astype(F)
    if case.plane == "rand_sat":
        return (rng.random((h, w, 3), dtype=F) ** 4).astype(F)
    if case.plane == "const03":
        return np.full((h, w, 3), F(0.3))
    if case.plane == "const09":
        return np.full((h, w, 3), F(0.9))
    if case.plane == "two_blobs":
        return _two_blobs(w, h)
    x, y, c = TRIO_AT
    disk = np.zeros((h, w, 3), F)
    disk[y, x, c] = TRIO[case.plane]
    return disk


def final_plane(case):
    if case.final == "zero":
        return np.zeros((case.h, case.w, 3), F)
    if case.final == "one":
        return np.ones((case.h, case.w, 3), F)
    return np.random.default_rng([case.w, case.h, 1000]).random((case.h, case.w, 3), dtype=F) * F(0.3)


def _cases():
    out = []
    for w, h in SHAPES:
        out += [Case(f"{w}x{h}-{p}", w, h, p) for p in PLANES]
        out += [Case(f"{w}x{h}-rand_unsat-final0", w, h, "rand_unsat", "zero"), Case(f"{w}x{h}-rand_sat-final1", w, h, "rand_sat", "one")]
    w, h = TRIO_SHAPE
    return tuple(out + [Case(f"{w}x{h}-{p}", w, h, p) for p in TRIO])


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# The reference's own output is stored for every plane kind at one landscape, one portrait and one tiny frame, and for the trio.
# The zero frame is pinned on the two small frames only: the fixture stays under 300 KB without its 64 x 36 output.
GOLDEN_SHAPES = ((64, 36), (5, 7), (3, 2))
GOLDEN = tuple(c for c in CASES if (c.w, c.h) in GOLDEN_SHAPES and c.name != "64x36-rand_unsat-final0")


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(final, disk), read-only."""
    out = final_plane(case), disk_plane(case)
    for a in out:
        assert a.dtype == F and a.shape == (case.h, case.w, 3)
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(case):
    """The restatement's frame for the case, computed once."""
    out = apply_lens_flare(*inputs(case))
    out.setflags(write=False)
    return out


def term(case, probe=None):
    return flare_term(inputs(case)[1], probe)


# ------------------------------------------------------------------------------------------------------------ sum planes
# w x h.  The fold kernel adds chunk sums (8192 elements each) in batches of 256 and the ragged rest from a tree: fewer than 8
# elements (leaf_sum's short branch), 257 chunks and no rest, 258 and a rest of 3107 either way round, 256 and a rest of 5348
SUM_SHAPES_TINY = ((1, 1), (3, 2), (9, 1), (7, 5))
SUM_SHAPES_LARGE = ((2056, 1024), (2053, 1031), (1031, 2053), (1450, 1450))
CHUNK = 8192


def sum_planes(w, h):
    """{name: (H, W) f32 glow plane}, drawn in this order from default_rng(1000 h + w)."""
    rng = np.random.default_rng(h * 1000 + w)
    out = {"rand4": (rng.random((h, w), dtype=F) ** 4).astype(F),
           "loguniform": np.exp(rng.uniform(np.log(1e-8), np.log(1e3), (h, w))).astype(F)}
    sparse = np.zeros((h, w), F)
    idx = rng.integers(0, h * w, max(3, h * w // 1000))
    sparse.flat[idx] = rng.random(idx.size, dtype=F) * F(50)
    out["sparse"] = sparse
    out["const03"] = np.full((h, w), F(0.3))
    return out


def numpy_sums(glow_hw):
    """(sum glow, sum x glow, sum y glow) as the reference takes them: np.sum over its (W, H) array."""
    h, w = glow_hw.shape
    glow = np.ascontiguousarray(glow_hw.T)
    xs, ys = np.mgrid[0:w, 0:h]
    return np.array([np.sum(glow), np.sum(xs * glow), np.sum(ys * glow)], dtype=np.float64)
