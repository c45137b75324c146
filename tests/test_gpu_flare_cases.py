"""Device lens flare (csrc/flare.hip) beyond the landscape frames of tests/test_gpu_flare.py: every case of tests/flare_cases.py
(portrait, square, tiny and scale-1 frames; sources on a pixel, a corner and the frame's middle; totals a float32 either side of
the 0.01 threshold; ratio below, at and above 1; frames that clip everywhere), the frame sums where the fold kernel's batches
iterate and where a frame has fewer than 8 pixels, a context reused after a bright frame, the HDR plane where the flare exceeds
1, and row blocks of a portrait frame.  tests/test_flare_ref.py pins the restatement these compare with and shows, without a
device, that every case is what it was chosen for.

The bar is tests/test_gpu_flare.py's TOL, one f32 ulp below 1.0, imported and not restated; sums and untouched frames are equal
bit for bit."""
import numpy as np
import pytest

import flare_cases as FC
import grade_ref as G
from test_gpu_flare import TOL, _blank

pytestmark = pytest.mark.gpu
F = FC.F
ids = lambda c: c.name


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


@pytest.fixture(scope="module")
def contexts(hip_lib):
    """One blank context per frame size, shared by the cases of that size (a case writes both layers it reads)."""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = _blank(w, h)
        return made[(w, h)]
    yield get
    for r in made.values():
        r.close()


def _flare(r, final, disk):
    from bhr_amd import _lib
    r.write_layer(_lib.LAYER_FINAL, final)
    r.write_layer(_lib.LAYER_DISK, disk)
    r.apply_lens_flare()
    return r.read_layer(_lib.LAYER_FINAL)


def test_the_bar_is_one_ulp_below_one():
    assert np.spacing(np.nextafter(F(1), F(0))) <= TOL < np.spacing(F(1))


@pytest.mark.parametrize("case", FC.CASES, ids=ids)
def test_table_cases_against_the_restatement(case, contexts):
    final, disk = FC.inputs(case)
    want = FC.restated(case)
    got = _flare(contexts(case.w, case.h), final, disk)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"[flare cases] {case.name}: device - restatement {err:.3g}, {int((got != want).sum())} of {want.size} values differ")
    if not case.flared:
        np.testing.assert_array_equal(_bits(got), _bits(final))
    else:
        assert (want != final).any() or case.final == "one"
        assert err <= TOL, f"{case.name}: the device is {err:.3g} from the restatement"


@pytest.mark.parametrize("size", FC.SUM_SHAPES_TINY + FC.SUM_SHAPES_LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sums_are_numpys_where_the_fold_iterates_and_on_tiny_frames(size, hip_lib):
    """Equality, as in test_flare_sums_are_numpys: more than 256 chunk sums (the fold loop's second batch), exactly 256 and a
    ragged rest, no rest at all, portrait, and frames of fewer than 8 pixels (leaf_sum's short branch)."""
    from bhr_amd import _lib
    w, h = size
    r = _blank(w, h)
    for name, glow in FC.sum_planes(w, h).items():
        r.write_layer(_lib.LAYER_DISK, np.repeat(glow[..., None], 3, axis=2))
        got, want = r.lens_flare_sums(), FC.numpy_sums(glow)
        print(f"[flare sums] {w}x{h} {name}: device {got.tolist()} NumPy {want.tolist()}")
        np.testing.assert_array_equal(got, want, err_msg=f"{w}x{h} {name}")
    r.close()


def test_a_dark_frame_after_a_bright_one_is_left_alone(contexts):
    """The context keeps its frame sums between calls: they must be the current disk layer's, every time."""
    bright, dark = FC.BY_NAME["64x36-rand_sat"], FC.BY_NAME["64x36-thr_below"]
    r = contexts(64, 36)
    first = _flare(r, *FC.inputs(bright))
    assert np.abs(first - FC.inputs(bright)[0]).max() > 0.01
    fresh = FC.inputs(dark)[0] * F(0.5)                          # a frame the context has not seen
    np.testing.assert_array_equal(_bits(_flare(r, fresh, FC.inputs(dark)[1])), _bits(fresh))
    np.testing.assert_array_equal(_bits(_flare(r, *FC.inputs(bright))), _bits(first))


@pytest.mark.parametrize("size", [(64, 36), (36, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("math", ["strict", "hybrid"])
def test_the_hdr_plane_keeps_the_whole_flare(math, size, hip_lib):
    """flare_apply_kernel<true> has no upper clip: the plane is max(s + flare, 0) with the restatement's unclipped term, on every
    value.  An f32 ulp grows with the value, so the bar is TOL max(1, want)."""
    from bhr_amd import _lib
    from oracle.flare_np import flare_term
    from test_gpu_grade import _default
    r, s = _default(math, w=size[0], h=size[1], lens_flare=True)
    r.set_grade(keep_hdr=True, tonemap="aces", transfer="srgb", exposure=1.0)
    r.render_async(s["cam_pos"], s["fov"])
    hdr = r.read_hdr()
    bg, disk, blur = (r.read_layer(k) for k in (_lib.LAYER_BG, _lib.LAYER_DISK, _lib.LAYER_BLUR))
    r.close()
    sm, term = G.combine(bg, disk, blur), flare_term(disk)
    assert term is not None and term.dtype == F
    want = np.maximum(sm + term, F(0))
    assert want.dtype == F
    err = np.abs(hdr.astype(np.float64) - want) / np.maximum(1.0, want)
    print(f"[flare hdr] {math} {size[0]}x{size[1]}: flare <= {term.max():.4g}, {float((term > 1).mean()):.1%} of its values above 1, "
          f"plane <= {want.max():.4g}, device - restatement {float(err.max()):.3g} of max(1, value)")
    assert term.max() > 1                                        # the headroom is really exercised
    assert err.max() <= TOL


def test_flare_in_row_blocks_of_a_portrait_frame(hip_lib):
    """tests/test_gpu_flare.py's row-block frame with min(w, h) == w: tile 0's sums handed to every tile's apply launch."""
    from bhr_amd import HipRenderer, _lib, scenes
    from bhr_amd.multigpu import group_render, row_blocks
    from oracle.flare_np import apply_lens_flare
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    kw = dict(step_size=0.1, disk_tilt=25.0, anti_alias="lod_radius")
    cam, fov, (w, h) = [6, 0, 0.5], 90, (90, 160)
    r = HipRenderer(w, h, sky, tex, **kw)
    r.render_async(cam, fov)
    base, disk = r.read_layer(_lib.LAYER_FINAL), r.read_layer(_lib.LAYER_DISK)
    r.close()
    want = apply_lens_flare(base, disk)
    assert np.abs(want - base).max() > 0.01
    tiles = [HipRenderer(w, h, sky, tex, rows=rows, **kw) for rows in row_blocks(h, 5)]
    got = group_render(tiles, cam, fov, lens_flare=True)
    for t in tiles:
        t.close()
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"[flare rows] {w}x{h} in 5 row blocks: device - restatement {err:.3g}")
    assert err <= TOL
