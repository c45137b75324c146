"""The grading stage on the device (bhr_set_grade / bhr_grade_frame, csrc/grade.hip) against its NumPy restatement
(tests/grade_ref.py): FINAL within grade_ref.TOL of the binary64 formulas, the HDR plane and every quantised row exact."""
import ctypes as C
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import grade_ref as G
import jpeg_ref
import quant_ref as Q
from bhr_amd import scenes
from test_gpu_quantisers import _renderer

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32

SHAPES = [(1, 1), (5, 3), (71, 37), (300, 70)]        # the scalar tail alone, sizes that are no multiple of 4, more than one block
STOPS = (-3.5, 0.0, 2.25)
WHITES = (1.0, 2.5)
GRADES = [dict(tonemap=op, transfer=tr, exposure=st, white=wh) for op in G.OPS for tr in G.TRANSFERS for st in STOPS for wh in WHITES]


@pytest.fixture(scope="module")
def matrix(hip_lib):
    from bhr_amd.output import dither_matrix
    m = dither_matrix()
    m.setflags(write=False)
    return m


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _assert_bits(got, want, msg=""):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=msg)


def _ref(h, g):
    return G.grade_hdr(h, g["tonemap"], g.get("exposure", 0.0), g.get("white", 2.5), g.get("transfer", "linear"))


def _assert_final(final, h, g, msg=""):
    err = np.abs(final.astype(np.float64) - _ref(h, g)).max()
    assert err <= G.TOL, f"{msg} {g}: FINAL is {err:.3g} from the restatement"
    return err


def layer_sets(w, h):
    """(BG, DISK, BLUR) triples: zeros; a ramp through the sRGB toe; noise with sums in [0, 2.5]; 1e4; 65504; and BG / BLUR with
    -1, +inf, -inf and NaN (a written DISK layer is finite and >= 0)."""
    rng = np.random.default_rng(1000 * w + h)
    shape = (h, w, 3)
    zero = np.zeros(shape, F32)
    out = {"zeros": (zero, zero, zero)}
    ramp = np.linspace(0.0031308 / 12.92 * 0.5, 0.01, 3 * w * h, dtype=F32).reshape(shape)
    out["toe ramp"] = (ramp, zero, zero)
    out["toe ramp split"] = (ramp * F32(0.25), ramp * F32(0.5), ramp * F32(0.25))
    out["noise"] = (rng.random(shape, dtype=F32) * F32(0.5), rng.random(shape, dtype=F32), rng.random(shape, dtype=F32))
    out["1e4"] = (zero, np.full(shape, 1e4, F32), rng.random(shape, dtype=F32))
    out["65504"] = (np.full(shape, 65504.0, F32), np.full(shape, 65504.0, F32), zero)
    odd = np.array([-1.0, np.inf, -np.inf, np.nan, 0.25, 0.0], F32)
    bg, blur = odd[rng.integers(0, odd.size, shape)], odd[rng.integers(0, odd.size, shape)]
    bg.reshape(-1)[:3], blur.reshape(-1)[:3] = odd[[1, 3, 0]][:bg.size], odd[[2, 4, 3]][:bg.size]      # inf - inf, NaN, -1 + NaN
    out["non-finite"] = (bg, rng.random(shape, dtype=F32), blur)
    return {k: tuple(np.ascontiguousarray(a, dtype=F32) for a in v) for k, v in out.items()}


def _inject(r, layers):
    from bhr_amd import _lib
    for which, data in zip((_lib.LAYER_BG, _lib.LAYER_DISK, _lib.LAYER_BLUR), layers):
        r.write_layer(which, data)


# ---- 1. injected layers, stand-alone --------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SHAPES)
def test_injected_layers_grade_as_the_restatement(size, matrix, hip_lib):
    w, h = size
    r = _renderer(w, h)
    worst = 0.0
    for name, layers in layer_sets(w, h).items():
        _inject(r, layers)
        want_h = G.hdr_plane(*layers)
        for g in GRADES:
            r.set_grade(keep_hdr=True, **g)
            r.grade_frame()
            final = r.read_layer(0)
            worst = max(worst, _assert_final(final, want_h, g, name))
            _assert_bits(r.read_hdr(), want_h, f"HDR {name} {g}")
            assert np.isfinite(final).all() and final.min() >= 0 and final.max() <= 1
        # the quantisers are functions of the FINAL the device returned (every operator and transfer once per layer set)
        for g in GRADES[::7]:
            r.set_grade(**g)
            r.grade_frame()
            final = r.read_layer(0)
            np.testing.assert_array_equal(r.read_final_u8(), Q.quantize8(final), err_msg=f"u8 {name} {g}")
            np.testing.assert_array_equal(r.read_final_u16(), Q.quantize16(final), err_msg=f"u16 {name} {g}")
            r.set_dither("blue")
            np.testing.assert_array_equal(r.read_final_u8(), Q.quantize8_dither(final, matrix), err_msg=f"dither {name} {g}")
            r.set_dither("none")
            np.testing.assert_array_equal(r.read_final_u8(), Q.quantize8(final), err_msg=f"u8 after dither {name} {g}")
            with pytest.raises(AssertionError):                  # graded without keep_hdr: the frame has no HDR plane
                r.read_hdr()
    print(f"[grade] {w}x{h}: FINAL at most {worst:.3g} from the restatement (bound {G.TOL})")
    r.close()


def test_grade_covers_every_operator_and_transfer_in_the_quantiser_subset():
    sub = GRADES[::7]
    assert {g["tonemap"] for g in sub} == set(G.OPS) and {g["transfer"] for g in sub} == set(G.TRANSFERS)


# ---- 2. identity -----------------------------------------------------------------------------------------------------------
def _default(math="strict", w=64, h=36, **kw):
    from bhr_amd import HipRenderer
    s = scenes.SCENES["default"]
    return HipRenderer(w, h, scenes.analytic_skybox(), scenes.noisy_disk(), math=math, **dict(s["kw"], **kw)), s


def _outputs_of(r, matrix=None):
    out = dict(final=r.read_layer(0), u8=r.read_final_u8(), u16=r.read_final_u16())
    r.set_dither("blue")
    out["dither"] = r.read_final_u8()
    r.set_dither("none")
    return out


def _assert_same_outputs(got, want, tag):
    _assert_bits(got["final"], want["final"], f"{tag}: FINAL")
    for k in ("u8", "u16", "dither"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{tag}: {k}")


@pytest.mark.parametrize("math", ["strict", "hybrid"])
@pytest.mark.parametrize("outputs", ["f32", "u8"])
def test_clip_at_zero_stops_is_the_ungraded_frame(math, outputs, hip_lib):
    r, s = _default(math, outputs=outputs)
    assert r.grade is None
    r.render_async(s["cam_pos"], s["fov"])
    plain = _outputs_of(r)
    assert plain["final"].max() == 1.0
    r.set_grade("clip")
    assert r.grade == dict(tonemap="clip", exposure=0.0, white=2.5, transfer="linear", keep_hdr=False)
    r.render_async(s["cam_pos"], s["fov"])
    _assert_same_outputs(_outputs_of(r), plain, "clip, 0 stops, linear")
    r.set_grade(None)
    assert r.grade is None
    r.render_async(s["cam_pos"], s["fov"])
    _assert_same_outputs(_outputs_of(r), plain, "grade off again")
    r.close()


# ---- 3. rendered and graded ------------------------------------------------------------------------------------------------
RENDERED = [dict(tonemap="aces", transfer="srgb", exposure=1.0), dict(tonemap="reinhard", transfer="linear")]


@pytest.mark.parametrize("math", ["strict", "hybrid"])
@pytest.mark.parametrize("outputs", ["f32", "u8"])
def test_rendered_frames_grade_as_the_restatement_of_their_own_layers(math, outputs, hip_lib):
    from bhr_amd import _lib
    r, s = _default(math, outputs=outputs)
    r.render_async(s["cam_pos"], s["fov"])
    plain = r.read_layer(0)
    for g in RENDERED:
        r.set_grade(keep_hdr=True, **g)
        r.render_async(s["cam_pos"], s["fov"])
        final = r.read_layer(0)
        bg, disk, blur = (r.read_layer(k) for k in (_lib.LAYER_BG, _lib.LAYER_DISK, _lib.LAYER_BLUR))
        over = float((G.combine(bg, disk, blur).max(axis=-1) > 1).mean())
        print(f"[grade] {math}: s > 1 on {over:.1%} of the pixels")
        assert over >= 0.40                                      # the test is about highlights
        h = G.hdr_plane(bg, disk, blur)
        _assert_bits(r.read_hdr(), h, f"HDR {g}")
        _assert_final(final, h, g, math)
        assert (final != plain).mean() > 0.3
        np.testing.assert_array_equal(r.read_final_u8(), Q.quantize8(final))
        np.testing.assert_array_equal(r.read_final_u16(), Q.quantize16(final))
        # no bloom: blur = 0
        r.render_async(s["cam_pos"], s["fov"], skip_bloom=True)
        final = r.read_layer(0)
        bg, disk = r.read_layer(_lib.LAYER_BG), r.read_layer(_lib.LAYER_DISK)
        assert not r.read_layer(_lib.LAYER_BLUR).any()
        _assert_bits(r.read_hdr(), G.hdr_plane(bg, disk), f"HDR without bloom {g}")
        _assert_final(final, G.hdr_plane(bg, disk), g, f"{math} without bloom")
        np.testing.assert_array_equal(r.read_final_u8(), Q.quantize8(final))
    r.close()


@pytest.mark.parametrize("math,size", [("strict", (1, 1)), ("strict", (5, 3)), ("strict", (71, 37)), ("hybrid", (71, 37))])
def test_odd_frame_shapes_store_their_own_u8_rows(math, size, hip_lib):
    """outputs "u8": the rows come from the grade kernel itself -- its 32-bit stores and, at these sizes, its scalar tail."""
    from bhr_amd import _lib
    w, h = size
    r, s = _default(math, w=w, h=h, outputs="u8")
    g = dict(tonemap="aces", transfer="srgb", exposure=1.0)
    r.set_grade(keep_hdr=True, **g)
    r.render_async(s["cam_pos"], s["fov"])
    u8 = r.read_final_u8()
    final = r.read_layer(0)
    np.testing.assert_array_equal(u8, Q.quantize8(final))
    bg, disk, blur = (r.read_layer(k) for k in (_lib.LAYER_BG, _lib.LAYER_DISK, _lib.LAYER_BLUR))
    _assert_bits(r.read_hdr(), G.hdr_plane(bg, disk, blur))
    _assert_final(final, G.hdr_plane(bg, disk, blur), g, f"{math} {w}x{h}")
    r.close()


# ---- 4. consumers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", ["f32", "u8"])
def test_every_consumer_takes_the_graded_frame(outputs, tmp_path, hip_lib):
    from bhr_amd.output import Y4MStream, jpeg_encode_device, jpeg_restart_interval, png_encode_device, read_y4m, rgb_to_yuv420
    r, s = _default("hybrid", outputs=outputs)
    r.render_async(s["cam_pos"], s["fov"])
    plain = r.read_final_u8()
    r.set_grade("aces", exposure=1.0, transfer="srgb")
    r.render_async(s["cam_pos"], s["fov"])
    u8, u16 = r.read_final_u8(), r.read_final_u16()
    assert (u8 != plain).mean() > 0.3
    np.testing.assert_array_equal(u8, Q.quantize8(r.read_layer(0)))
    np.testing.assert_array_equal(Q.png_read(png_encode_device(r))[0], u8)
    np.testing.assert_array_equal(Q.png_read(png_encode_device(r, bit_depth=16))[0], u16)
    assert jpeg_encode_device(r, 90) == jpeg_ref.encode(u8, 90, jpeg_restart_interval(r.width))
    path = str(tmp_path / "g.y4m")
    with Y4MStream(r, path, fps=24, slots=2) as st:
        st.submit()
        st.drain()
    _, planes = read_y4m(path)
    for got, want in zip(planes[0], rgb_to_yuv420(u8)):
        np.testing.assert_array_equal(got, want)
    r.close()


# ---- 5. frame slots --------------------------------------------------------------------------------------------------------
SLOT_GRADES = [dict(tonemap="aces", transfer="srgb", exposure=1.0)] * 2 + [dict(tonemap="reinhard", white=1.5, keep_hdr=True)] * 2 + [None] * 2


def _positions():
    s = scenes.SCENES["default"]
    return [[s["cam_pos"][0] + 0.3 * i, 0.2 * i, s["cam_pos"][2]] for i in range(6)]


@pytest.mark.parametrize("math", ["strict", "hybrid"])
def test_two_frame_slots_grade_like_one(math, hip_lib):
    one, s = _default(math, frame_slots=1, outputs="f32+u8")
    want = []
    for pos, g in zip(_positions(), SLOT_GRADES):
        one.set_grade(**(g or {}))
        one.render_async(pos, s["fov"])
        want.append((one.read_layer(0), one.read_final_u8(), one.read_hdr() if g and g.get("keep_hdr") else None))
    one.close()
    assert (want[0][0] != want[1][0]).any()
    for read_every in (1, 2):                       # 2: the even frames are still in flight when the next one is launched
        two, _ = _default(math, frame_slots=2, outputs="f32+u8")
        assert two.frame_slots == 2
        now = "off"
        for i, (pos, g) in enumerate(zip(_positions(), SLOT_GRADES)):
            if repr(g) != now:
                two.set_grade(**(g or {}))             # after frames 2 and 4, with frame i - 1 possibly in flight
                now = repr(g)
            two.render_async(pos, s["fov"])
            if (i + 1) % read_every == 0:
                _assert_bits(two.read_layer(0), want[i][0], f"frame {i} (reading every {read_every})")
                np.testing.assert_array_equal(two.read_final_u8(), want[i][1], err_msg=f"frame {i} u8")
                if want[i][2] is not None:
                    _assert_bits(two.read_hdr(), want[i][2], f"frame {i} HDR")
        two.close()


def test_a_shutter_frame_is_the_grade_of_its_resolved_layers(hip_lib):
    from bhr_amd import _lib
    r, s = _default("hybrid")
    g = dict(tonemap="aces", transfer="srgb", exposure=0.5, keep_hdr=True)
    r.set_grade(**g)
    pos = _positions()[:3]
    r.render_shutter_async(pos, s["fov"], [-0.01, 0.0, 0.01])
    final, hdr = r.read_layer(0), r.read_hdr()
    bg, disk, blur = (r.read_layer(k) for k in (_lib.LAYER_BG, _lib.LAYER_DISK, _lib.LAYER_BLUR))
    _assert_bits(hdr, G.hdr_plane(bg, disk, blur))
    _assert_final(final, hdr, g, "shutter")
    r.write_layer(_lib.LAYER_FINAL, np.zeros_like(final))
    r.grade_frame()
    _assert_bits(r.read_layer(0), final, "stand-alone grade of the shutter frame's layers")
    _assert_bits(r.read_hdr(), hdr)
    r.close()


# ---- 6. flare --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("math", ["strict", "hybrid"])
def test_the_flare_sits_in_front_of_the_grade(math, hip_lib):
    from bhr_amd import _lib
    r, s = _default(math, lens_flare=True)
    g = dict(tonemap="aces", transfer="srgb", exposure=1.0)
    r.set_grade(keep_hdr=True, **g)
    r.render_async(s["cam_pos"], s["fov"])
    final, hdr = r.read_layer(0), r.read_hdr()
    bg, disk, blur = (r.read_layer(k) for k in (_lib.LAYER_BG, _lib.LAYER_DISK, _lib.LAYER_BLUR))
    sm = G.combine(bg, disk, blur)
    # the flare term, from the device: FINAL = 0, then the stand-alone pass on the frame's DISK gives clip(0 + fl, 0, 1)
    r.write_layer(_lib.LAYER_FINAL, np.zeros_like(final))
    r.apply_lens_flare()
    fl = r.read_layer(0)
    assert fl.max() > 0.1 and fl.min() >= 0
    known = fl < 1
    want = np.maximum(sm + fl, F32(0))
    assert want.dtype == F32
    np.testing.assert_array_equal(_bits(hdr)[known], _bits(want)[known])
    assert (hdr[~known] >= (sm + F32(1))[~known]).all()
    share = float((~known).mean())
    print(f"[grade] {math}: the flare alone saturates {share:.1%} of the values")
    assert share <= 0.15
    assert (hdr > sm).mean() > 0.3                               # the flare is in the plane ...
    _assert_final(final, hdr, g, f"{math} flared")                # ... and FINAL is the grade of it
    r.close()


def test_a_dim_flared_frame_keeps_its_bits_in_the_hdr_plane(hip_lib):
    """Nothing clips on a frame whose layers stay below 0.1: the flared FINAL of the ungraded frame is the graded frame's HDR."""
    from bhr_amd import HipRenderer, _lib
    s = scenes.SCENES["default"]
    sky = scenes.analytic_skybox() * F32(0.1)
    tex = scenes.noisy_disk()
    tex[..., :3] *= F32(0.06)
    r = HipRenderer(64, 36, sky, tex, lens_flare=True, **s["kw"])
    r.render_async(s["cam_pos"], s["fov"])
    flared = r.read_layer(0)
    layers = [r.read_layer(k) for k in (_lib.LAYER_BG, _lib.LAYER_DISK, _lib.LAYER_BLUR)]
    assert max(a.max() for a in layers) <= 0.1 and flared.max() < 1.0
    assert (flared > G.combine(*layers)).mean() > 0.05          # there is a flare
    r.set_grade("clip", keep_hdr=True)
    r.render_async(s["cam_pos"], s["fov"])
    _assert_bits(r.read_hdr(), flared)
    _assert_bits(r.read_layer(0), flared)
    r.close()


# ---- 7. row blocks and refusals ----------------------------------------------------------------------------------------------
def test_a_row_block_grades_like_those_rows_of_the_frame(matrix, hip_lib):
    w, h, r0, r1 = 64, 36, 8, 24
    layers = layer_sets(w, h)["noise"]
    g = dict(tonemap="reinhard", transfer="srgb", exposure=0.75, keep_hdr=True)
    whole = _renderer(w, h)
    _inject(whole, layers)
    whole.set_grade(**g)
    whole.grade_frame()
    final, hdr, u16 = whole.read_layer(0), whole.read_hdr(), whole.read_final_u16()
    whole.set_dither("blue")
    d8 = whole.read_final_u8()
    _assert_final(final, hdr, g)
    block = _renderer(w, h, rows=(r0, r1))
    _inject(block, [a[r0:r1] for a in layers])
    block.set_grade(**g)
    block.grade_frame()
    _assert_bits(block.read_layer(0), final[r0:r1])
    _assert_bits(block.read_hdr(), hdr[r0:r1])
    np.testing.assert_array_equal(block.read_final_u16(), u16[r0:r1])
    block.set_dither("blue")
    np.testing.assert_array_equal(block.read_final_u8(), d8[r0:r1])
    whole.close()
    block.close()


def test_a_rendered_row_block_grades_like_those_rows(hip_lib):
    """bhr_render on a row-block context under a grade (no flare, no bloom halo: the block's own rows)."""
    whole, s = _default("strict")
    block, _ = _default("strict", rows=(8, 24))
    g = dict(tonemap="aces", transfer="srgb")
    for r in (whole, block):
        r.set_grade(**g)
        r.render_async(s["cam_pos"], s["fov"], skip_bloom=True)
    _assert_bits(block.read_layer(0), whole.read_layer(0)[8:24])
    whole.close()
    block.close()


BAD_GRADES = [(3, 0, 0.0, 2.5), (-1, 0, 0.0, 2.5), (0, 2, 0.0, 2.5), (0, -1, 0.0, 2.5), (0, 0, np.nan, 2.5), (0, 0, np.inf, 2.5),
              (0, 0, -np.inf, 2.5), (0, 0, 16.5, 2.5), (0, 0, -16.5, 2.5), (1, 0, 0.0, 0.0), (1, 0, 0.0, -1.0), (1, 0, 0.0, np.nan),
              (1, 0, 0.0, np.inf), (1, 0, 0.0, 65505.0)]


def test_refusals_leave_the_context_as_it_was(hip_lib):
    from bhr_amd import _lib
    r, s = _default("strict")
    r.render_async(s["cam_pos"], s["fov"])
    plain = r.read_layer(0)
    cam = r.camera_uniforms(s["cam_pos"], s["fov"])

    def refused():
        for op, tr, st, wh in BAD_GRADES:
            bad = _lib.Grade(op, tr, st, wh, 1)
            assert hip_lib.bhr_set_grade(r._ctx, C.byref(bad)) == _lib.BHR_ERR_INVALID, (op, tr, st, wh)
            assert b"bhr_set_grade" in hip_lib.bhr_last_error()
        assert hip_lib.bhr_set_grade(None, None) == _lib.BHR_ERR_INVALID
        zero = np.zeros((36, 64, 3), F32)
        assert hip_lib.bhr_write_layer(r._ctx, _lib.LAYER_HDR, _lib.fptr(zero)) == _lib.BHR_ERR_INVALID
        assert hip_lib.bhr_read_layer(r._ctx, 5, _lib.fptr(zero)) == _lib.BHR_ERR_INVALID

    refused()
    assert hip_lib.bhr_grade_frame(r._ctx) == _lib.BHR_ERR_STATE          # no grade is set
    assert hip_lib.bhr_grade_frame(None) == _lib.BHR_ERR_INVALID
    with pytest.raises(AssertionError):
        r.read_hdr()                                                      # BHR_ERR_STATE: no frame kept one
    for bad in (dict(tonemap="filmic"), dict(tonemap="clip", exposure=17.0), dict(tonemap="clip", white=0.0), dict(tonemap="clip", transfer="pq")):
        with pytest.raises(ValueError):
            r.set_grade(**bad)
    assert r.grade is None
    r.render_async(s["cam_pos"], s["fov"])
    _assert_bits(r.read_layer(0), plain, "after the refusals, no grade")
    # under a valid grade the refusals leave that grade in place
    r.set_grade("aces", exposure=1.0, transfer="srgb")
    r.render_async(s["cam_pos"], s["fov"])
    graded = r.read_layer(0)
    assert (graded != plain).any()
    with pytest.raises(AssertionError):
        r.read_hdr()                                                      # graded without keep_hdr
    refused()
    r.render_async(s["cam_pos"], s["fov"])
    _assert_bits(r.read_layer(0), graded, "after the refusals, under a grade")
    # the stand-alone passes stay the reference's functions
    r.bloom_only()
    _assert_bits(r.read_layer(0), plain, "bhr_bloom ignores the grade")
    # renders that store rows from inside their V passes
    ctxs = (C.c_void_p * 1)(r._ctx)
    out = np.empty((36, 64, 3), F32)
    for flags in (0, _lib.GATHER_U8):
        assert hip_lib.bhr_group_render(ctxs, 1, C.byref(cam), flags, _lib.fptr(out) if not flags else None) == _lib.BHR_ERR_INVALID
        assert b"grade" in hip_lib.bhr_last_error()
    assert hip_lib.bhr_tile_render(r._ctx, C.byref(cam), 0) == _lib.BHR_ERR_INVALID
    assert b"grade" in hip_lib.bhr_last_error()
    handles = _lib.TileHandles()
    assert hip_lib.bhr_tile_export(r._ctx, 0, C.byref(handles)) == _lib.BHR_ERR_INVALID
    assert b"grade" in hip_lib.bhr_last_error()
    r.render_async(s["cam_pos"], s["fov"])
    _assert_bits(r.read_layer(0), graded, "after the refused group and tile renders")
    r.set_grade(None)
    _lib.check(hip_lib.bhr_group_render(ctxs, 1, C.byref(cam), 0, _lib.fptr(out)))
    _assert_bits(out, plain, "bhr_group_render with the grade off again")
    r.close()


def test_tile_renders_refuse_a_grade_and_work_again_without(tmp_path, hip_lib):
    """Two processes, one tile each (tests/grade_tile_worker.py): linked, every rank's bhr_tile_render is refused while a grade
    is set and renders the frame of one context once it is off again."""
    shm = "bhr_test_" + uuid.uuid4().hex[:12]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "grade_tile_worker.py"), str(tmp_path), str(k), "2", shm], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for k in range(2)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for k, p in enumerate(procs):
        assert p.returncode == 0, f"rank {k}:\n{outs[k][-3000:]}"
    from bhr_amd import HipRenderer
    s = scenes.SCENES["default"]
    full = HipRenderer(640, 360, scenes.analytic_skybox(), scenes.noisy_disk(), frame_slots=1, **s["kw"])
    _assert_bits(np.load(os.path.join(tmp_path, "frame.npy")), full.render(s["cam_pos"], s["fov"]))
    full.close()
