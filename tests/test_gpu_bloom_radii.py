"""The split-f16 post-pass (csrc/bloom.hip) at every weight table count NT = 1 .. 12 (tests/bloom_radii.py: both ends of
every width range, QHD, 5K and the width classes of the V epilogue; heights 1, 7, 31, 33, 32 k + 5 and below the radius):
against the binary64 oracle and the exact f32 kernels on synthetic layers, the same bits for every forced tiling
(`bloom_tiles`), frames (fast, hybrid, supersampled) equal to the stand-alone pass over their own layers, row blocks equal
to one context, the fall-back to the exact kernels from W = 8850, and written disk layers the f16 halves cannot carry."""
import numpy as np
import pytest

import bloom_radii as B
from bhr_amd import scenes

pytestmark = pytest.mark.gpu

KW = dict(step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=0.0)
CAM, FOV = [6.0, 0.0, 0.5], 90.0
EMPTY_SKY, EMPTY_TEX = np.zeros((16, 32, 3), np.float32), np.zeros((32, 64, 4), np.float32)


def _scene():
    return scenes.analytic_skybox(128, 256), scenes.noisy_disk(256, 1024)


def _stand_alone(r, disk, bg, split, tiles=0):
    """(blur, final, u8) of bhr_bloom on the written layers, split-f16 (1) or exact f32 (0) kernels, `tiles` per wave"""
    from bhr_amd import _lib
    r.set_option("bloom_split", split)
    r.set_option("bloom_tiles", tiles)
    r.write_layer(_lib.LAYER_DISK, disk)
    r.write_layer(_lib.LAYER_BG, bg)
    r.bloom_only()
    out = r.read_layer(_lib.LAYER_BLUR), r.read_layer(_lib.LAYER_FINAL), r.read_final_u8()
    r.set_option("bloom_split", -1)
    r.set_option("bloom_tiles", 0)
    return out


def _combine(bg, disk, blur):
    """the V epilogue in f32: clip((bg + disk) + blur, 0, 1) and save_image's truncation"""
    final = np.clip((bg + disk) + blur, np.float32(0), np.float32(1)).astype(np.float32)
    return final, (final * np.float32(255)).astype(np.uint8)


def _errors(got, ref):
    d = np.abs(got.astype(np.float64) - ref)
    return d.max(), np.sqrt(np.mean(d ** 2, axis=(0, 1)))


@pytest.mark.parametrize("shape", B.shapes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_stand_alone_pass_against_binary64_and_every_tiling(shape, oracle, hip_lib):
    """Synthetic layers at one shape: the split blur within 5e-6 (max) and 1e-6 (per-channel RMSE) of binary64 and 3e-6
    of the exact kernels; final and u8 the f32 combine of the pass's own blur, bit for bit; every forced tiling (1 .. 8
    tiles per wave, T = 5 and T = 8) the same bits as the planned one"""
    from bhr_amd import HipRenderer
    W, H = shape
    nt = B.split_nt(W)
    disk, bg = B.synthetic_layers(W, H, seed=W * 1000 + H)
    r = HipRenderer(W, H, EMPTY_SKY, EMPTY_TEX, math="fast", frame_slots=1)
    split = _stand_alone(r, disk, bg, 1)
    exact = _stand_alone(r, disk, bg, 0)
    tiled = {t: _stand_alone(r, disk, bg, 1, tiles=t) for t in range(1, 9)}
    r.close()
    for name, (blur, final, u8) in (("split", split), ("exact", exact)):
        want_final, want_u8 = _combine(bg, disk, blur)
        np.testing.assert_array_equal(final, want_final, err_msg=f"{name} final")
        np.testing.assert_array_equal(u8, want_u8, err_msg=f"{name} u8")
    if nt == 1:                                             # R = 0: one tap of weight 1
        np.testing.assert_array_equal(exact[0], disk)
    ref, _ = oracle.OracleRenderer(W, H, EMPTY_SKY, EMPTY_TEX, fast="f64").bloom(disk.transpose(1, 0, 2))
    ref = ref.transpose(1, 0, 2).astype(np.float64)
    mx, rmse = _errors(split[0], ref)
    mx_x, rmse_x = _errors(exact[0], ref)
    d = np.abs(split[0] - exact[0]).max()
    print(f"\n[bloom radii] {W}x{H} NT {nt}: split vs binary64 max {mx:.3g} RMSE {rmse}; exact vs binary64 max {mx_x:.3g} "
          f"RMSE {rmse_x}; split vs exact max {d:.3g}")
    assert mx <= 5e-6 and (rmse <= 1e-6).all(), (mx, rmse)
    assert d <= 3e-6, d
    for t, got in tiled.items():
        for k, name in enumerate(("blur", "final", "u8")):
            np.testing.assert_array_equal(got[k], split[k], err_msg=f"bloom_tiles {t}: {name}")


FRAMES = [(1, 1), (40, 3), (49, 7), (844, 37), (1649, 33), (2449, 31), (2560, 37), (4049, 7), (4064, 69), (5120, 37),
          (6449, 33), (6464, 31), (8049, 37), (8849, 69)]


@pytest.mark.parametrize("shape", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_post_pass_equals_the_stand_alone_pass(shape, hip_lib):
    """Fast and hybrid frames: the post-pass fed by the march (packed H input and bg + disk written by its epilogue) gives
    the bits the stand-alone split pass gives on the frame's own read-back layers -- blur, final and the V pass's u8 rows"""
    from bhr_amd import HipRenderer, _lib
    W, H = shape
    sky, tex = _scene()
    for math in ("fast", "hybrid"):
        r = HipRenderer(W, H, sky, tex, math=math, frame_slots=1, outputs="f32+blur+u8", **KW)
        r.render_async(CAM, FOV)
        bg, disk = r.read_layer(_lib.LAYER_BG), r.read_layer(_lib.LAYER_DISK)
        blur, final, u8 = r.read_layer(_lib.LAYER_BLUR), r.read_layer(_lib.LAYER_FINAL), r.read_final_u8()
        if W >= 40:
            assert disk.max() > 0.05, (math, disk.max())
        np.testing.assert_array_equal(u8, _combine(bg, disk, blur)[1], err_msg=math)
        got = _stand_alone(r, disk, bg, -1)                      # the context's own arithmetic: split
        r.close()
        np.testing.assert_array_equal(blur, got[0], err_msg=f"{math} blur")
        np.testing.assert_array_equal(final, got[1], err_msg=f"{math} final")


@pytest.mark.parametrize("k,shape", [(2, (160, 90)), (2, (203, 37)), (4, (96, 54)), (4, (40, 3))])
def test_supersampled_frame_post_pass_equals_the_stand_alone_pass(k, shape, hip_lib):
    """A supersampled hybrid march writes the packed H input and bg + disk of the RESOLVED layers: same bits as the
    stand-alone split pass over them"""
    from bhr_amd import HipRenderer, _lib
    W, H = shape
    sky, tex = _scene()
    r = HipRenderer(W, H, sky, tex, math="hybrid", frame_slots=1, outputs="f32+blur+u8", supersample=k, **KW)
    r.render_async(CAM, FOV)
    bg, disk = r.read_layer(_lib.LAYER_BG), r.read_layer(_lib.LAYER_DISK)
    blur, final, u8 = r.read_layer(_lib.LAYER_BLUR), r.read_layer(_lib.LAYER_FINAL), r.read_final_u8()
    r.close()
    assert disk.max() > 0.05
    np.testing.assert_array_equal(u8, _combine(bg, disk, blur)[1])
    p = HipRenderer(W, H, EMPTY_SKY, EMPTY_TEX, math="hybrid", frame_slots=1)
    got = _stand_alone(p, disk, bg, -1)
    p.close()
    np.testing.assert_array_equal(blur, got[0])
    np.testing.assert_array_equal(final, got[1])


# (W, H, cuts): NT 1, 5, 8, 12; blocks thinner than the halo 16 (NT - 1) rows, cuts off multiples of 4, 16 and 32
ROW_BLOCKS = [(40, 50, [0, 3, 17, 20, 50]), (2560, 133, [0, 37, 41, 100, 133]), (4850, 165, [0, 5, 90, 150, 165]),
              (8849, 229, [0, 61, 64, 200, 229])]


@pytest.mark.parametrize("W,H,cuts", ROW_BLOCKS, ids=lambda v: str(v) if not isinstance(v, list) else "cuts")
def test_row_blocks_equal_one_context_at_every_radius_class(W, H, cuts, hip_lib):
    from bhr_amd import HipRenderer, multigpu
    sky, tex = _scene()
    full = HipRenderer(W, H, sky, tex, math="fast", frame_slots=1, **KW)
    ref = full.render(CAM, FOV)
    ref_u8 = full.read_final_u8()
    full.close()
    assert ref.max() > 0.05
    tiles = [HipRenderer(W, H, sky, tex, rows=(cuts[k], cuts[k + 1]), math="fast", frame_slots=1, **KW) for k in range(len(cuts) - 1)]
    for sched in ("serial", "pipelined"):
        multigpu.group_render(tiles, CAM, FOV, gather="peer", schedule=sched)
        np.testing.assert_array_equal(multigpu.read_gathered(tiles), ref, err_msg=f"{W}x{H} {sched} peer")
        multigpu.group_render(tiles, CAM, FOV, gather="peer_u8", schedule=sched)
        np.testing.assert_array_equal(multigpu.read_gathered_u8(tiles), ref_u8, err_msg=f"{W}x{H} {sched} peer_u8")
        np.testing.assert_array_equal(multigpu.group_render(tiles, CAM, FOV, gather="host", schedule=sched), ref,
                                      err_msg=f"{W}x{H} {sched} host")
    for t in tiles:
        t.close()


def test_split_path_ends_at_8849(hip_lib):
    """W = 8849 (R = 176, NT = 12): the split kernels run.  W = 8850: the exact kernels, whatever `bloom_split` asks for --
    frames and the stand-alone pass"""
    from bhr_amd import HipRenderer, _lib
    sky, tex = _scene()
    H = 37
    for W in (B.SPLIT_W_MAX, B.SPLIT_W_MAX + 1):
        r = HipRenderer(W, H, sky, tex, math="fast", frame_slots=1, outputs="f32+blur", **KW)
        blur = {}
        for split in (-1, 1, 0):
            r.set_option("bloom_split", split)
            r.render_async(CAM, FOV)
            blur[split] = r.read_layer(_lib.LAYER_BLUR)
        disk, bg = r.read_layer(_lib.LAYER_DISK), r.read_layer(_lib.LAYER_BG)
        alone = {split: _stand_alone(r, disk, bg, split)[0] for split in (1, 0)}
        r.close()
        assert blur[0].max() > 0.01
        np.testing.assert_array_equal(blur[-1], blur[1])
        np.testing.assert_array_equal(alone[0], blur[0])
        if W == B.SPLIT_W_MAX:
            assert not np.array_equal(blur[1], blur[0])
            assert np.abs(blur[1] - blur[0]).max() <= 3e-6
            np.testing.assert_array_equal(alone[1], blur[1])
        else:
            np.testing.assert_array_equal(blur[1], blur[0])
            np.testing.assert_array_equal(alone[1], blur[0])


def test_written_disk_layers_the_split_halves_cannot_carry(oracle, hip_lib):
    """The stand-alone pass is one function of its input under every arithmetic: a written disk value above 3.99 (what two
    f16 halves scaled by 2^14 carry) sends the pass to the exact kernels, so hybrid and strict contexts agree bit for bit;
    negative and non-finite values (the folded `lum > 0` test, render.py:3036-3041, holds for non-negative layers only)
    are refused and leave the layer as it was"""
    from bhr_amd import HipRenderer, _lib
    W, H = 203, 37
    disk, bg = B.synthetic_layers(W, H, seed=6)
    hot = disk.copy()
    hot[20, 100] = 5.0
    hot[3, 7, 1] = 4.5
    edge = disk.copy()
    edge[11, 50] = 3.99                                       # the largest value the halves carry: still the split kernels
    ctx = {m: HipRenderer(W, H, EMPTY_SKY, EMPTY_TEX, math=m, frame_slots=1) for m in ("hybrid", "strict")}
    out = {m: _stand_alone(r, hot, bg, -1) for m, r in ctx.items()}
    for k in range(3):
        np.testing.assert_array_equal(out["hybrid"][k], out["strict"][k])
    ref, _ = oracle.OracleRenderer(W, H, EMPTY_SKY, EMPTY_TEX, fast="f64").bloom(hot.transpose(1, 0, 2))
    mx, _ = _errors(out["hybrid"][0], ref.transpose(1, 0, 2))
    assert mx <= 5 * 5e-6, mx
    # a layer in range again: the split kernels again, within the usual distance of the exact ones
    h = ctx["hybrid"]
    for layer in (disk, edge):
        split, exact = _stand_alone(h, layer, bg, -1), _stand_alone(ctx["strict"], layer, bg, -1)
        assert not np.array_equal(split[0], exact[0])
        assert np.abs(split[0] - exact[0]).max() <= 4 * 3e-6
    np.testing.assert_array_equal(_stand_alone(h, hot, bg, -1)[0], out["strict"][0])
    # refused: a negative-luminance pixel, a negative channel of a bright one, NaN, infinities
    _stand_alone(h, disk, bg, -1)
    before = h.read_layer(_lib.LAYER_DISK)
    for bad in ((0.3, -0.5, 0.0), (0.9, 0.9, -1e-30), (np.nan, 0.0, 0.0), (np.inf, 0.0, 0.0), (0.0, -np.inf, 0.0)):
        x = disk.copy()
        x[17, 33] = bad
        with pytest.raises(ValueError):
            h.write_layer(_lib.LAYER_DISK, x)
        np.testing.assert_array_equal(h.read_layer(_lib.LAYER_DISK), before)
    for r in ctx.values():
        r.close()
