"""The promise of math="hybrid" (csrc/hybrid.hip), checked pixel by pixel: every pixel whose ray has its orbit's impact
parameter b in [b_c - lo, b_c + hi] (an outgoing ray of a camera outside 3 r_s excepted), or an orbital plane within
PLANE_SIN of the disk plane, lies in a tile of the strict list.  The library's lists (both classification paths) are held
against the binary64 restatement of tests/hybrid_band.py -- itself pinned to the oracle's rays by tests/test_hybrid_band.py:

  (a) the partitioned launch order is a permutation of the tiles, its strict head as long as hybrid_info says;
  (b) soundness: no pixel that must march strict lies in a fast tile;
  (c) the library's tile flags equal the restated rule's, but for tiles whose closest comparison lies within 1e-6 of its
      threshold (counted and printed: none are expected).

Views: the BASELINE ones (fhd, 4k tilt 25 lod_radius, 8k step 0.05), a sweep of the ring tiles' span across tile_pad's
0.1 / 0.2 r_s regimes, cameras on both sides of the far-camera switch at 3 r_s (turned away from the hole, too: a look-at
camera has no outgoing rays), telephoto far cameras, the in-plane views, a coarse step, row blocks and a camera path."""
import ctypes as C

import numpy as np
import pytest

import hybrid_band as hb

pytestmark = pytest.mark.gpu

KW = dict(step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=0.0, anti_alias="disabled")
POV, FOV = [6.0, 0.0, 0.5], 90.0
TIE = 1e-6
CHUNK_PX = 1 << 21                     # pixels per slice of the per-pixel geometry (an 8k frame in 16 slices)


def _scene():
    from bhr_amd import scenes
    return scenes.analytic_skybox(64, 128), scenes.noisy_disk(32, 128)


def _uniforms(r, cam_pos, fov, look=0.0):
    u = r.camera_uniforms(cam_pos, fov)
    if look:                                       # turned away from the hole about the view's up axis
        c = hb.uniforms(cam_pos, fov, r.width, r.height, look)
        u.forward[:], u.right[:] = list(c.forward), list(c.right)
    return u


def _march(r, u):
    """One hybrid march (no bloom) from explicit uniforms."""
    from bhr_amd import _lib
    _lib.check(r._lib.bhr_render(r._ctx, C.byref(u), r._flags(False, True, False, "hybrid")))
    r.sync()


def _need_tiles(r, u, lo, hi):
    """Per tile of r's row block: holds a pixel that must march strict (must_be_strict over every pixel, in slices)."""
    cam = hb.cam_from_uniforms(u)
    W, H, row0, row1 = r.width, r.height, r.row0, r.row1
    need = np.zeros(((W + 7) // 8) * ((row1 - row0 + 7) // 8), bool)
    step = max(8, CHUNK_PX // W // 8 * 8)
    for y0 in range(row0, row1, step):
        y1 = min(row1, y0 + step)
        geo = hb.pixel_geometry(cam, W, H, y0, y1, r.disk_tilt)
        m = hb.must_be_strict(geo, lo, hi)
        need[hb.tile_of_pixels(W, row0, y0, y1)[m]] = True
    return need


def _worst_missed(r, u, lo, hi, lib_flags, aux):
    """The missed pixel deepest inside the band: its b - b_c, tile, tile span (for the failure message)."""
    cam = hb.cam_from_uniforms(u)
    W, H, row0, row1 = r.width, r.height, r.row0, r.row1
    best = None
    step = max(8, CHUNK_PX // W // 8 * 8)
    for y0 in range(row0, row1, step):
        y1 = min(row1, y0 + step)
        geo = hb.pixel_geometry(cam, W, H, y0, y1, r.disk_tilt)
        t = hb.tile_of_pixels(W, row0, y0, y1)
        miss = hb.must_be_strict(geo, lo, hi) & ~lib_flags[t]
        if not miss.any():
            continue
        depth = np.where(miss, np.minimum(geo["b"] - (hb.B_CRIT - lo), hb.B_CRIT + hi - geo["b"]), -np.inf)
        y, x = np.unravel_index(int(np.argmax(depth)), depth.shape)
        if best is None or depth[y, x] > best[0]:
            tile = int(t[y, x])
            best = (float(depth[y, x]), dict(pixel=(int(x), int(y0 + y)), b_minus_bc=float(geo["b"][y, x] - hb.B_CRIT),
                                             s=float(geo["s"][y, x]), tile=tile, tile_span=float(aux["span"].ravel()[tile])))
    return best[1] if best else None


def _check(r, u, tag, need=None, soundness=True, pad_f=hb.PAD_F):
    """(a), (b), (c) for the last hybrid march of r from uniforms u.  Returns need (reusable for the same view)."""
    info, order = r.hybrid_info(), r.hybrid_launch_order()
    n, ns = info["tiles"], info["strict_tiles"]
    tiles_x, tiles_y = (r.width + 7) // 8, (r.row1 - r.row0 + 7) // 8
    # (a)
    assert n == tiles_x * tiles_y and len(order) == n, (tag, n, len(order))
    assert np.array_equal(np.sort(order), np.arange(n)), f"{tag}: the launch order is not a permutation of the tiles"
    lib_flags = np.zeros(n, bool)
    lib_flags[order[:ns]] = True
    lo, hi = hb.effective_band(r.step_size)
    assert abs(info["band_below"] - lo) <= 1e-12 and abs(info["band_above"] - hi) <= 1e-12, (tag, info, lo, hi)
    lo, hi = info["band_below"], info["band_above"]
    # (c)
    flags, margin, aux = hb.tile_flags(hb.cam_from_uniforms(u), r.width, r.height, r.row0, r.row1 - r.row0, r.disk_tilt, lo, hi, pad_f)
    flags, margin = flags.ravel(), margin.ravel()
    diff = flags != lib_flags
    ties = int((diff & (margin < TIE)).sum())
    print(f"\n[{tag}] strict tiles {ns} of {n}; tiles that differ within {TIE} of a threshold: {ties}")
    bad = np.nonzero(diff & (margin >= TIE))[0]
    assert bad.size == 0, (f"{tag}: {bad.size} tiles classified unlike classify()'s restatement (library strict "
                           f"{int(lib_flags[bad].sum())}); first {int(bad[0])}: span {aux['span'].ravel()[bad[0]]:.4g}, "
                           f"b in [{aux['bmin'].ravel()[bad[0]]:.6f}, {aux['bmax'].ravel()[bad[0]]:.6f}], margin {margin[bad[0]]:.3g}")
    # (b)
    if soundness:
        if need is None:
            need = _need_tiles(r, u, lo, hi)
        if (need & ~lib_flags).any():
            pytest.fail(f"{tag}: {int((need & ~lib_flags).sum())} fast tiles hold pixels that must march strict; worst "
                        f"{_worst_missed(r, u, lo, hi, lib_flags, aux)}")
    return need


def _run_view(W, H, cam_pos, fov, tag, look=0.0, rows=None, pads=(0.0, 1.0), **kw):
    """(a)-(c) under both classification paths at the default pad, (c) at the other pads; one context.  Returns the
    hybrid_info of the default-pad march."""
    from bhr_amd import HipRenderer
    sky, tex = _scene()
    k = dict(KW, **kw)
    r = HipRenderer(W, H, sky, tex, rows=rows, math="hybrid", frame_slots=1, **k)
    try:
        u = _uniforms(r, cam_pos, fov, look)
        need = None
        for where in (1, 0):
            r.set_option("hybrid_classify", where)
            _march(r, u)
            need = _check(r, u, f"{tag} classify {where}", need)
            if where == 1:
                info = r.hybrid_info()
        r.set_option("hybrid_classify", 1)
        for pad in pads:
            r.set_option("hybrid_pad", pad)
            _march(r, u)
            _check(r, u, f"{tag} pad {pad}", soundness=False, pad_f=pad)
        r.set_option("hybrid_pad", hb.PAD_F)
        return info
    finally:
        r.close()


@pytest.mark.parametrize("name", ["fhd", "4k", "8k"])
def test_band_baseline_views(name, hip_lib):
    if name == "fhd":
        info = _run_view(1920, 1080, POV, FOV, name)
    elif name == "4k":
        info = _run_view(3840, 2160, POV, FOV, name, disk_tilt=25.0, anti_alias="lod_radius")
    else:
        info = _run_view(7680, 4320, POV, FOV, name, step_size=0.05)
    assert 0 < info["strict_tiles"] < 0.15 * info["tiles"], info


# the ring tiles' span of b at the default pov goes with 1 / H: ~0.04 r_s at 2160 rows, 0.08 at fhd, 0.16 at 540, 0.4 at 216:
# tile_pad's three regimes (share pad_f of the span, the linear ramp, the whole span)
SWEEP = [(h * 16 // 9, h) for h in (2160, 1080, 720, 540, 432, 360, 288, 216)] + [(1366, 766)]


@pytest.mark.parametrize("W,H", SWEEP, ids=[f"{w}x{h}" for w, h in SWEEP])
def test_band_tile_span_sweep(W, H, hip_lib):
    _run_view(W, H, POV, FOV, f"sweep {W}x{H}")


# (cam, fov, look_away_deg): both sides of the far-camera switch at |cam| = 3; turned views hold outgoing rays
NEAR = [([r, 0.0, 0.1], 100.0, look) for r in (1.3, 1.6, 2.6, 2.95, 3.05) for look in (0.0, 70.0)] + \
       [([r * 0.6, r * 0.8, 0.2], 100.0, 95.0) for r in (2.95, 3.05)]


@pytest.mark.parametrize("cam,fov,look", NEAR, ids=[f"r{np.linalg.norm(c):.2f}-look{lk:.0f}" for c, _, lk in NEAR])
def test_band_cameras_near_the_hole(cam, fov, look, hip_lib):
    _run_view(640, 360, cam, fov, f"cam {cam} look {look}", look=look)


@pytest.mark.parametrize("r0,fov", [(13.0, 30.0), (30.0, 25.0), (60.0, 20.0)])
def test_band_telephoto_far_cameras(r0, fov, hip_lib):
    info = _run_view(640, 360, [r0 * 0.96, r0 * 0.25, r0 * 0.1], fov, f"far {r0}")
    assert info["strict_tiles"] > 0


@pytest.mark.parametrize("cam,tilt", [([6.0, 0.0, 0.0], 0.0), ([-10.27977657706746, 3.4882456957730086, 5.652677980932753], 58.41173651690485)])
def test_band_in_plane_views(cam, tilt, hip_lib):
    _run_view(640, 360, cam, 100.0, f"in-plane {cam}", r_max=25.0, r_disk_inner=2.35, r_disk_outer=20.0, disk_tilt=tilt)


def test_band_coarse_step_widens_the_band(hip_lib):
    info = _run_view(960, 540, POV, FOV, "step 0.3", step_size=0.3)
    assert abs(info["band_below"] / hb.BAND_LO - 3) < 1e-6 and abs(info["band_above"] / hb.BAND_HI - 3) < 1e-6, info


@pytest.mark.parametrize("rows", [(97, 251), (96, 256)])
def test_band_row_blocks(rows, hip_lib):
    _run_view(640, 360, POV, FOV, f"rows {rows}", rows=rows)


def test_band_camera_path_on_one_context(hip_lib):
    """24 frames of an orbit at constant radius (the cached lists serve every frame after the first), then a dolly of 1e-6
    (inside same_view's tolerance: the lists stay) and one of 1e-3 (a new classification): (b) on every frame against its
    own camera, (c) wherever the lists were made for that very camera."""
    from bhr_amd import HipRenderer
    from bhr_amd.camera import orbit_position
    sky, tex = _scene()
    W, H = 640, 360
    r = HipRenderer(W, H, sky, tex, math="hybrid", **KW)
    path = [orbit_position(POV, f, 24, 360.0) for f in range(24)]
    path += [[POV[0] + 1e-6, POV[1], POV[2]], [POV[0] + 1e-3, POV[1], POV[2]]]
    orders = []
    try:
        for k, cam in enumerate(path):
            u = _uniforms(r, cam, FOV)
            _march(r, u)
            orders.append(r.hybrid_launch_order())
            if k == 0 or k == len(path) - 1:               # lists made for this very camera: (a)-(c)
                _check(r, u, f"path frame {k}")
            else:                                          # lists cached from frame 0: (b) against this frame's camera
                lo, hi = hb.effective_band(r.step_size)
                need = _need_tiles(r, u, lo, hi)
                lib_flags = np.zeros(len(orders[-1]), bool)
                lib_flags[orders[-1][:r.hybrid_info()["strict_tiles"]]] = True
                assert not (need & ~lib_flags).any(), (k, cam, int((need & ~lib_flags).sum()))
    finally:
        r.close()
    assert all(np.array_equal(o, orders[0]) for o in orders[1:25])          # the orbit and the tiny dolly reuse the lists
