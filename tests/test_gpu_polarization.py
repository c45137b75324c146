"""Polarisation on the device (bhr_set_polarization; include/bhr.h states the model, DESIGN.md 4 "Polarisation"): the Stokes
planes of a frame from the ray map against the binary64 reference (tests/polar_ref.py) fed the DEVICE's own records, the order
and weights of several crossings, the I plane, the cell grid, frame slots, the overflow list, that nothing existing moves, the
refusals, and the drivers end to end.

The bar.  TOL = 4 x 1.10e-6 = 4.39e-6 on Q / I and U / I: the largest |float32 reference - float64 reference| over the first
records of the single-crossing pixels of every view, field and size of this file with Pi_0 = 1 is 1.10e-6 (measured on the host on
records of a plain binary64 march of these views, polar_ref.march_records: default 0.82e-6, tilt 1.10e-6, close 1.06e-6; the
largest is the tilted view's at 64 x 36; test_single_crossing_pixels prints the same figure on the device's own records); four times
it covers another operation order and the device's libm.  No pixel class dominates: the views have no nearly radial ray inside
the disk's image.

Scenes: scenes.analytic_skybox() and scenes.noisy_disk().  Views: the default (6, 0, 0.5) at fov 90; the same over a disk tilted
by 25 degrees with anti-aliasing (a map with differentials); a close camera at (2.5, 2, 1.2).  The condition on a view: at least
85 % of its pixels with a crossing have one crossing, at every size that has crossings.  On the host march the shares at 9 x 7 /
64 x 36 / 97 x 55 are: default 0.868 (33 of 38) / 0.912 / 0.913, tilt 0.875 (35 of 40) / 0.909 / 0.910, close 0.929 (26 of 28) /
0.908 / 0.906.  The close camera of the other ray-map tests, (3, 2, 0.3), has 0.756 / 0.847 / 0.842 and (3, 2, 1) 0.842 at 9 x 7,
so neither serves.  The 1 x 1 frame of a camera that looks at the hole has one ray, the radial one: it crosses no disk in any
view, so that size has no share and nothing to compare; it checks that the pass runs on one pixel and stores zeros."""
import ctypes as C
import functools

import numpy as np
import pytest

import polar_ref as R

pytestmark = pytest.mark.gpu

FOV = 90.0
TOL = 4.39e-6          # 4 x 1.10e-6, the float32 reference's largest distance from the float64 one (the head of this file)
VIEWS = {"default": ((6.0, 0.0, 0.5), {}), "tilt": ((6.0, 0.0, 0.5), dict(disk_tilt=25.0, anti_alias="lod_radius")),
         "close": ((2.5, 2.0, 1.2), {})}
FIELDS = {"toroidal": "toroidal", "vertical": "vertical", "radial": "radial", "mixed": (0.3, 0.8, 0.5)}
SIZES = ((64, 36), (97, 55), (9, 7), (1, 1))
LUMA = np.array(R.LUMA)


@functools.lru_cache(maxsize=None)
def _scene():
    from bhr_amd import scenes
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    sky.setflags(write=False)
    tex.setflags(write=False)
    return sky, tex


def _mk(W=64, H=36, tex=None, **kw):
    from bhr_amd import HipRenderer
    sky, noisy = _scene()
    return HipRenderer(W, H, sky, noisy if tex is None else tex, math="strict", **kw)


def _vector(field):
    from bhr_amd import polarization
    return polarization.field_vector(field)


def _predict(r, pos, passes, field, frac, dtype=np.float64):
    """(a, b, ok, live): the reference per record of the device's own map, and which records a pixel has."""
    cam = R.camera_dict(r.camera_uniforms(list(pos), FOV, 0))
    a, b, ok = R.frame_stokes(cam, r.width, r.height, passes["hits"], r.disk_tilt, _vector(field), frac, r.r_disk_inner, r.r_disk_outer, dtype)
    K = passes["hits"].shape[0]
    live = np.arange(K)[:, None, None] < np.minimum(passes["crossings"], K)[None]
    return a, b, ok, live


def _frame(r, field, frac, t=0.0, cell=16):
    r.set_polarization(field, frac, cell)
    r.render_from_ray_map_async(t_offset=t, skip_bloom=True)
    return r.stokes()


def _ratio(S):
    I, Q, U = S.astype(np.float64)
    lit = I > 1e-4 * max(float(I.max()), 1e-30)
    safe = np.where(lit, I, 1.0)
    return Q / safe, U / safe, lit


@pytest.mark.parametrize("view", list(VIEWS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_crossing_pixels(size, view):
    W, H = size
    pos, kw = VIEWS[view]
    r = _mk(W, H, **kw)
    try:
        r.build_ray_map(pos, FOV)
        assert r.ray_map_info()["diff"] == (1 if kw else 0)
        p = r.ray_map_passes()
        cnt = p["crossings"]
        one, any_ = cnt == 1, cnt >= 1
        share = one.sum() / max(any_.sum(), 1)
        print(f"{view} {W}x{H}: {any_.sum()} pixels with a crossing, {one.sum()} with one ({share:.3f}), {(cnt == 2).sum()} with two, {(cnt > 2).sum()} with more")
        # the one ray of a 1 x 1 frame is radial and crosses no disk (the head of this file): no share, zeros in the planes
        empty = (W, H) == (1, 1)
        if empty:
            assert not any_.any()
        else:
            # the condition: the compared class is at least 85 % of the pixels with a crossing
            assert share >= 0.85
        worst = own = 0.0
        for name, field in FIELDS.items():
            for t, frac in ((0.0, 0.7), (7.3, 1.0)):
                S = _frame(r, field, frac, t)
                assert np.isfinite(S).all()
                if empty:
                    assert not S.any()
                    continue
                a, b, ok, live = _predict(r, pos, p, field, frac)
                a32, b32, _, _ = _predict(r, pos, p, field, frac, np.float32)
                q, u, lit = _ratio(S)
                m = one & lit
                assert m.any()
                dq, du = np.abs(q - a[0])[m].max(), np.abs(u - b[0])[m].max()
                own = max(own, np.abs(a32 - a)[0][m].max(), np.abs(b32 - b)[0][m].max())
                worst = max(worst, dq, du)
                assert dq <= TOL and du <= TOL, f"{view} {W}x{H} {name} t {t} Pi_0 {frac}: |d Q/I| {dq:.3e}, |d U/I| {du:.3e} over {TOL:.2e}"
                assert (np.hypot(S[1], S[2]) <= frac * S[0] * (1 + 1e-5) + 1e-12).all()        # Q^2 + U^2 <= (Pi_0 I)^2
                if name == "toroidal" and W * H >= 64 * 36:
                    assert np.hypot(q, u)[m].max() > 0.2 * frac                                # there is something to compare
        print(f"  largest device difference {worst:.3e}; float32 reference on the same records {own:.3e}; bar {TOL:.2e}")
    finally:
        r.close()


def test_zero_fraction_gives_no_q_and_u():
    pos, kw = VIEWS["default"]
    r = _mk()
    try:
        r.build_ray_map(pos, FOV)
        S0 = _frame(r, "toroidal", 0.0)
        S1 = _frame(r, "toroidal", 0.7)
        assert (S0[1] == 0).all() and (S0[2] == 0).all() and np.array_equal(S0[0], S1[0]) and S1[1].any() and S1[2].any()
    finally:
        r.close()


@pytest.mark.parametrize("view", ["default", "close"])
def test_opaque_texture_pins_front_to_back_order(view):
    """Under an opaque uniform texture the first crossing hides the rest: every pixel is its FIRST record's prediction."""
    pos, kw = VIEWS[view]
    _, noisy = _scene()
    r = _mk(97, 55, tex=np.ones_like(noisy), **kw)
    try:
        r.build_ray_map(pos, FOV)
        p = r.ray_map_passes()
        assert (p["crossings"] >= 2).sum() > 100
        for field in ("toroidal", (0.3, 0.8, 0.5)):
            S = _frame(r, field, 1.0)
            a, b, ok, live = _predict(r, pos, p, field, 1.0)
            q, u, lit = _ratio(S)
            m = live[0] & ok[0] & lit
            assert (m & (p["crossings"] >= 2)).sum() > 100
            assert np.abs(q - a[0])[m].max() <= TOL and np.abs(u - b[0])[m].max() <= TOL
            # ... and it is NOT the second record's: the test can tell the orders apart
            two = m & live[1] & ok[1]
            assert (np.abs(q - a[1])[two] > 100 * TOL).sum() > 0.5 * two.sum()
    finally:
        r.close()


@pytest.mark.parametrize("view", ["default", "tilt", "close"])
def test_two_crossing_weights(view):
    """The weights c_k do not depend on the field: solved from I and Q under field A, they predict U under A and Q, U under B.
    The bar of a prediction: the device's Q_A is good to TOL I, so c_1 = (Q_A - a_2 I) / (a_1 - a_2) to TOL I / |a_1 - a_2|, and a
    predicted x_1 c_1 + x_2 c_2 to TOL I |x_1 - x_2| / |a_1 - a_2|; the device's own value of it to TOL I."""
    pos, kw = VIEWS[view]
    r = _mk(97, 55, **kw)
    try:
        r.build_ray_map(pos, FOV)
        p = r.ray_map_passes()
        two = p["crossings"] == 2
        A, B = (0.3, 0.8, 0.5), "vertical"
        SA, SB = _frame(r, A, 1.0, 7.3).astype(np.float64), _frame(r, B, 1.0, 7.3).astype(np.float64)
        assert np.array_equal(SA[0], SB[0])                      # I does not depend on the field
        aA, bA, okA, _ = _predict(r, pos, p, A, 1.0)
        aB, bB, okB, _ = _predict(r, pos, p, B, 1.0)
        I = SA[0]
        usable = two & okA[0] & okA[1] & okB[0] & okB[1] & (I > 1e-4 * I.max())
        m = usable & (np.abs(aA[0] - aA[1]) > 0.05)
        print(f"{view}: {two.sum()} two-crossing pixels, {usable.sum()} lit, {m.sum()} with |a_1 - a_2| > 0.05")
        assert m.sum() >= 0.5 * two.sum() and m.sum() > 50
        gap = np.where(m, np.abs(aA[0] - aA[1]), 1.0)
        c1 = (SA[1] - aA[1] * I) / np.where(m, aA[0] - aA[1], 1.0)
        c2 = I - c1
        assert (c1[m] > -TOL * I[m] / gap[m]).all() and (c2[m] > -TOL * I[m] / gap[m]).all()
        assert (c2[m] > 1e-3 * I[m]).sum() > 0.5 * m.sum()       # the second crossing does weigh in
        for name, got, x in (("U_A", SA[2], bA), ("Q_B", SB[1], aB), ("U_B", SB[2], bB)):
            want = c1 * x[0] + c2 * x[1]
            bar = TOL * I * (1.0 + np.abs(x[0] - x[1]) / gap)
            excess = (np.abs(got - want)[m] / bar[m]).max()
            print(f"  {name}: largest |device - predicted| / bar = {excess:.3f}")
            assert excess <= 1.0
    finally:
        r.close()


@pytest.mark.parametrize("view", list(VIEWS))
def test_i_plane_is_the_luma_of_the_disk_layer(view):
    from bhr_amd import _lib
    pos, kw = VIEWS[view]
    r = _mk(97, 55, **kw)
    try:
        r.build_ray_map(pos, FOV)
        S = _frame(r, "toroidal", 0.7, 7.3)
        disk = r.read_layer(_lib.LAYER_DISK).astype(np.float64)
        free = (disk < 1.0).all(axis=-1) & (r.ray_map_passes()["crossings"] <= 4)
        terms = disk * LUMA
        ulp = np.spacing(terms.max(axis=-1).astype(np.float32)).astype(np.float64)
        err = np.abs(S[0] - terms.sum(axis=-1))
        print(f"{view}: {free.sum()} unclamped pixels, largest |I - luma| {np.max(err[free] / np.maximum(ulp[free], 1e-30)):.2f} ulp of the largest term")
        assert free.sum() > 0.9 * free.size and S[0].max() > 0.01
        assert (err[free] <= 4 * ulp[free]).all()
    finally:
        r.close()


def test_nothing_existing_moves():
    from bhr_amd import _lib
    pos, kw = VIEWS["default"]
    r = _mk(97, 55, outputs="f32+blur+u8")
    try:
        r.build_ray_map(pos, FOV)

        def frame():
            r.render_from_ray_map_async(t_offset=7.3)
            return [r.read_layer(k).tobytes() for k in (_lib.LAYER_BG, _lib.LAYER_DISK, _lib.LAYER_BLUR, _lib.LAYER_FINAL)] + [r.read_final_u8().tobytes()]

        def marched():
            r.render_async(list(pos), FOV, frame=3)
            return r.read_layer(_lib.LAYER_FINAL).tobytes()
        off, plain = frame(), marched()
        r.set_polarization("toroidal", 0.7, 16)
        on, with_pol = frame(), marched()
        assert r.stokes()[1].any()                                # (of the map frame: a marched frame leaves the planes alone)
        r.set_polarization(None)
        again = frame()
        assert on == off and again == off and with_pol == plain
    finally:
        r.close()


def test_overflow_pixels_are_zero_and_the_rest_unchanged():
    pos, kw = VIEWS["close"]
    r = _mk(97, 55)
    try:
        r.build_ray_map(pos, FOV)
        full = _frame(r, (0.3, 0.8, 0.5), 1.0, 7.3)
        cells_full = r.stokes_cells()
        r.set_option("raymap_slots", 1)
        r.build_ray_map(pos, FOV)
        info, cnt = r.ray_map_info(), r.ray_map_passes()["crossings"]
        over = cnt > 1
        assert info["slots"] == 1 and info["overflow_pixels"] == over.sum() > 100
        S = _frame(r, (0.3, 0.8, 0.5), 1.0, 7.3)
        assert (S[:, over] == 0).all() and full[0][over].any()
        assert np.array_equal(S[:, ~over], full[:, ~over])
        assert not np.array_equal(r.stokes_cells(), cells_full)
    finally:
        r.close()


@pytest.mark.parametrize("cell", [8, 16, 32])
def test_cells_are_the_means_of_the_planes(cell):
    pos, kw = VIEWS["default"]
    W, H = 97, 55
    r = _mk(W, H)
    try:
        r.build_ray_map(pos, FOV)
        S = _frame(r, "toroidal", 0.7, 7.3, cell).astype(np.float64)
        cells = r.stokes_cells()
        gh, gw = -(-H // cell), -(-W // cell)
        assert cells.shape == (gh, gw, 3) and cells.dtype == np.float32
        worst = 0.0
        for gy in range(gh):
            for gx in range(gw):
                block = S[:, gy * cell:(gy + 1) * cell, gx * cell:(gx + 1) * cell]        # an edge cell: the pixels it has
                n = block[0].size
                for k in range(3):
                    bar = 2 * float(np.spacing(np.float32(np.abs(block[k]).max()))) * n
                    err = abs(float(cells[gy, gx, k]) - block[k].mean())
                    worst = max(worst, err / bar if bar > 0 else (0.0 if err == 0 else np.inf))
        print(f"cell {cell}: largest |device - mean| / bar = {worst:.4f}")
        assert worst <= 1.0 and np.abs(cells[..., 1]).max() > 0
        again = _frame(r, "toroidal", 0.7, 7.3, cell)
        assert np.array_equal(again, S.astype(np.float32)) and r.stokes_cells().tobytes() == cells.tobytes()      # the same bits
    finally:
        r.close()


def test_frame_slots_own_their_planes():
    pos, kw = VIEWS["default"]
    times = (0.0, 1.1, 2.2, 3.3)
    r = _mk(97, 55, frame_slots=2)
    try:
        r.build_ray_map(pos, FOV)
        r.set_polarization((0.3, 0.8, 0.5), 1.0, 8)
        alone = []
        for t in times:
            r.render_from_ray_map_async(t_offset=t)
            alone.append((r.stokes(), r.stokes_cells()))
        assert not np.array_equal(alone[0][0], alone[1][0])
        for n in range(1, len(times) + 1):
            for t in times[:n]:                                   # n frames in flight on the two slots, nothing read in between
                r.render_from_ray_map_async(t_offset=t)
            S, cells = r.stokes(), r.stokes_cells()
            assert np.array_equal(S, alone[n - 1][0]) and np.array_equal(cells, alone[n - 1][1]), f"{n} frames in flight"
    finally:
        r.close()


def test_a_scene_write_waits_for_the_stokes_pass():
    """The Stokes pass samples the disk texture behind its frame's march bracket, so it is the frame's last reader of the scene.
    With two frame slots a texture composed straight behind a map frame -- nothing read in between -- must wait for it: every
    frame's planes and DISK layer are those of the texture the frame was launched under, as one frame at a time gives them.
    A full-HD frame, so that the pass is still running when the compose launches arrive."""
    import os
    import types
    from bhr_amd import HipRenderer, _lib
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compose.npz"))
    c = d["comp"]
    st = types.SimpleNamespace(
        n_r=c.shape[1], n_phi=c.shape[2], enable_rt=True, color_temp=float(d["color_temp"]), omega_rows=d["omega_rows"], edge=d["edge"],
        temp_base=c[0], spiral=c[1], spiral_temp=c[2], turbulence=c[3], turb_temp=c[4], arcs=c[5], arcs_temp=c[6], rt_spikes=c[7],
        rt_temp=c[8], hotspot=c[9], hotspot_temp=c[10], az_hotspot=c[11], disturb_mod=c[12])
    pos, kw = VIEWS["default"]
    sky, _ = _scene()
    times = (0.0, 5.0, 50.0, 180.0)              # the texture's roll: four different textures
    r = HipRenderer(1920, 1080, sky, np.zeros((st.n_r, st.n_phi, 4), dtype=np.float32), math="strict", frame_slots=2)
    try:
        r.upload_parametric_state(st)
        r.build_ray_map(pos, FOV)
        r.set_polarization((0.3, 0.8, 0.5), 1.0, 16)
        alone = []
        for t in times:
            r.update_disk_texture_gpu(t)
            r.sync()
            r.render_from_ray_map_async(t_offset=0.0, skip_bloom=True)
            alone.append((r.stokes(), r.stokes_cells(), r.read_layer(_lib.LAYER_DISK)))
            r.sync()
        assert alone[0][0][1].any() and not np.array_equal(alone[0][0], alone[1][0])
        for n in range(1, len(times) + 1):
            for t in times[:n]:                                   # compose, frame, compose, frame ... on the two slots, nothing read
                r.update_disk_texture_gpu(t)
                r.render_from_ray_map_async(t_offset=0.0, skip_bloom=True)
            r.update_disk_texture_gpu(times[n % len(times)])      # ... and another texture straight behind the last frame
            S, cells, disk = r.stokes(), r.stokes_cells(), r.read_layer(_lib.LAYER_DISK)
            assert np.array_equal(disk, alone[n - 1][2]), f"{n} frames in flight: the DISK layer"
            assert np.array_equal(S, alone[n - 1][0]) and np.array_equal(cells, alone[n - 1][1]), f"{n} frames in flight: the Stokes planes"
    finally:
        r.close()


def test_the_stokes_kernels_use_no_scratch():
    r = _mk(9, 7)
    try:
        for diff in (False, True):
            res = r.stokes_resources(diff)
            print(f"Stokes kernel, differentials {diff}: {res}")
            assert res["scratch_bytes"] == 0 and 0 < res["vgprs"] <= 102          # 102: the most registers at five waves per SIMD
    finally:
        r.close()


def test_refusals(hip_lib):
    from bhr_amd import HipRenderer, _lib
    pos, kw = VIEWS["default"]
    sky, tex = _scene()
    r = _mk()
    try:
        def set_raw(*v):
            par = _lib.Polarization(*v)
            rc = hip_lib.bhr_set_polarization(r._ctx, C.byref(par))
            return rc, hip_lib.bhr_last_error().decode()
        for bad in ((0.0, 0.0, 0.0, 0.7, 16), (float("nan"), 1.0, 0.0, 0.7, 16), (float("inf"), 1.0, 0.0, 0.7, 16), (0.0, 1.0, 0.0, 1.5, 16),
                    (0.0, 1.0, 0.0, -0.1, 16), (0.0, 1.0, 0.0, float("nan"), 16), (0.0, 1.0, 0.0, 0.7, 12), (0.0, 1.0, 0.0, 0.7, 0),
                    (0.0, 1.0, 0.0, 0.7, 16, (1, 0, 0))):
            rc, msg = set_raw(*bad)
            assert rc == _lib.BHR_ERR_INVALID and "polarisation" in msg, (bad, msg)
        with pytest.raises(AssertionError, match="polarisation"):          # off: nothing to read
            r.stokes()
        r.build_ray_map(pos, FOV)
        r.set_polarization("toroidal")
        for read in (r.stokes, r.stokes_cells):                            # set, but no frame from the map yet
            with pytest.raises(AssertionError, match="no frame from the ray map"):
                read()
        r.render_async(list(pos), FOV)                                     # a marched frame is none
        with pytest.raises(AssertionError, match="no frame from the ray map"):
            r.stokes()
        with pytest.raises(AssertionError, match="polarisation"):
            r.render_shutter_from_ray_map_async([0.0, 0.1])
        with pytest.raises(AssertionError, match="polarisation"):
            r.render_from_ray_map_async(cam_pos=[6.0 * np.cos(0.3), 6.0 * np.sin(0.3), 0.5], fov=FOV)      # the build camera turned about z
        with pytest.raises(ValueError, match="Stokes plane"):
            _lib.check(hip_lib.bhr_read_stokes(r._ctx, 3, _lib.fptr(np.zeros(r.width * r.height, dtype=np.float32))))
        r.render_from_ray_map_async(t_offset=0.0)
        assert r.stokes()[0].any()
        r.build_ray_map(pos, FOV)                                          # a new map: its frames are to come
        with pytest.raises(AssertionError, match="no frame from the ray map"):
            r.stokes()
        r.build_ray_map(pos, FOV, supersample=2)
        with pytest.raises(AssertionError, match="polarisation.*supersampled"):
            r.render_from_ray_map_async(t_offset=0.0)
        r.set_polarization(None)
        r.render_from_ray_map_async(t_offset=0.0)                          # off: the supersampled map renders
        r.sync()
    finally:
        r.close()
    for make, word in ((lambda: HipRenderer(64, 36, sky, tex, math="strict", spin=0.5), "spin"),
                       (lambda: HipRenderer(64, 36, sky, tex, math="strict", rows=(0, 18)), "whole-frame")):
        q = make()
        try:
            with pytest.raises(ValueError, match=word):
                q.set_polarization("toroidal")
        finally:
            q.close()
    q = _mk()
    try:
        from bhr_amd.disk_v2 import DiskV2Params
        q.use_disk_v2(DiskV2Params(r_in=q.r_disk_inner, r_out=q.r_disk_outer))
        with pytest.raises(ValueError, match="Disk V2"):
            q.set_polarization("toroidal")
    finally:
        q.close()


def _driver_scene(W, H):
    return dict(width=W, height=H, cam_pos=[6.0, 0.0, 0.5], fov=90.0, step_size=0.1, n_stars=400, tex_w=256, tex_h=128, math="fast")


def test_drivers_end_to_end(tmp_path, capsys):
    """A still at sd writes the .npz and the ticks PNG; a 4-frame --ray_map video writes one grid stack, whose frame 0 is the
    still's grid; the frames themselves are what they are without the polarisation."""
    import json
    import os
    from PIL import Image
    from bhr_amd import drivers, polarization
    W, H = 640, 360
    sc = _driver_scene(W, H)
    pol = dict(field="toroidal", fraction=0.7, cell=16)
    npz, png = str(tmp_path / "still.npz"), str(tmp_path / "ticks.png")
    img = drivers.render_image(**sc, polarization=pol, stokes_path=npz, ticks_path=png)
    assert "Polarization: field (0.0, 1.0, 0.0)" in capsys.readouterr().out
    plain = drivers.render_image(**sc, stars=None)
    with np.load(npz) as z:
        still_cells = z["cells"]
        I, Q, U = z["I"], z["Q"], z["U"]
        assert still_cells.shape == (-(-H // 16), W // 16, 3) and I.shape == (H, W) and int(z["cell"]) == 16
        assert tuple(z["field"]) == (0.0, 1.0, 0.0) and float(z["fraction"]) == 0.7 and str(z["convention"]) == polarization.CONVENTION
        assert tuple(z["cam_pos"]) == (6.0, 0.0, 0.5)
    assert I.max() > 0 and np.abs(Q).max() > 0 and (np.hypot(Q, U) <= 0.7 * I * (1 + 1e-5) + 1e-12).all()
    # the frame is the marched strict frame's layers under the context's bloom, like a point-star still: the same picture as
    # without the flag up to the arithmetic of the march (math="fast" marches the plain one)
    assert img.shape == plain.shape == (H, W, 3) and np.abs(img - plain).mean() < 2e-3
    ticks = np.array(Image.open(png).convert("RGB"))
    assert ticks.shape == (H, W, 3)
    from bhr_amd.output import quantize
    changed = (ticks != quantize(img)).any(axis=-1)
    assert 50 < changed.sum() < 0.2 * W * H and (ticks[changed] == 255).all()
    # the video
    r, _, n_r, n_phi = drivers.make_renderer(W, H, sc["cam_pos"], sc["fov"], n_stars=400, tex_w=256, tex_h=128, math="strict")
    out = str(tmp_path / "v" / "v.mp4")
    try:
        with pytest.raises(ValueError, match="ray_map"):
            drivers.render_video(r, W, H, n_frames=4, fps=24, output_path=out, fov=sc["fov"], static_cam_pos=sc["cam_pos"], video_stream="off",
                                 assemble=False, polarization=pol)
        drivers.render_video(r, W, H, n_frames=4, fps=24, output_path=out, fov=sc["fov"], static_cam_pos=sc["cam_pos"], video_stream="off",
                             assemble=False, ray_map=True, polarization=pol)
        with pytest.raises(AssertionError):                       # switched off on return
            r.stokes()
    finally:
        r.close()
    assert json.load(open(os.path.join(drivers._frames_dir(out), "progress.json")))["params"]["polarization"] == \
        {"field": [0.0, 1.0, 0.0], "fraction": 0.7, "cell": 16}
    with np.load(str(tmp_path / "v" / "v.stokes.npz")) as z:
        stack = z["cells"]
        assert "I" not in z.files and int(z["cell"]) == 16
    assert stack.shape == (4,) + still_cells.shape
    assert np.array_equal(stack[0], still_cells)
    assert not np.array_equal(stack[1], stack[0])                 # the texture moves on
