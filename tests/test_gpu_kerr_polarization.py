"""Kerr polarisation on the device (bhr_set_kerr_polarization; include/bhr.h "Kerr polarisation"): the Stokes planes
of a frame from the Kerr ray map against the binary64 reference (tests/kerr_polar_ref.py) fed the DEVICE's own records -- hits and
photon momenta --, the weights of two crossings, the I plane, that nothing existing moves, the overflow list, frame slots, scene
writes, the refusals, and the hole that does not spin against the context's Schwarzschild planes.

The bar.  TOL = 4 x kerr_polar_ref.F32_DISTANCE = 4 x 2.08e-6 on Q / I and U / I: the largest |float32 reference - float64
reference| over the records of these views, spins, modes and fields with Pi_0 = 1, measured and asserted on the host
(tests/test_kerr_polar_ref.py); four times it covers another operation order, FMA contraction and the device's libm.

Scenes: scenes.analytic_skybox() and scenes.noisy_disk(), fov 90, the renderer's defaults (r_disk 2 .. 15, step 0.1).  The
condition on a view: single-crossing pixels are at least 85 % of the pixels with a crossing (75 % at 5 x 3); the host march has
0.857 .. 0.976 and >= 0.80.  The 1 x 1 frame's one ray is the radial one: it crosses no disk and the planes hold zeros.

Measured on an MI355X: largest device difference 2.18e-6 ((4, 3, 2) at 64 x 36; the float32 reference on the same records 2.09e-6),
1.34e-6 at 33 x 9, 1.99e-6 at 9 x 7, 1.60e-6 at 5 x 3; forced A = 0 against the Schwarzschild planes 0.178 / 0.185 / 0.139."""
import ctypes as C
import functools

import numpy as np
import pytest

import kerr_polar_ref as P

pytestmark = pytest.mark.gpu

FOV = 90.0
TOL = 4 * P.F32_DISTANCE
TOL_SCHWARZSCHILD = 4.39e-6                      # tests/test_gpu_polarization.py: the Schwarzschild pass's bar
VIEWS = ((6.0, 0.0, 0.5), (2.5, 2.0, 1.2), (4.0, 3.0, 2.0))
SPINS = ((0.0, True), (0.6, False), (-0.9, False), (0.998, False))         # (A, forced)
FIELDS = ("toroidal", "radial", "vertical", (0.3, 0.8, 0.5))
SIZES = ((64, 36), (33, 9), (9, 7), (5, 3), (1, 1))
LUMA = np.array((0.2126, 0.7152, 0.0722))


@functools.lru_cache(maxsize=None)
def _scene():
    from bhr_amd import scenes
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    sky.setflags(write=False)
    tex.setflags(write=False)
    return sky, tex


def _mk(W=64, H=36, A=0.6, mode="model", force=False, tex=None, **kw):
    from bhr_amd import HipRenderer
    sky, noisy = _scene()
    r = HipRenderer(W, H, sky, noisy if tex is None else tex, math="strict", **kw)
    _spin(r, A, mode, force)
    return r


def _spin(r, A, mode, force=False):
    r.set_redshift("model")
    r.set_spin(A, force_kerr=force)
    r.set_redshift(mode)


def _vector(field):
    from bhr_amd import polarization
    return polarization.field_vector(field)


def _cam(r, pos):
    c = r.camera_uniforms(list(pos), FOV, 0)
    return dict(pos=np.array(list(c.pos), dtype=np.float32), right=np.array(list(c.right), dtype=np.float32), up=np.array(list(c.up), dtype=np.float32),
                forward=np.array(list(c.forward), dtype=np.float32), pw=np.float32(c.pixel_width), ph=np.float32(c.pixel_height), width=r.width, height=r.height)


def _build(r, pos, field="toroidal", frac=0.7, cell=16):
    """The polarisation first: the build then keeps the momenta.  -> (passes, momenta)."""
    r.set_kerr_polarization(field, frac, cell)
    r.build_kerr_ray_map(list(pos), FOV)
    return r.kerr_ray_map_passes(), r.kerr_ray_map_momentum()


def _predict(r, pos, passes, mom, A, mode, field, frac, dtype=np.float64):
    a, b, ok = P.frame_stokes(_cam(r, pos), passes["hits"], mom, A, mode, _vector(field), frac, r.r_disk_inner, r.r_disk_outer, dtype)
    K = passes["hits"].shape[0]
    live = np.arange(K)[:, None, None] < np.minimum(passes["crossings"], K)[None]
    return a, b, ok, live


def _frame(r, field, frac, t=0.0, cell=16):
    r.set_kerr_polarization(field, frac, cell)      # (a change of the setting keeps the map and its momenta)
    r.render_from_kerr_ray_map_async(t_offset=t, skip_bloom=True)
    return r.stokes()


def _ratio(S):
    I, Q, U = S.astype(np.float64)
    lit = I > 1e-4 * max(float(I.max()), 1e-30)
    safe = np.where(lit, I, 1.0)
    return Q / safe, U / safe, lit


@pytest.mark.parametrize("view", VIEWS, ids=lambda v: "-".join(f"{c:g}" for c in v))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_single_crossing_pixels(size, view):
    W, H = size
    r = _mk(W, H)
    worst = own = 0.0
    try:
        for A, force in SPINS:
            for mode in ("model", "exact"):
                _spin(r, A, mode, force)
                p, mom = _build(r, view)
                cnt = p["crossings"]
                one, any_ = cnt == 1, cnt >= 1
                share = one.sum() / max(any_.sum(), 1)
                empty = (W, H) == (1, 1)
                if empty:
                    assert not any_.any()
                else:
                    assert share >= (0.75 if (W, H) == (5, 3) else 0.85), (A, mode, share)
                # a record's momentum is there exactly where its hit is
                assert np.array_equal(mom.any(axis=-1), p["hits"][..., :2].any(axis=-1))
                for n, field in enumerate(FIELDS):
                    t, frac = ((0.0, 0.7), (7.3, 1.0))[n % 2] if A != 0.6 else ((7.3, 1.0), (0.0, 0.7))[n % 2]
                    S = _frame(r, field, frac, t)
                    assert np.isfinite(S).all()
                    if empty:
                        assert not S.any()
                        continue
                    a, b, ok, live = _predict(r, view, p, mom, A, mode, field, frac)
                    a32, b32, _, _ = _predict(r, view, p, mom, A, mode, field, frac, np.float32)
                    q, u, lit = _ratio(S)
                    m = one & lit & ok[0]
                    assert m.sum() >= 0.9 * (one & lit).sum() and m.any()
                    dq, du = np.abs(q - a[0])[m].max(), np.abs(u - b[0])[m].max()
                    own = max(own, np.abs(a32 - a)[0][m].max(), np.abs(b32 - b)[0][m].max())
                    worst = max(worst, dq, du)
                    assert dq <= TOL and du <= TOL, f"{view} {W}x{H} A {A} {mode} {field} t {t} Pi_0 {frac}: |d Q/I| {dq:.3e}, |d U/I| {du:.3e} over {TOL:.2e}"
                    assert (np.hypot(S[1], S[2]) <= frac * S[0] * (1 + 1e-5) + 1e-12).all()        # Q^2 + U^2 <= (Pi_0 I)^2
                    if field == "toroidal" and W * H >= 64 * 36:
                        assert np.hypot(q, u)[m].max() > 0.2 * frac                                # there is something to compare
        print(f"{view} {W}x{H}: largest device difference {worst:.3e}; float32 reference on the same records {own:.3e}; bar {TOL:.2e}")
    finally:
        r.close()


@pytest.mark.parametrize("A, mode, view", [(0.6, "exact", VIEWS[1]), (-0.9, "model", VIEWS[0])])
def test_two_crossing_weights(A, mode, view):
    """The weights c_k do not depend on the field: solved from I and Q under field A, they predict U under A and Q, U under B
    (tests/test_gpu_polarization.py has the bar's derivation)."""
    r = _mk(64, 36, A, mode)
    try:
        p, mom = _build(r, view)
        two = p["crossings"] == 2
        fA, fB = (0.3, 0.8, 0.5), "vertical"
        SA, SB = _frame(r, fA, 1.0, 7.3).astype(np.float64), _frame(r, fB, 1.0, 7.3).astype(np.float64)
        assert np.array_equal(SA[0], SB[0])                      # I does not depend on the field
        aA, bA, okA, _ = _predict(r, view, p, mom, A, mode, fA, 1.0)
        aB, bB, okB, _ = _predict(r, view, p, mom, A, mode, fB, 1.0)
        I = SA[0]
        usable = two & okA[0] & okA[1] & okB[0] & okB[1] & (I > 1e-4 * I.max())
        m = usable & (np.abs(aA[0] - aA[1]) > 0.05)
        print(f"{view} A {A} {mode}: {two.sum()} two-crossing pixels, {usable.sum()} lit, {m.sum()} with |a_1 - a_2| > 0.05")
        assert m.sum() >= 0.5 * two.sum() and m.sum() > 20
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


@pytest.mark.parametrize("mode", ["model", "exact"])
def test_i_plane_is_the_luma_of_the_disk_layer(mode):
    from bhr_amd import _lib
    r = _mk(64, 36, -0.9, mode)
    try:
        p, _ = _build(r, VIEWS[1])
        S = _frame(r, "toroidal", 0.7, 7.3)
        disk = r.read_layer(_lib.LAYER_DISK).astype(np.float64)
        free = (disk < 1.0).all(axis=-1) & (p["crossings"] <= 4)
        terms = disk * LUMA
        ulp = np.spacing(terms.max(axis=-1).astype(np.float32)).astype(np.float64)
        err = np.abs(S[0] - terms.sum(axis=-1))
        print(f"{mode}: {free.sum()} unclamped pixels, largest |I - luma| {np.max(err[free] / np.maximum(ulp[free], 1e-30)):.2f} ulp of the largest term")
        assert free.sum() > 0.9 * free.size and S[0].max() > 0.01
        assert (err[free] <= 4 * ulp[free]).all()
    finally:
        r.close()


@pytest.mark.parametrize("mode", ["model", "exact"])
def test_nothing_existing_moves(mode):
    """BG, DISK, BLUR, FINAL and the u8 rows of a map frame, the map's planes, and a marched frame: the bytes they are without it."""
    from bhr_amd import _lib
    pos = VIEWS[0]
    r = _mk(33, 9, 0.998, mode, outputs="f32+blur+u8")
    try:
        def frame():
            r.render_from_kerr_ray_map_async(t_offset=7.3)
            return [r.read_layer(k).tobytes() for k in (_lib.LAYER_BG, _lib.LAYER_DISK, _lib.LAYER_BLUR, _lib.LAYER_FINAL)] + [r.read_final_u8().tobytes()]

        def marched():
            r.render_async(list(pos), FOV, frame=3)
            return r.read_layer(_lib.LAYER_FINAL).tobytes()
        r.build_kerr_ray_map(list(pos), FOV)
        plain_map = {k: v.tobytes() for k, v in r.kerr_ray_map_passes().items()}
        with pytest.raises(AssertionError, match="without the photon momenta"):
            r.kerr_ray_map_momentum()
        off, plain = frame(), marched()
        p, mom = _build(r, pos)
        assert {k: v.tobytes() for k, v in p.items()} == plain_map and mom.any()
        on, with_pol = frame(), marched()
        assert r.stokes()[1].any()
        r.set_kerr_polarization(None)
        again = frame()                                              # the map keeps its momenta; a frame without the setting ignores them
        assert on == off and again == off and with_pol == plain
    finally:
        r.close()


def test_overflow_pixels_are_zero_and_the_rest_unchanged():
    pos = VIEWS[1]
    r = _mk(64, 36, 0.6, "exact")
    try:
        _build(r, pos)
        full = _frame(r, (0.3, 0.8, 0.5), 1.0, 7.3)
        r.set_option("raymap_slots", 1)
        p, mom = _build(r, pos)
        info, cnt = r.kerr_ray_map_info(), p["crossings"]
        over = cnt > 1
        assert info["slots"] == 1 and mom.shape[0] == 1 and info["overflow_pixels"] == over.sum() > 50
        S = _frame(r, (0.3, 0.8, 0.5), 1.0, 7.3)
        assert (S[:, over] == 0).all() and full[0][over].any()
        assert np.array_equal(S[:, ~over], full[:, ~over])
    finally:
        r.close()


def test_frame_slots_own_their_planes():
    times = (0.0, 1.1, 2.2, 3.3)
    r = _mk(64, 36, -0.9, "exact", frame_slots=2)
    try:
        _build(r, VIEWS[0], (0.3, 0.8, 0.5), 1.0, 8)
        alone = []
        for t in times:
            r.render_from_kerr_ray_map_async(t_offset=t)
            alone.append((r.stokes(), r.stokes_cells()))
        assert not np.array_equal(alone[0][0], alone[1][0])
        for n in range(1, len(times) + 1):
            for t in times[:n]:                                   # n frames in flight on the two slots, nothing read in between
                r.render_from_kerr_ray_map_async(t_offset=t)
            S, cells = r.stokes(), r.stokes_cells()
            assert np.array_equal(S, alone[n - 1][0]) and np.array_equal(cells, alone[n - 1][1]), f"{n} frames in flight"
    finally:
        r.close()


def test_a_scene_write_waits_for_the_stokes_pass():
    """tests/test_gpu_polarization.py's test of the same name over the Kerr pass: a texture composed straight behind a map frame
    leaves that frame's planes and DISK layer alone.  A full-HD frame, so that the pass is still running when the compose arrives."""
    import os
    import types
    from bhr_amd import HipRenderer, _lib
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compose.npz"))
    c = d["comp"]
    st = types.SimpleNamespace(
        n_r=c.shape[1], n_phi=c.shape[2], enable_rt=True, color_temp=float(d["color_temp"]), omega_rows=d["omega_rows"], edge=d["edge"],
        temp_base=c[0], spiral=c[1], spiral_temp=c[2], turbulence=c[3], turb_temp=c[4], arcs=c[5], arcs_temp=c[6], rt_spikes=c[7],
        rt_temp=c[8], hotspot=c[9], hotspot_temp=c[10], az_hotspot=c[11], disturb_mod=c[12])
    sky, _ = _scene()
    times = (0.0, 5.0, 50.0)
    r = HipRenderer(1920, 1080, sky, np.zeros((st.n_r, st.n_phi, 4), dtype=np.float32), math="strict", frame_slots=2)
    try:
        _spin(r, 0.9, "exact")
        r.upload_parametric_state(st)
        r.set_kerr_polarization((0.3, 0.8, 0.5), 1.0, 16)
        r.build_kerr_ray_map(list(VIEWS[0]), FOV)
        alone = []
        for t in times:
            r.update_disk_texture_gpu(t)
            r.sync()
            r.render_from_kerr_ray_map_async(t_offset=0.0, skip_bloom=True)
            alone.append((r.stokes(), r.stokes_cells(), r.read_layer(_lib.LAYER_DISK)))
            r.sync()
        assert alone[0][0][1].any() and not np.array_equal(alone[0][0], alone[1][0])
        for n in range(1, len(times) + 1):
            for t in times[:n]:
                r.update_disk_texture_gpu(t)
                r.render_from_kerr_ray_map_async(t_offset=0.0, skip_bloom=True)
            r.update_disk_texture_gpu(times[n % len(times)])      # ... and another texture straight behind the last frame
            S, cells, disk = r.stokes(), r.stokes_cells(), r.read_layer(_lib.LAYER_DISK)
            assert np.array_equal(disk, alone[n - 1][2]), f"{n} frames in flight: the DISK layer"
            assert np.array_equal(S, alone[n - 1][0]) and np.array_equal(cells, alone[n - 1][1]), f"{n} frames in flight: the Stokes planes"
    finally:
        r.close()


def test_the_kerr_stokes_kernels_use_no_scratch():
    r = _mk(9, 7)
    try:
        for mode in ("model", "exact"):
            res = r.kerr_stokes_resources(mode)
            print(f"Kerr Stokes kernel, {mode} redshift: {res}")
            assert res["scratch_bytes"] == 0 and res["lds_bytes"] == 0 and 0 < res["vgprs"] <= 102   # 102: the most registers at five waves per SIMD
    finally:
        r.close()


def test_refusals(hip_lib):
    from bhr_amd import HipRenderer, _lib
    pos = VIEWS[0]
    sky, tex = _scene()
    # a setter call without a spin names the Schwarzschild setter; with one, bhr_set_polarization keeps refusing it
    r = HipRenderer(64, 36, sky, tex, math="strict")
    try:
        with pytest.raises(AssertionError, match="bhr_set_polarization"):
            r.set_kerr_polarization("toroidal")
        r.set_kerr_polarization(None)                                      # NULL is always taken
        r.set_spin(0.6)
        with pytest.raises(ValueError, match="the transport rule is Schwarzschild's"):
            r.set_polarization("toroidal")

        def set_raw(*v):
            par = _lib.Polarization(*v)
            rc = hip_lib.bhr_set_kerr_polarization(r._ctx, C.byref(par))
            return rc, hip_lib.bhr_last_error().decode()
        for bad in ((0.0, 0.0, 0.0, 0.7, 16), (float("nan"), 1.0, 0.0, 0.7, 16), (0.0, 1.0, 0.0, 1.5, 16), (0.0, 1.0, 0.0, float("nan"), 16),
                    (0.0, 1.0, 0.0, 0.7, 12), (0.0, 1.0, 0.0, 0.7, 16, (1, 0, 0))):
            rc, msg = set_raw(*bad)
            assert rc == _lib.BHR_ERR_INVALID and "bhr_set_kerr_polarization" in msg and "polarisation" in msg, (bad, msg)
        with pytest.raises(AssertionError, match="no polarisation is set"):
            r.stokes()
        # a map built without the momenta
        r.build_kerr_ray_map(list(pos), FOV)
        r.set_kerr_polarization("toroidal")
        with pytest.raises(AssertionError, match=r"built without the photon momenta.*build it again \(bhr_kerr_raymap_build\)"):
            r.render_from_kerr_ray_map_async()
        with pytest.raises(AssertionError, match="no frame from the ray map"):
            r.stokes()
        # a supersampled build
        r.set_option("raymap_supersample", 2)
        with pytest.raises(ValueError, match="no supersampled form"):
            r.build_kerr_ray_map(list(pos), FOV)
        r.set_option("raymap_supersample", 1)
        r.build_kerr_ray_map(list(pos), FOV)
        r.render_from_kerr_ray_map_async()
        assert r.stokes()[1].any()
        # a turned view; the build's own position through the same call is the build view
        with pytest.raises(AssertionError, match="turned views have none"):
            r.render_from_kerr_ray_map_async(cam_pos=[6.0 * np.cos(0.3), 6.0 * np.sin(0.3), 0.5])
        r.render_from_kerr_ray_map_async(cam_pos=list(pos))
        assert r.stokes()[1].any()
        # a changed spin or mode: the planes are gone and the map is another hole's
        r.set_spin(0.5)
        with pytest.raises(AssertionError, match="no frame from the ray map"):
            r.stokes()
        with pytest.raises(AssertionError, match="the map was built for spin"):
            r.render_from_kerr_ray_map_async()
        r.set_spin(0.6)
        r.render_from_kerr_ray_map_async()
        assert r.stokes()[1].any()
        r.set_redshift("exact")
        with pytest.raises(AssertionError, match="no frame from the ray map"):
            r.stokes_cells()
        with pytest.raises(AssertionError, match="the map was built for spin"):
            r.render_from_kerr_ray_map_async()
        # build flags stay refused
        with pytest.raises(ValueError, match="none are defined"):
            _lib.check(hip_lib.bhr_kerr_raymap_build(r._ctx, C.byref(r.camera_uniforms(list(pos), FOV, 0)), 1))
        with pytest.raises(ValueError, match="unknown mode"):
            _lib.check(hip_lib.bhr_kerr_stokes_resources(2, (C.c_int32 * 3)()))
    finally:
        r.close()


@pytest.mark.parametrize("view", VIEWS, ids=lambda v: "-".join(f"{c:g}" for c in v))
def test_forced_spin_zero_against_the_schwarzschild_planes(view):
    """The context's own Schwarzschild Stokes planes of the same view against the Kerr pass at A = 0 (forced), model redshift: within
    the model distance measured on the host (kerr_polar_ref.SCHWARZSCHILD_DISTANCE, the camera stretch the Schwarzschild pass
    ignores) plus both device bars, on the pixels both marches give one crossing."""
    from bhr_amd import HipRenderer
    sky, tex = _scene()
    r = HipRenderer(64, 36, sky, tex, math="strict")
    try:
        worst = 0.0
        r.build_ray_map(list(view), FOV)
        one_s = r.ray_map_passes()["crossings"] == 1
        planes = {}
        for field in FIELDS:
            r.set_polarization(field, 1.0, 16)
            r.render_from_ray_map_async(t_offset=0.0, skip_bloom=True)
            planes[field] = r.stokes()
        r.set_polarization(None)
        r.set_spin(0.0, force_kerr=True)
        p, _ = _build(r, view)
        one = one_s & (p["crossings"] == 1)
        assert one.sum() > 0.8 * one_s.sum()
        for field in FIELDS:
            qk, uk, lit_k = _ratio(_frame(r, field, 1.0, 0.0))
            qs, us, lit_s = _ratio(planes[field])
            m = one & lit_k & lit_s
            assert m.sum() > 0.9 * one.sum()
            worst = max(worst, np.abs(qk - qs)[m].max(), np.abs(uk - us)[m].max())
        print(f"{view}: largest |d Q/I|, |d U/I| between the Kerr pass at A = 0 and the Schwarzschild pass {worst:.4f}")
        assert worst <= P.SCHWARZSCHILD_DISTANCE + TOL + TOL_SCHWARZSCHILD
        assert worst > 1e-3                                              # ... and the stretch is there: the two are different models
    finally:
        r.close()
