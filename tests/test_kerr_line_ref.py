"""The Kerr line profile's NumPy reference (tests/kerr_line_ref.py) on the host: the records of binary64 host marches of the GPU
test's views at 64 x 36, every spin and both redshift modes, through the model -- the integer bookkeeping (every Q lands in exactly
one cell, the sum does not depend on the order), `first` against `all`, the two emissivities against t_offset, the fixed-point
bound, and F32_DISTANCE, the float32 reference's distance from the float64 one, which the GPU test's bar is four times."""
import functools

import numpy as np
import pytest

import kerr_line_ref as L
import kerr_ref as K
import kerr_redshift_ref as R

W, H = 64, 36
CASES = tuple((A, v, m) for A in L.SPINS for v in L.VIEWS for m in L.MODES)


@functools.lru_cache(maxsize=None)
def _tex():
    from bhr_amd import scenes
    tex = scenes.noisy_disk()
    tex.setflags(write=False)
    return tex


@functools.lru_cache(maxsize=None)
def _records(A, view, mode):
    cam, hits, crossings = L.host_records(view, A, mode, W, H)
    hits.setflags(write=False)
    crossings.setflags(write=False)
    return cam, hits, crossings


def _frame(case, dtype=np.float64, t_offset=0.0, **kw):
    A, view, mode = case
    cam, hits, crossings = _records(A, view, mode)
    s = L.settings(**kw)
    return s, L.frame(cam, hits, crossings, A, mode, s, _tex(), t_offset, dtype=dtype)


def test_g_model_is_kerr_ref_g_factor_s_g():
    """shade_g (kerr_ref.g_factor from its g on) of g_model's g is kerr_ref.g_factor's colour, bit for bit."""
    A, view = 0.6, L.VIEWS[0]
    cam, hits, crossings = _records(A, view, "model")
    sel = crossings >= 1
    h = hits[0][sel].astype(np.float64)
    a = A * K.M
    r = np.sqrt(h[:, 0] ** 2 + h[:, 1] ** 2 - a * a)
    base = np.full((h.shape[0], 3), 0.5)
    g = L.g_model(h[:, 0], h[:, 1], h[:, 2:5], a, cam["pos"])
    assert np.array_equal(R.shade_g(base, g, r, 2.0, 15.0), K.g_factor(base, h[:, 0], h[:, 1], r, h[:, 2:5], a, cam["pos"], 2.0, 15.0))


def test_exact_records_carry_the_march_s_photon_numbers():
    """host_records gives the exact redshift's photon as (px, py, 0): its (L_z, P, U) are the march's."""
    A, view = 0.998, L.VIEWS[1]
    cam = K.build_camera(view, 90.0, W, H)
    m = R.march(cam["pos"].astype(np.float64), K.pixel_rays(cam).reshape(-1, 3), A, 0.1, cam["r_escape"])
    rows = m["hits"][m["hits"][:, 1] == 0]
    hx, hy = rows[:, 2], rows[:, 3]
    rho2 = hx * hx + hy * hy
    rho = np.sqrt(rho2)
    px, py = (hx * rows[:, 5] * rho - hy * rows[:, 4]) / rho2, (hy * rows[:, 5] * rho + hx * rows[:, 4]) / rho2
    lz, P, U = L.photon_numbers(hx, hy, px, py, A * K.M)
    assert np.allclose(lz, rows[:, 4], rtol=1e-12, atol=1e-12) and np.allclose(P, rows[:, 5], rtol=1e-12, atol=1e-12)
    assert np.allclose(U, rows[:, 6], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", CASES[::5], ids=str)
def test_every_q_lands_in_one_cell_and_the_order_does_not_matter(case):
    rng = np.random.default_rng(11)
    for kw in (dict(), dict(n_bins=7, g_range=(0.6, 1.0), orders="all"), dict(n_bins=1000, emissivity="texture", orders="all"),
               dict(n_bins=1, g_range=(2.0, 3.0))):
        s, f = _frame(case, **kw)
        bins, under, over = L.histogram(f["g"], f["w"], f["counted"], s)
        total = int(L.sample_q(f["w"][f["counted"]], s["power"]).sum(dtype=np.uint64))
        assert int(bins.sum(dtype=np.uint64)) + int(under) + int(over) == total
        n = int(f["counted"].sum())
        assert n > 100
        b2, u2, o2 = L.histogram(f["g"], f["w"], f["counted"], s, order=rng.permutation(n))
        assert np.array_equal(bins, b2) and under == u2 and over == o2
        if kw.get("g_range") == (2.0, 3.0):
            assert under == total and not bins.any() and over == 0        # g <= 1.5: everything below the range
        # the planes are 0 exactly where nothing counts
        assert not f["g"][~f["counted"]].any() and not f["w"][~f["counted"]].any()


@pytest.mark.parametrize("case", CASES[1::7], ids=str)
def test_first_is_below_all_bin_by_bin(case):
    for em in L.DEFAULTS["emissivity"], "texture":
        s, f1 = _frame(case, emissivity=em, orders="first")
        _, fa = _frame(case, emissivity=em, orders="all")
        if em == "powerlaw":
            b1, ba = L.histogram(f1["g"], f1["w"], f1["counted"], s)[0], L.histogram(fa["g"], fa["w"], fa["counted"], s)[0]
            assert (b1 <= ba).all()
        assert (f1["counted"] <= fa["counted"]).all()
        # the first counted record is weighed the same way in both -- but for the transmittance of uncounted records in front of it
        k1 = f1["counted"]
        assert np.array_equal(f1["g"][k1], fa["g"][k1])
        assert (f1["w"][k1] >= fa["w"][k1]).all()


def test_powerlaw_ignores_t_offset_and_texture_does_not():
    case = (0.6, L.VIEWS[0], "exact")
    for orders in ("first", "all"):
        _, p0 = _frame(case, t_offset=0.0, orders=orders)
        _, p1 = _frame(case, t_offset=7.3, orders=orders)
        assert np.array_equal(p0["w"], p1["w"]) and np.array_equal(p0["g"], p1["g"])
        _, t0 = _frame(case, t_offset=0.0, orders=orders, emissivity="texture")
        _, t1 = _frame(case, t_offset=7.3, orders=orders, emissivity="texture")
        assert np.array_equal(t0["g"], t1["g"]) and not np.array_equal(t0["w"], t1["w"])


def test_the_fixed_point_bound():
    """8 slots of a 7680 x 4320 frame at the largest Q stay under 2^61, and so under 2^63; the largest Q is 2^32."""
    assert L.max_sum_bound(8, 7680, 4320) < 2 ** 61 < 2 ** 63
    for p in (0.0, 1.5, 4.0, 8.0):
        w_max = np.float32(L.G_CAP) ** np.float32(p)
        assert int(L.sample_q(w_max, p)) <= (1 << 32) + 512          # f32 rounding of unit and of the product: 2^-23 relative


def test_second_crossings_are_there():
    """The condition the GPU test's orders case puts on its input: at least 5 % two-crossing pixels among the lit ones."""
    _, _, crossings = _records(0.998, L.VIEWS[1], "exact")
    assert (crossings >= 2).sum() >= 0.05 * (crossings >= 1).sum()


def test_f32_distance():
    """The largest |float32 reference - float64 reference| of g (relative) and of w (relative to the frame's largest w) over the
    records of every case, both emissivities at t_offset 0 and 7.3 with orders "all": kerr_line_ref.F32_DISTANCE_G / _W hold it and
    are not more than 1.5 times it."""
    worst_g = worst_w = 0.0
    for case in CASES:
        for em, t_off in (("powerlaw", 0.0), ("texture", 7.3)):
            _, f64 = _frame(case, np.float64, t_off, emissivity=em, orders="all")
            _, f32 = _frame(case, np.float32, t_off, emissivity=em, orders="all")
            both = f64["counted"] & f32["counted"]
            assert both.sum() >= 0.999 * f64["counted"].sum()
            assert f32["g"].dtype == np.float32 and f32["w"].dtype == np.float32
            dg = np.abs(f32["g"].astype(np.float64) - f64["g"])[both] / f64["g"][both]
            dw = np.abs(f32["w"].astype(np.float64) - f64["w"])[both] / f64["w"].max()
            worst_g, worst_w = max(worst_g, float(dg.max())), max(worst_w, float(dw.max()))
    print(f"F32_DISTANCE measured: g {worst_g:.3e}, w {worst_w:.3e}")
    assert worst_g <= L.F32_DISTANCE_G <= 1.5 * worst_g
    assert worst_w <= L.F32_DISTANCE_W <= 1.5 * worst_w
