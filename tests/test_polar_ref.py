"""The polarisation's model on the CPU (tests/polar_ref.py; include/bhr.h "polarisation"): the planar transport rule against an
independent parallel-transport integrator, the model's invariants, and the host's tick overlay and .npz."""
import numpy as np
import pytest

import polar_ref as R

# periapsis (r_s), the plane's normal (tilted out of the equator), the polarisation angle at the start
RAYS = [(8.0, (0.3, 0.2, 1.0), 0.3), (6.0, (-0.5, 0.4, 1.0), -1.2), (4.6, (1.0, 0.5, 1.0), 1.1), (3.5, (0.2, -0.9, 0.7), 2.6),
        (3.0, (0.6, 0.6, 0.5), 0.0), (2.5, (-0.3, 0.8, 0.9), 0.7), (1.6, (0.2, -0.7, 0.8), 2.0)]


@pytest.mark.parametrize("r_peri,normal,psi0", RAYS)
def test_planar_rule_agrees_with_the_integrator(r_peri, normal, psi0):
    out = R.transport(r_peri, normal, psi0, h=0.01)
    d = np.angle(np.exp(1j * (out["psi_end"] - out["psi_start"])))
    print(f"periapsis {r_peri}: swept {out['swept']:.3f} rad, |d psi| {abs(d):.2e}, plane normal drift {out['N_drift']:.1e}")
    assert abs(d) <= 1e-6
    assert out["N_drift"] <= 1e-6                 # the ray stays in its plane
    if r_peri <= 1.6:
        assert out["swept"] > 2 * np.pi           # more than a full turn about the hole
    if r_peri <= 2.5:
        assert out["swept"] > np.pi


def _random_crossings(n=4000, seed=5, tilt=0.0):
    rng = np.random.default_rng(seed)
    cam = {"pos": np.array([6.0, 0.0, 0.5]), "right": np.array([0.0, 1.0, 0.0]), "up": np.array([-0.083, 0.0, 0.9965]),
           "forward": np.array([-0.9965, 0.0, -0.083]), "pw": 0.03, "ph": 0.03}
    D = rng.normal(size=(n, 3))
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    r = rng.uniform(2.0, 15.0, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    w = rng.normal(size=(n, 3))
    return cam, D, r * np.cos(phi), r * np.sin(phi), w


@pytest.mark.parametrize("tilt", [0.0, 25.0])
def test_step_6_gives_a_unit_vector_across_the_photon(tilt):
    cam, D, hx, hy, w = _random_crossings(tilt=tilt)
    for field in ((0, 1, 0), (1, 0, 0), (0, 0, 1), (0.3, 0.8, 0.5)):
        a, b, ok, d = R.crossing_stokes(cam, D, hx, hy, w, tilt, field, 0.7, 2.0, 15.0, details=True)
        assert ok.sum() > 3900
        f, K = d["f"][ok], d["K"][ok]
        assert np.abs(np.sum(f * f, axis=1) - 1.0).max() <= 1e-12
        assert np.abs(np.sum(f * K, axis=1)).max() <= 1e-12
        assert np.abs(np.sum(K * d["N"][ok], axis=1)).max() <= 1e-12        # K lies in the ray's plane
        assert np.abs(d["cpsi"][ok] ** 2 + d["spsi"][ok] ** 2 - 1.0).max() <= 1e-12


def test_invariants():
    cam, D, hx, hy, w = _random_crossings(seed=9)
    B = np.array([0.3, 0.8, 0.5])
    a, b, ok = R.crossing_stokes(cam, D, hx, hy, w, 0.0, B, 0.7, 2.0, 15.0)
    for other in (-B, 3.0 * B):
        a2, b2, ok2 = R.crossing_stokes(cam, D, hx, hy, w, 0.0, other, 0.7, 2.0, 15.0)
        assert (ok2 == ok).all() and np.abs(a2 - a).max() <= 1e-14 and np.abs(b2 - b).max() <= 1e-14
    a0, b0, _ = R.crossing_stokes(cam, D, hx, hy, w, 0.0, B, 0.0, 2.0, 15.0)
    assert (a0 == 0).all() and (b0 == 0).all()
    # Q^2 + U^2 <= (Pi_0 I)^2 for any weights c_k >= 0: per crossing a^2 + b^2 = p^2 <= Pi_0^2, and the sum is a convex mix
    assert (a * a + b * b <= 0.7 ** 2 * (1 + 1e-12)).all()
    c = np.random.default_rng(2).uniform(0, 1, (len(a) // 4, 4))
    I = c.sum(axis=1)
    Q, U = (c * a.reshape(-1, 4)).sum(axis=1), (c * b.reshape(-1, 4)).sum(axis=1)
    assert (Q * Q + U * U <= (0.7 * I) ** 2 * (1 + 1e-12)).all()
    # outside the annulus and on a radial ray: nothing
    a3, b3, ok3 = R.crossing_stokes(cam, D[:3], [1.5, 16.0, 0.5], [0.0, 0.0, 0.5], w[:3], 0.0, B, 0.7, 2.0, 15.0)
    assert not ok3.any() and (a3 == 0).all() and (b3 == 0).all()
    radial = -cam["pos"] / np.linalg.norm(cam["pos"])
    a4, b4, ok4 = R.crossing_stokes(cam, radial[None], hx[:1], hy[:1], w[:1], 0.0, B, 0.7, 2.0, 15.0)
    assert not ok4.any() and a4[0] == 0 and b4[0] == 0


def test_float32_evaluation_stays_near_the_float64_one():
    """What the device test's bar rests on: the model evaluated in f32 on random crossings."""
    cam, D, hx, hy, w = _random_crossings(seed=3)
    cam32 = {k: (np.asarray(v, dtype=np.float32).astype(np.float64) if k not in ("pw", "ph") else v) for k, v in cam.items()}
    D32, hx32, hy32, w32 = (np.asarray(v, dtype=np.float32) for v in (D, hx, hy, w))
    for field in ((0, 1, 0), (0.3, 0.8, 0.5)):
        a64, b64, ok = R.crossing_stokes(cam32, D32, hx32, hy32, w32, 0.0, field, 1.0, 2.0, 15.0, np.float64)
        a32, b32, ok32 = R.crossing_stokes(cam32, D32, hx32, hy32, w32, 0.0, field, 1.0, 2.0, 15.0, np.float32)
        assert a32.dtype == np.float32 and (ok == ok32).all()
        # random directions D include rays close to radial, where N = normalize(C x D) amplifies D's rounding: leave those out
        far = ok & (np.linalg.norm(np.cross(cam32["pos"], D32.astype(np.float64)), axis=1) > 0.5)
        assert max(np.abs(a32 - a64)[far].max(), np.abs(b32 - b64)[far].max()) <= 2e-5


def _cells(q, u, i=1.0):
    c = np.zeros((3, 3, 3))
    c[1, 1] = (i, q, u)
    return c


def _lit(img):
    ys, xs = np.nonzero(img[..., 0])
    return ys, xs


def test_draw_ticks_orientation():
    from bhr_amd import polarization as P
    frame = np.zeros((48, 48, 3), dtype=np.uint8)
    ys, xs = _lit(P.draw_ticks(frame, _cells(0.5, 0.0), 16))          # Q > 0, U = 0: horizontal
    assert len(set(ys)) == 1 and len(set(xs)) >= 10 and 16 <= xs.min() and xs.max() < 32 and 16 <= ys[0] < 32
    ys, xs = _lit(P.draw_ticks(frame, _cells(-0.5, 0.0), 16))         # Q < 0: vertical
    assert len(set(xs)) == 1 and len(set(ys)) >= 10 and 16 <= ys.min() and ys.max() < 32
    ys, xs = _lit(P.draw_ticks(frame, _cells(0.0, 0.5), 16))          # U > 0: 45 degrees, towards image-up on the right
    assert len(set(xs)) >= 7 and len(set(ys)) >= 7
    assert ys[np.argmax(xs)] == ys.min() and ys[np.argmin(xs)] == ys.max()
    assert np.all((xs - xs.mean()) + (ys - ys.mean()) == 0)           # rows grow downwards: x + y constant
    ys, xs = _lit(P.draw_ticks(frame, _cells(0.0, -0.5), 16))         # U < 0: the other diagonal
    assert ys[np.argmax(xs)] == ys.max()
    assert not frame.any()                                             # a copy is drawn on
    assert not P.draw_ticks(frame, _cells(0.0, 0.0), 16).any() and not P.draw_ticks(frame, np.zeros((3, 3, 3)), 16).any()
    # length is proportional to sqrt(Q^2 + U^2) / I_max
    c = np.zeros((1, 2, 3))
    c[0, 0], c[0, 1] = (1.0, 0.6, 0.0), (0.5, 0.3, 0.0)
    ys, xs = _lit(P.draw_ticks(np.zeros((16, 32, 3), dtype=np.uint8), c, 16))
    left, right = (xs < 16).sum(), (xs >= 16).sum()
    assert left > right >= 0.4 * left
    # an edge cell is drawn about the centre of the pixels it has
    ys, xs = _lit(P.draw_ticks(np.zeros((8, 20, 3), dtype=np.uint8), np.array([[(1.0, 0.0, 0.0), (1.0, 0.5, 0.0)]]), 16))
    assert xs.min() == 10 and xs.max() == 19 and set(ys) == {4}      # 17.5 -/+ 7.2, cut by the frame; row 3.5 rounds to even


def test_degree_and_angle():
    from bhr_amd import polarization as P
    deg, chi = P.degree_and_angle([2.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, -0.5, 0.0])
    assert np.allclose(deg, [0.5, 0.5, 0.0]) and np.allclose(chi[:2], [0.0, -np.pi / 4])


def test_write_stokes_round_trip(tmp_path):
    from bhr_amd import polarization as P
    rng = np.random.default_rng(0)
    cells = rng.uniform(size=(4, 7, 3)).astype(np.float32)
    planes = rng.uniform(size=(3, 55, 97)).astype(np.float32)
    path = str(tmp_path / "s.npz")
    P.write_stokes(path, cells, 16, "toroidal", 0.7, camera=dict(cam_pos=[6, 0, 0.5], fov=90.0), stokes=planes)
    with np.load(path) as z:
        assert (z["cells"] == cells).all() and (z["I"] == planes[0]).all() and (z["Q"] == planes[1]).all() and (z["U"] == planes[2]).all()
        assert int(z["cell"]) == 16 and tuple(z["field"]) == (0.0, 1.0, 0.0) and float(z["fraction"]) == 0.7
        assert str(z["convention"]) == P.CONVENTION and "image-right" in P.CONVENTION and "IAU" in P.CONVENTION
        assert tuple(z["cam_pos"]) == (6.0, 0.0, 0.5) and float(z["fov"]) == 90.0
    stack = rng.uniform(size=(4, 3, 5, 3)).astype(np.float32)
    P.write_stokes(path, stack, 8, (0.3, 0.8, 0.5), 1.0)
    with np.load(path) as z:
        assert z["cells"].shape == (4, 3, 5, 3) and "I" not in z.files and "cam_pos" not in z.files
    with pytest.raises(ValueError, match="npz"):
        P.write_stokes(str(tmp_path / "s.txt"), cells, 16, "toroidal", 0.7)


def test_check_and_presets():
    from bhr_amd import polarization as P
    assert P.PRESETS == {"toroidal": (0.0, 1.0, 0.0), "radial": (1.0, 0.0, 0.0), "vertical": (0.0, 0.0, 1.0)}
    assert P.check("toroidal") == {"field": (0.0, 1.0, 0.0), "fraction": 0.7, "cell": 16}
    assert P.check((0.3, 0.8, 0.5), 1.0, 8) == {"field": (0.3, 0.8, 0.5), "fraction": 1.0, "cell": 8}
    assert P.parse_field(["radial"]) == (1.0, 0.0, 0.0) and P.parse_field(["0.3", "0.8", "0.5"]) == (0.3, 0.8, 0.5)
    for bad, word in ((dict(field="spiral"), "field"), (dict(field=(0, 0, 0)), "field"), (dict(field=(1, 2)), "three"),
                      (dict(field=(1, float("nan"), 0)), "field"), (dict(field="toroidal", fraction=1.5), "polarization_fraction"),
                      (dict(field="toroidal", fraction=float("nan")), "polarization_fraction"), (dict(field="toroidal", cell=12), "polarization_cell")):
        with pytest.raises(ValueError, match=word):
            P.check(**bad)
    with pytest.raises(ValueError, match="three"):
        P.parse_field(["1", "2"])
