// march_kerr_polar.hip -> march_kerr_polar.o: the Kerr polarisation's kernel (bhr_set_kerr_polarization; include/bhr.h states the
// model, DESIGN 4 "Kerr polarisation" derives it), in an object of its own with exactly the flags of march_kerr.o and
// march_kerr_raymap.o: kerr_shade_hit is inlined here as it is into the Kerr map's shade kernel, so the accumulator differences
// this kernel takes are differences of the values that kernel accumulated, bit for bit.
//
// kerr_raymap_stokes_kernel<RS> runs behind the shade and overflow launches of a frame from the Kerr ray map with
// kerr_raymap_shade_kernel's mapping -- a lane per pixel, an 8x8 tile per wave, tiles row-major -- and walks the lane's records
// front to back from the Shade Ray::init leaves.  Around each kerr_shade_hit it takes what the crossing added to the accumulator
// (its Rec. 709 luma is the crossing's weight c_k) and carries the polarisation from the gas to the camera by the Walker-Penrose
// constant, which has a closed form in the march's own Kerr-Schild chart: for a photon k^mu and a polarisation f^mu parallel-
// transported along it,
//   kappa1 = k^t (x.f) - f^t (x.k) + a (k^x f^y - k^y f^x),   kappa2 = x.(k x f) - a (k^t f^z - k^z f^t)
// (bold: the spatial Kerr-Schild components, Euclidean dot and cross) are conserved; they are bilinear and antisymmetric in
// (k, f), so f -> f + alpha k changes nothing and no gauge is fixed.  No integration, no Boyer-Lindquist transform, no
// trigonometric call.  Per record the kernel builds the gas's tetrad at the hit (Gram-Schmidt under g = eta + f l l from the
// gas's 4-velocity of the redshift mode), the photon's direction in it, the electric vector across the field, kappa of that;
// the camera's side -- p_c, the two lifted image axes E_x, E_y and their kappa's -- is computed once per lane ahead of the loop,
// and the record's tick is the solution (alpha, beta) of alpha kappa(E_x) + beta kappa(E_y) = kappa_em.  Field, Pi_0 and a are
// kernel arguments (scalars).  Three planar f32 stores, pixel index j W + i as the map's own.
//
// The traced photon runs from the camera to the gas (ray_kerr.h: the time-reversed picture, in which the gas turns in the +phi
// sense); a polarisation is a line, so the reversal, which flips k and leaves the spatial parts of f and the tetrad alone,
// changes nothing of it.  e_phi points along the disk's v_hat = r_hat x n as the Schwarzschild pass's does.
//
// The cell means are march_polar.hip's stokes_cells_kernel over the same planes.  kerr_shade_hit, the g-factors and Ray are
// called, not edited: no other object's code moves.
#include <type_traits>

#include "ray_kerr.h"

namespace {

template <int RS>
using KerrBlock = std::conditional_t<RS == KERR_EXACT, BhrKerrExactMarchArgs, BhrKerrMarchArgs>;

// a vector in the disk plane's tangent space without its z part: contravariant (t, x, y)
struct P3 {
    float t, x, y;
};
__device__ __forceinline__ P3 p3(float t, float x, float y) {
    P3 v;
    v.t = t;
    v.x = x;
    v.y = y;
    return v;
}
__device__ __forceinline__ P3 axpy(float s, P3 a, P3 b) { return p3(fmaf(s, a.t, b.t), fmaf(s, a.x, b.x), fmaf(s, a.y, b.y)); }
// g = eta + f l l at a point of the plane z = 0 (l_t = 1, l_z = 0), on two such vectors
struct PlaneMetric {
    float f, lx, ly;
};
__device__ __forceinline__ float gdot(const PlaneMetric &g, P3 a, P3 b) {
    const float la = a.t + (g.lx * a.x + g.ly * a.y), lb = b.t + (g.lx * b.x + g.ly * b.y);
    return (a.x * b.x + a.y * b.y - a.t * b.t) + g.f * (la * lb);
}
__device__ __forceinline__ P3 gunit(const PlaneMetric &g, P3 a) {
    const float s = 1.0f / sqrtf(gdot(g, a, a));
    return p3(s * a.t, s * a.x, s * a.y);
}

// the two conserved numbers of (k, f) at the point x; k = (kt, kv), f = (ft, fv) contravariant
__device__ __forceinline__ void walker_penrose(float a, V3 x, float kt, V3 kv, float ft, V3 fv, float &k1, float &k2) {
    k1 = (kt * dot(x, fv) - ft * dot(x, kv)) + a * (kv.x * fv.y - kv.y * fv.x);
    k2 = dot(x, cross(kv, fv)) - a * (kt * fv.z - kv.z * ft);
}

// The gas's 4-velocity at the hit (hx, hy, 0) of Boyer-Lindquist radius r, in the traced picture (+phi), as (t, x, y).
//   model  the g-factor model's gas: the speed beta = min(r_s Omega / sqrt(1 - 1 / r_s), 0.99) of Kerr's Omega at r_s =
//          max(r, 1 + 1e-3), along the orbit, as the static observer at the hit sees it: u = gamma (u_s + beta e), u_s = d_t /
//          sqrt(1 - f), e the unit vector along d_phi orthogonal to u_s.  At a = 0 it is the Schwarzschild pass's gas.
//   exact  kerr_g_exact's gas: the circular geodesic of Kerr's Omega outside the ISCO, the plunge that keeps the ISCO's E and L
//          inside it (ray_kerr.h states both), raised to contravariant components.
template <int RS>
__device__ __forceinline__ P3 gas_velocity(const BhrMarchArgs &a, const PlaneMetric &g, float hx, float hy, float r, float rho2, float irho) {
    const float ka = kerr(a).kerr_a;
    if (RS == KERR_EXACT) {
        const BhrKerrExactMarchArgs &k = kerr_exact(a);
        if (r >= k.isco_r) {
            const float om = kerr_omega(r, ka);
            const float q = 1.0f - ka * om;
            const float ut = 1.0f / sqrtf(fmaxf(1.0f - om * om * rho2 - q * q / r, 1e-6f));
            return p3(ut, -(ut * om) * hy, (ut * om) * hx);
        }
        const float E = k.isco_e, L = k.isco_l;
        const float rho = sqrtf(rho2);
        const float c0 = E - ka * L / rho2;
        const float qa = 1.0f - r / rho2;
        const float qb = -2.0f * c0 / rho;
        const float dr = fmaxf(k.isco_r - r, 0.0f);
        const float disc = 4.0f * ((1.0f - E) * (1.0f + E)) * (dr * dr * dr) / (r * rho2);
        const float w = (-qb - sqrtf(disc)) / (2.0f * qa);
        const float S = c0 + r * w / rho;
        const float lr = L / rho2, wr = w * irho, fs = g.f * S;
        return p3(E + fs, (wr * hx - lr * hy) - fs * g.lx, (wr * hy + lr * hx) - fs * g.ly);
    }
    const float r_safe = fmaxf(r, BHR_RS + 1e-3f);
    const float omega = kerr_omega(r_safe, ka);
    const float lorentz = sqrtf(fmaxf(1.0f - BHR_RS / r_safe, 1e-6f));
    const float beta = fminf(r_safe * omega / fmaxf(lorentz, 1e-6f), 0.99f);
    const float gamma = 1.0f / sqrtf(fmaxf(1.0f - beta * beta, 1e-6f));
    const P3 us = p3(1.0f / sqrtf(fmaxf(1.0f - g.f, 1e-6f)), 0.0f, 0.0f);
    const P3 m = p3(0.0f, -hy * irho, hx * irho);
    const P3 e = gunit(g, axpy(gdot(g, m, us), us, m));
    return p3(gamma * (us.t + beta * e.t), gamma * (beta * e.x), gamma * (beta * e.y));
}

template <int RS>
__global__ __launch_bounds__(256) void kerr_raymap_stokes_kernel(KerrBlock<RS> a, BhrRayMapMomArgs m, BhrStokesArgs s) {
    const int tile = wave_slot();
    if (tile >= a.n_tiles) return;
    const int lane = threadIdx.x & 63;
    const int i = (tile % a.tiles_x) * 8 + (lane & 7);
    const int j = (tile / a.tiles_x) * 8 + (lane >> 3);
    if (!(i < a.width && j < a.rows)) return;
    const size_t pix = (size_t)j * a.width + i;
    const size_t p = (size_t)m.plane;
    const int count = m.crossings[pix];
    float sI = 0.0f, sQ = 0.0f, sU = 0.0f;
    if (count <= m.slots) {          // a pixel on the overflow list keeps the zeros
        const float ka = kerr(a).kerr_a, a2 = ka * ka;
        // the camera's side, once: the photon Ray::init launches (its closed form), the image axes lifted to vectors
        // g-orthogonal to it, E = (p_c . e, e), and their kappa's
        const V3 C = ld3(a.cp);
        V3 unused_x, unused_y;
        const V3 D = pixel_ray<false>(a, i, j, unused_x, unused_y);
        float k1x, k2x, k1y, k2y;
        {
            const float w = dot(C, C) - a2;
            const float S = sqrtf(w * w + 4.0f * a2 * (C.z * C.z));
            const float r2 = 0.5f * (w + S);
            const float r = sqrtf(r2);
            const float f = r / S, Q = r2 + a2;
            const V3 l = mk((r * C.x + ka * C.y) / Q, (r * C.y - ka * C.x) / Q, C.z / r);
            const float c = dot(l, D);
            const float sc = 1.0f / sqrtf(1.0f - f * (1.0f - c * c));
            const float lam = (1.0f + sc * c) / (1.0f - f);
            const float fl = f * lam;
            const V3 pc = mk(sc * D.x + fl * l.x, sc * D.y + fl * l.y, sc * D.z + fl * l.z);
            const float kt = 1.0f + fl;
            const V3 kv = sc * D;
            const V3 R = ld3(a.cr);
            const V3 ex = normalized(R - dot(R, D) * D);
            V3 ey = cross(D, ex);
            if (dot(ey, ld3(a.cu)) < 0.0f) ey = mk(-ey.x, -ey.y, -ey.z);
            walker_penrose(ka, C, kt, kv, dot(pc, ex), ex, k1x, k2x);
            walker_penrose(ka, C, kt, kv, dot(pc, ey), ey, k1y, k2y);
        }
        const float det = k1x * k2y - k1y * k2x;
        const bool cam_ok = det * det > 0.0f;    // the radial ray of a hole that does not spin has none: I only

        Shade sh;                    // as Ray::init leaves it
        sh.accum = mk(0, 0, 0);
        sh.alpha_total = 0.0f;
        sh.unsure = 0;
        for (int c = 0; c < count; ++c) {
            const float *q = m.hits + (size_t)c * m.comps * p + pix;
            const float hx = q[0], hy = q[p];
            const V3 to_cam = mk(q[2 * p], q[3 * p], q[4 * p]);
            const float *qm = m.mom + (size_t)c * 3 * p + pix;
            const V3 ph = mk(qm[0], qm[p], qm[2 * p]);
            const V3 before = sh.accum;
            kerr_shade_hit<RS>(a, sh, hx, hy, to_cam);
            const V3 add = sh.accum - before;
            const float ck = 0.2126f * add.x + 0.7152f * add.y + 0.0722f * add.z;
            sI = sI + ck;
            // kerr_shade_hit's own test: outside the annulus it returned early and the crossing adds nothing
            const float r = sqrtf(hx * hx + hy * hy - ka * ka);
            if (!cam_ok || !(a.r_outer >= r && r >= a.r_inner)) continue;

            // the metric in the plane: f = 1 / r, l = ((r x + a y) / Q, (r y - a x) / Q, 0), Q = x^2 + y^2
            const float rho2 = hx * hx + hy * hy;
            const float irho = 1.0f / sqrtf(rho2);
            PlaneMetric g;
            g.f = 1.0f / r;
            g.lx = (r * hx + ka * hy) / rho2;
            g.ly = (r * hy - ka * hx) / rho2;
            // the gas and its tetrad: u, then e_phi along v_hat, then e_z = d_z (unit and orthogonal already), then e_r outwards
            const P3 u = gas_velocity<RS>(a, g, hx, hy, r, rho2, irho);
            const P3 vh = p3(0.0f, hy * irho, -hx * irho);
            const P3 ep = gunit(g, axpy(gdot(g, vh, u), u, vh));
            const P3 rh = p3(0.0f, hx * irho, hy * irho);
            const P3 er = gunit(g, axpy(-gdot(g, rh, ep), ep, axpy(gdot(g, rh, u), u, rh)));
            // the photon's direction in the gas frame: n'_(i) = (k . e_(i)) / (-k . u), with k_mu = (-1, ph)
            const float inu = 1.0f / (u.t - (ph.x * u.x + ph.y * u.y));
            // (a unit vector for a null k; the record's momentum is interpolated across its step and is null to second order in
            // it only, so the direction is normalized: the polarised weight then stays within Pi_0)
            const V3 np = normalized(mk(((ph.x * er.x + ph.y * er.y) - er.t) * inu, ((ph.x * ep.x + ph.y * ep.y) - ep.t) * inu, ph.z * inu));
            // the field and the electric vector, in tetrad components (r, phi, z)
            const V3 e = cross(np, mk(s.b[0], s.b[1], s.b[2]));
            const float s2 = dot(e, e);
            if (!(s2 > 0.0f)) continue;
            const V3 eh = (1.0f / sqrtf(s2)) * e;
            // f_em = e_hat^(i) e_(i), and the photon's contravariant k = (1 + f U, ph - f U l), U = 1 + l . ph
            const float ft = eh.x * er.t + eh.y * ep.t;
            const V3 fv = mk(eh.x * er.x + eh.y * ep.x, eh.x * er.y + eh.y * ep.y, eh.z);
            const float fU = g.f * (1.0f + (g.lx * ph.x + g.ly * ph.y));
            float k1, k2;
            walker_penrose(ka, mk(hx, hy, 0.0f), 1.0f + fU, mk(ph.x - fU * g.lx, ph.y - fU * g.ly, ph.z), ft, fv, k1, k2);
            // alpha kappa(E_x) + beta kappa(E_y) = kappa_em, up to the common factor 1 / det (a tick is a line)
            const float x = k1 * k2y - k1y * k2, y = k1x * k2 - k1 * k2x;
            const float den = x * x + y * y;
            if (!(den > 0.0f)) continue;
            const float wgt = s.frac * s2 * ck;
            sQ = sQ + wgt * ((x * x - y * y) / den);
            sU = sU + wgt * ((2.0f * x * y) / den);
        }
    }
    s.out[pix] = sI;
    s.out[p + pix] = sQ;
    s.out[2 * p + pix] = sU;
}

}  // namespace

const void *bhr_kerr_stokes_kernel(int32_t exact) {
    return exact ? (const void *)kerr_raymap_stokes_kernel<KERR_EXACT> : (const void *)kerr_raymap_stokes_kernel<0>;
}
