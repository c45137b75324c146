// ray_delay.h -- the delayed Ray of the march (march_delay.o; see march_device.h): the strict Ray that also keeps the coordinate
// time its light has travelled, so that every disk crossing is shaded at the time the light LEFT the gas (bhr_render_delayed).
//
// Units: r_s = 1, c = 1.  The strict march integrates x'' = -1.5 L^2 x / r^5 with |d| = 1 at the camera.  Along that parameter l a
// Schwarzschild null geodesic has u = 1/r obeying (du/dphi)^2 = 1/b^2 - u^2 (1 - u), dphi/dl = L u^2 and dt/dphi = 1 / (b u^2 (1 - u)),
// with L^2 = |d x p|^2 at launch and b = L / E, hence
//   E     = sqrt(1 - L^2 / r_cam^3)         from |d| = 1 at the camera: 1 = (dr/dl)^2 + L^2 / r^2 = E^2 + L^2 / r^3 there
//   dt/dl = E w(r),   w(r) = r / (r - 1)
// E is 1 for a radial ray and falls with the impact parameter; tests/test_delay_ref.py holds dt/dl against an independent
// integration of the four-dimensional geodesic.
//
// Every operation below is f32, rounded once, with no contraction (the strict objects' flags); sqrt and the quotients are the
// correctly rounded sequences of march_device.h (sqrt_rn, div_rn).
//   launch     L2 = Ln * Ln with Ln = sqrtf(|d x p|^2) (the strict Ray's own), r3 = r2p * r,
//              E = sqrt_rn(1 - div_rn(L2, r3)),  w = wr(r),  T = 0
//   wr(r)      rs = max(r, 1 + 1e-3)  (the march's r_safe);  wr = div_rn(rs, rs - 1)
//   step       from (p, d, r) to (np, nd, rn) under the step's own h (the strict Ray's, recomputed from r: the same operations on
//              the same values):
//              m  = (0.5 (p + np)) + (0.125 h) (d - nd)   per component: RN(RN(0.5 RN(p + np)) + RN(RN(0.125 h) RN(d - nd)))
//              rm = sqrt_rn((m.x m.x + m.y m.y) + m.z m.z)
//              s  = (w + 4 wr(rm)) + wr(rn)               4 x exact
//              dT = (E * div6(h)) * s
//   crossing   a crossing the strict step parked: t_frac = div_rn(f_old, f_old - f_new + 1e-8f), the strict step's own bits;
//              T_hit = T + t_frac * dT, stored beside the parked crossing (word 5 of its LDS slot, which the strict Ray without
//              differentials leaves unused)
//   commit     T = T + dT,  w = wr(rn)
//   shade      t_eff = t_offset - scale * T_hit, RN(t_offset - RN(scale T_hit)); shade_hit as ever, reading t_eff and cp through a
//              lane-local frame block (march_device.h: "ONLY f.t_offset and f.cp may be read through f")
// scale = 0 gives t_eff = t_offset exactly (T_hit is finite: w <= 1001, h <= 10 h_base) and so the strict frame bit for bit;
// redshift, brightness, alpha, the sky, the step counts and termination never see T.
//
// A step costs one rsq-class and two rcp-class hardware approximations on top of the strict step's eleven.  T, E and w are three
// more values alive across the march loop.  No ray differentials (word 5 .. 8 of a slot are theirs) and the texture source only.
#pragma once
#define BHR_RAY_OBSERVER 1   // ray_strict.h: the schedules' Ray is the one below, derived from the strict one
#include "ray_strict.h"

namespace {

// The kernels of this object take the march's block with the scale behind it (bhr_internal.h: BhrDelayMarchArgs) and hand it to the
// shared schedule as the BhrMarchArgs it is; the delay code reads the tail through this.
__device__ __forceinline__ const BhrDelayMarchArgs &delay(const BhrMarchArgs &a) { return static_cast<const BhrDelayMarchArgs &>(a); }

template <bool DIFF, int SRC = 0>
struct DelayRay : StrictRay<DIFF, SRC> {
    static_assert(!DIFF && SRC == 0, "the delayed march has no ray differentials and the texture source only");
    typedef StrictRay<DIFF, SRC> Base;
    float T;     // coordinate time from the camera to p, along the ray
    float E;     // the ray's energy per unit of the march's parameter
    float w;     // wr(r) of the current r

    static __device__ __forceinline__ float wr(float r) {
        const float rs = fmaxf(r, BHR_RS + 1e-3f);
        return div_rn(rs, rs - 1.0f);
    }

    __device__ __forceinline__ void init(const BhrMarchArgs &a, int i, int j_local) {
        V3 unused_x, unused_y;
        init_along(a, pixel_ray<false>(a, i, j_local, unused_x, unused_y), i, j_local);
    }
    __device__ __forceinline__ void init_along(const BhrMarchArgs &a, V3 ray_dir, int i, int j_local) {
        Base::init_along(a, ray_dir, i, j_local);
        const V3 Lv = cross(this->d, this->p);
        const float Ln = sqrtf(dot(Lv, Lv));
        // L^2 / r^3 <= 1 / r_cam < 1 for a unit d outside the horizon: the root's argument is a positive normal number
        E = sqrt_rn(1.0f - div_rn(Ln * Ln, this->r2p * this->r));
        w = wr(this->r);
        T = 0.0f;
    }

    // the strict step, then the time it took: Simpson's rule over the step with the Hermite midpoint
    __device__ __forceinline__ bool step(const BhrMarchArgs &a) {
        const V3 p0 = this->p, d0 = this->d;
        const float r0 = this->r, f0 = this->f_old;
        const int n0 = this->n_pend;
        // h of this step: the strict step's own sequence on the same r (the compiler folds the two)
        float r_safe;
        asm("v_max_f32 %0, %1, %2" : "=v"(r_safe) : "v"(r0), "v"(BHR_RS + 1e-3f));
        const float den1 = this->r2p * this->r2p * r0;
        float y_s, y_q, y_1;
        rsq_rcp_rcp(r_safe, den1, y_s, y_q, y_1);
        const float far_scale = __builtin_fminf(sqrt_rn_s(r_safe, y_s), 10.0f);
        const float q = rcp_rn_s(r_safe, y_q);
        const float near_damp = rcp_rn(fmaf(2.0f, q * q * q, 1.0f));
        const float h = a.h_base * __builtin_amdgcn_fmed3f(far_scale * near_damp, 0.2f, 10.0f);

        Base::step(a);

        const float h8 = 0.125f * h;
        const V3 m = mk(0.5f * (p0.x + this->p.x) + h8 * (d0.x - this->d.x), 0.5f * (p0.y + this->p.y) + h8 * (d0.y - this->d.y),
                        0.5f * (p0.z + this->p.z) + h8 * (d0.z - this->d.z));
        const float rm = sqrt_rn(dot(m, m));
        const float wn = wr(this->r);
        const float dT = (E * div6(h)) * ((w + 4.0f * wr(rm)) + wn);
        if (this->n_pend != n0) {                 // the strict step parked a crossing in slot n0: its time goes beside it
            const float t_frac = div_rn(f0, f0 - this->f_old + 1e-8f);
            g_park[n0][5][threadIdx.x] = T + t_frac * dT;
        }
        T = T + dT;
        w = wn;
        return true;
    }

    // shade the oldest parked crossing at its emission time (the strict Ray's flush_one under t_eff)
    __device__ __forceinline__ void flush_one(const BhrMarchArgs &a) {
        if (this->n_pend > 0) {
            const int t = threadIdx.x;
            const float t_hit = g_park[0][5][t];
            if (this->n_pend == 2) g_park[0][5][t] = g_park[1][5][t];
            const Pending<false> h = park_pop<false>(this->n_pend);
            BhrMarchArgs f;                       // ONLY f.t_offset and f.cp are set, and only they are read (march_device.h: shade_hit)
            f.t_offset = a.t_offset - delay(a).delay_scale * t_hit;
            f.cp[0] = a.cp[0];
            f.cp[1] = a.cp[1];
            f.cp[2] = a.cp[2];
            shade_hit<false, 0>(a, f, this->sh, h.hit_x, h.hit_y, h.to_cam, h.dxx, h.dxy, h.dyx, h.dyy);
        }
    }
};

template <bool DIFF, int SRC = 0>
using Ray = DelayRay<DIFF, SRC>;

}  // namespace
