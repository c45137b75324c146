// ray_strict.h -- the strict Ray of the march (march_strict.o, march_strict_ilp.o, march_raymap.o, under ray_observer.h
// march_observer.o and under ray_delay.h march_delay.o; see march_device.h).
#pragma once
#define BHR_RAY_STRICT 1
#include "march_device.h"

namespace {

// =============================================================================
// strict build: render.py:2854-3006 operation by operation, 3-D state
// =============================================================================
template <bool DIFF, int SRC = 0>
struct StrictRay {
    V3 p, d;
    float m15L2;   // -1.5 * L2
    float r;       // |p|
    float r2p;     // |p|^2
    float f_old;   // plane function at p
    float affine;
    Shade sh;
    int n_pend;    // parked disk crossings (0..2), in the lane's LDS slots, oldest first
    int step_count;
    int pix;       // linear pixel index inside the row block, -1 = lane has no ray
    int done;      // 0 running, 2 captured or escaped (escaped() tells), 3 ran out of iterations, 4 empty lane
    bool full;     // wave-uniform: some live lane has both its parking slots occupied
    V3 dpx, ddx, dpy, ddy;   // ray differentials (DIFF only)

    __device__ __forceinline__ void init(const BhrMarchArgs &a, int i, int j_local) {
        init_along(a, pixel_ray<DIFF>(a, i, j_local, ddx, ddy), i, j_local);
    }
    // the ray of pixel (i, j_local) leaves the camera along ray_dir (ray_observer.h: a moving observer's is not the pixel's own)
    __device__ __forceinline__ void init_along(const BhrMarchArgs &a, V3 ray_dir, int i, int j_local) {
        p = ld3(a.cp);
        d = ray_dir;
        V3 Lv = cross(d, p);
        float Ln = sqrtf(dot(Lv, Lv));
        m15L2 = -1.5f * (Ln * Ln);
        r2p = dot(p, p);
        r = sqrtf(r2p);
        f_old = p.z - p.y * a.tan_t;
        affine = 0.0f;
        sh.accum = mk(0, 0, 0);
        sh.alpha_total = 0.0f;
        sh.unsure = 0;
        n_pend = 0;
        full = false;
        step_count = 0;
        done = a.max_iter <= 0 ? 3 : 0;
        pix = j_local * a.width + i;
        if (DIFF) {
            dpx = mk(0, 0, 0);
            dpy = mk(0, 0, 0);
        }
    }

    // a(s) = (-1.5 L2 / r^5) s with r = sqrt(s.s), r^5 = (r2 r2) r     (render.py:2518-2524)
    __device__ __forceinline__ float coef(float r2, float rr) const { return div_rn(m15L2, r2 * r2 * rr); }
    // factor (d_pos - 5 pos proj), proj = pos.d_pos / r2                  (render.py:2526-2539)
    __device__ __forceinline__ V3 jac(V3 s, V3 dl, float factor, float r2) const {
        float proj = div_rn(dot(s, dl), r2);
        return factor * mk(dl.x - 5.0f * s.x * proj, dl.y - 5.0f * s.y * proj, dl.z - 5.0f * s.z * proj);
    }
    __device__ __forceinline__ V3 rk_sum(V3 k1, V3 k2, V3 k3, V3 k4) const {   // (k1 + 2 k2 + 2 k3 + k4) / 6
        // 2 k is exact, so fma(2, k2, k1) == k1 + 2 k2 rounded once, as in the reference
        return mk(div6(fmaf(2.0f, k3.x, fmaf(2.0f, k2.x, k1.x)) + k4.x), div6(fmaf(2.0f, k3.y, fmaf(2.0f, k2.y, k1.y)) + k4.y),
                  div6(fmaf(2.0f, k3.z, fmaf(2.0f, k2.z, k1.z)) + k4.z));
    }

    // One iteration of the while-loop at render.py:2854-3006.  The state is committed unconditionally: a lane whose ray
    // has terminated leaves the loop and never reads it again (escaped rays read d = new_dir), and with two parking slots
    // in LDS a hit always finds room, with or without differentials.  (Until round 2 the AA kernel kept ONE slot in
    // registers and repeated the step of a lane that found it occupied; under the ILP scheduler at 4 waves per SIMD the
    // LDS scheme is 3 % faster -- 4k AA 6.44 -> 6.26 ms, same pixels -- and the redo path is gone.)
    __device__ __forceinline__ bool step(const BhrMarchArgs &a) {
        // clamps as single v_med3 / v_min instructions (no NaN can reach them: r is a finite norm); the C forms cost a
        // canonicalising v_max, and compare + select pairs
        float r_safe;                                    // max(r, r_cap + 1e-3) without the canonicalising second v_max
        asm("v_max_f32 %0, %1, %2" : "=v"(r_safe) : "v"(r), "v"(BHR_RS + 1e-3f));
        // The eleven hardware approximations of a step (five v_rsq for the exact square roots, six v_rcp for the exact
        // quotients) in six groups of independent operands, back to back (round 4; sqrt_rn_s / div_rn_s: the same
        // refinements on the same seeds, every value bit for bit what the one-at-a-time order gives).
        const float den1 = r2p * r2p * r;                // r^5 of coef(r2p, r)
        float y_s, y_q, y_1;
        rsq_rcp_rcp(r_safe, den1, y_s, y_q, y_1);
        float far_scale = __builtin_fminf(sqrt_rn_s(r_safe, y_s), 10.0f);   // sqrt(r_safe / r_cap), r_cap = 1; capped at max_fac
        float q = rcp_rn_s(r_safe, y_q);                 // r_cap / r_safe, r_cap = 1
        float near_damp = rcp_rn(fmaf(2.0f, q * q * q, 1.0f));   // 2 x is exact: one rounding, as 1 + 2 x has
        float dt_fac = __builtin_amdgcn_fmed3f(far_scale * near_damp, 0.2f, 10.0f);   // render.py:2865-2868
        float h = a.h_base * dt_fac;

        float f1 = div_rn_s(m15L2, den1, y_1);
        V3 k1p = h * d;
        V3 k1d = h * (f1 * p);
        V3 s2 = add_half(p, k1p);
        float r2_2 = dot(s2, s2);
        V3 k2p = h * add_half(d, k1d);
        V3 s3 = add_half(p, k2p);
        float r2_3 = dot(s3, s3);
        float y_2, y_3;
        rsq2(r2_2, r2_3, y_2, y_3);
        const float den2 = r2_2 * r2_2 * sqrt_rn_s(r2_2, y_2), den3 = r2_3 * r2_3 * sqrt_rn_s(r2_3, y_3);
        rcp2(den2, den3, y_2, y_3);
        float f2 = div_rn_s(m15L2, den2, y_2);
        float f3 = div_rn_s(m15L2, den3, y_3);
        V3 k2d = h * (f2 * s2);
        V3 k3p = h * add_half(d, k2d);
        V3 k3d = h * (f3 * s3);
        V3 s4 = p + k3p;
        float r2_4 = dot(s4, s4);
        V3 k4p = h * (d + k3d);
        V3 np = p + rk_sum(k1p, k2p, k3p, k4p);
        float r2n = dot(np, np);
        float y_4, y_n;
        rsq2(r2_4, r2n, y_4, y_n);
        float f4 = coef(r2_4, sqrt_rn_s(r2_4, y_4));
        float rn = sqrt_rn_s(r2n, y_n);
        V3 k4d = h * (f4 * s4);
        V3 nd = d + rk_sum(k1d, k2d, k3d, k4d);

        V3 ndpx, nddx, ndpy, nddy;
        if (DIFF) {
            {
                V3 a1p = h * ddx;
                V3 a1d = h * jac(p, dpx, f1, r2p);
                V3 a2p = h * add_half(ddx, a1d);
                V3 a2d = h * jac(s2, add_half(dpx, a1p), f2, r2_2);
                V3 a3p = h * add_half(ddx, a2d);
                V3 a3d = h * jac(s3, add_half(dpx, a2p), f3, r2_3);
                V3 a4p = h * (ddx + a3d);
                V3 a4d = h * jac(s4, dpx + a3p, f4, r2_4);
                ndpx = dpx + rk_sum(a1p, a2p, a3p, a4p);
                nddx = ddx + rk_sum(a1d, a2d, a3d, a4d);
            }
            {
                V3 a1p = h * ddy;
                V3 a1d = h * jac(p, dpy, f1, r2p);
                V3 a2p = h * add_half(ddy, a1d);
                V3 a2d = h * jac(s2, add_half(dpy, a1p), f2, r2_2);
                V3 a3p = h * add_half(ddy, a2d);
                V3 a3d = h * jac(s3, add_half(dpy, a2p), f3, r2_3);
                V3 a4p = h * (ddy + a3d);
                V3 a4d = h * jac(s4, dpy + a3p, f4, r2_4);
                ndpy = dpy + rk_sum(a1p, a2p, a3p, a4p);
                nddy = ddy + rk_sum(a1d, a2d, a3d, a4d);
            }
        }

        float aff = affine + h;
        // termination precedes the plane test (render.py:2916-2926): the ray goes on iff r_s <= |new_pos| <= r_escape and the
        // affine parameter is within its limit -- the reference's strict inequalities, the two radii as one v_med3 + one
        // compare (which of them ended the ray: escaped(), behind the loop)
        const bool ended = __builtin_amdgcn_fmed3f(rn, BHR_RS, a.r_esc) != rn || aff > a.max_affine;
        const bool alive = !ended;
        float f_new = np.z - np.y * a.tan_t;
        const bool crossing = f_old * f_new < 0;
        if (SRC == 2) {
            if (alive) volume_segment(a, sh, p, np, d, f_old, f_new, r, rn);
        } else if (__builtin_amdgcn_ballot_w64(crossing) != 0ull) {
            // a wave-uniform branch around the crossing code (a few steps per ray): `full` is a uniform value set under uniform
            // control and lives in a scalar register -- the march loop tests it instead of comparing n_pend in every step
            if (alive && crossing) {
                float t_frac = div_rn(f_old, f_old - f_new + 1e-8f);
                float hx = p.x + t_frac * (np.x - p.x);
                float hy = p.y + t_frac * (np.y - p.y);
                float hit_r = sqrt_rn(hx * hx + hy * hy);
                if (a.r_outer >= hit_r && hit_r >= a.r_inner) {   // render.py:2951
                    Pending<DIFF> h;
                    h.hit_x = hx;
                    h.hit_y = hy;
                    h.to_cam = mk(-d.x, -d.y, -d.z);              // direction at the START of the step (render.py:2954)
                    // the differentials were committed BEFORE the hit interpolation (render.py:2928-2932),
                    // hence hit_d_pos == new_d_pos in render.py:2947-2949
                    if (DIFF) { h.dxx = ndpx.x; h.dxy = ndpx.y; h.dyx = ndpy.x; h.dyy = ndpy.y; }
                    park_store<DIFF>(n_pend, h);                  // a free slot is guaranteed (march_tile_body flushes at 2)
                    n_pend += 1;
                }
            }
            full = __builtin_amdgcn_ballot_w64(n_pend == 2) != 0ull;
        }
        affine = aff;
        if (DIFF) { dpx = ndpx; ddx = nddx; dpy = ndpy; ddy = nddy; }
        p = np;
        d = nd;
        r = rn;
        r2p = r2n;
        f_old = f_new;
        step_count += 1;
        done = ended ? 2 : (step_count >= a.max_iter ? 3 : 0);
        return true;
    }

    // The loop's own termination test once more, on the state a finished lane is left with (r = |p| and the affine parameter
    // are those very values): the tile kernels call it behind the march loop instead of reading `done` back (see the fast
    // Ray's settle()).
    __device__ __forceinline__ void settle(const BhrMarchArgs &a) {
        done = (__builtin_amdgcn_fmed3f(r, BHR_RS, a.r_esc) != r || affine > a.max_affine) ? 2 : 3;
    }
    __device__ __forceinline__ bool escaped() const { return done == 2 && !(r < BHR_RS); }

    // shade the oldest parked crossing (lanes that have one), the second slot moves up
    __device__ __forceinline__ void flush_one(const BhrMarchArgs &a) {
        if (n_pend > 0) {
            const Pending<DIFF> h = park_pop<DIFF>(n_pend);
            shade_hit<DIFF, SRC>(a, sh, h.hit_x, h.hit_y, h.to_cam, h.dxx, h.dxy, h.dyx, h.dyy);
        }
    }
    // The ray map's build (march_raymap.hip) in flush_one's place: the oldest parked crossing goes, exactly as parked, into the next
    // map slot of the lane's pixel `at` instead of being shaded; n_rec counts the pixel's crossings past the slots.
    __device__ __forceinline__ void record_one(const BhrRayMapArgs &m, size_t at, int &n_rec) {
        if (n_pend > 0) {
            const Pending<DIFF> h = park_pop<DIFF>(n_pend);
            if (n_rec < m.slots) {
                const size_t p = (size_t)m.plane;
                float *q = m.hits + (size_t)n_rec * m.comps * p + at;
                q[0] = h.hit_x;
                q[p] = h.hit_y;
                q[2 * p] = h.to_cam.x;
                q[3 * p] = h.to_cam.y;
                q[4 * p] = h.to_cam.z;
                if (DIFF) {
                    q[5 * p] = h.dxx;
                    q[6 * p] = h.dxy;
                    q[7 * p] = h.dyx;
                    q[8 * p] = h.dyy;
                }
            }
            n_rec += 1;
        }
    }
    __device__ __forceinline__ void finish(const BhrMarchArgs &a) { write_pixel(a, pix % a.width, pix / a.width, escaped(), d, sh); }
    __device__ __forceinline__ void finish_at(const BhrMarchArgs &a, int i, int j) { write_pixel(a, i, j, escaped(), d, sh); }
    __device__ __forceinline__ void values(const BhrMarchArgs &a, float bk[3], float dk[3]) const { pixel_values(a, escaped(), d, sh, bk, dk); }
};

// The Ray the schedules march (march_tile.h, march_persistent.h): the strict one itself, unless the Ray header that included
// this file derives its own from it (ray_observer.h, ray_delay.h).
#ifndef BHR_RAY_OBSERVER
template <bool DIFF, int SRC = 0>
using Ray = StrictRay<DIFF, SRC>;
#endif

}  // namespace
