// ray_fast.h -- the fast Ray of the march (march.o; see march_device.h).
#pragma once
#define BHR_RAY_STRICT 0
#include "march_device.h"

namespace {

// =============================================================================
// fast build.  The force is central, so a ray never leaves the plane spanned by the camera
// position and its initial direction, and RK4 commutes with rotations: marching the 2-D state
// (U, W) in an orthonormal in-plane basis (g1, g2) visits exactly the reference's sequence of
// positions up to rounding, with a third fewer vector operations.  The basis is chosen per ray
// so that g1 is the line of nodes (orbital plane ^ disk plane): the disk-plane function
// z - y tan(tilt) = n.x then reduces to (n.g2) W, i.e. W is the scaled height above the disk and
// is SMALL where the crossing is detected -- the absolute precision of the crossing point is the
// same as with the reference's 3-D z coordinate (a basis tied to the camera direction loses a
// factor r/|z| there, measured as 2x the parity error).  Ray differentials split into an in-plane
// pair coupled through the projection term of the Jacobian and an out-of-plane component that
// sees only the isotropic term:  J d = c (d - 5 s (s.d)/r^2).
//
// The ray's own clock (round 4).  Every ray marches in an affine parameter of its own, lambda' = lambda / tau with
// tau^2 (1.5 L2) = 1: the equation of motion becomes u'' = -u / r^5 -- no coefficient to multiply in at the four radii of
// a step (c = -(1/r)^5 straight from the v_rsq) -- with velocities tau x direction and the step h_base dt_fac / tau (a
// per-lane factor in a vector register: a product with the scalar h_base issues at half rate).  RK4 is invariant
// under the rescaling, so the sequence of positions is the reference's up to rounding; tau carries a relative rounding
// error of ~1e-7 into the force constant, the size of the rounding of L2 itself.  Positions stay in r_s.
// =============================================================================
template <bool DIFF, int SRC = 0>
struct Ray {
    float u, w, du, dw;   // position / velocity (tau x direction) along (g1, g2)
    float hk;             // h_base / tau: step = dt_fac hk
    float ij;             // 1 / |(u, w)|
    float c1;             // acceleration coefficient at (u, w):  -1 / r^5
    float esc2;           // r_escape^2, in a vector register (an SGPR operand halves the v_med3's issue rate)
    float Bn;             // n . g2: the plane function z - y tan(tilt) is Bn w
    V3 g1, g2;            // in-plane orthonormal basis
    bool full;            // wave-uniform: some live lane has both its parking slots occupied
    float affine;         // in units of h_base
    Shade sh;
    int n_pend;    // parked disk crossings (0..2), in the lane's LDS slots, oldest first
    int step_count;
    int pix;
    int done;
    // differentials (DIFF only): components along (g1, g2, e3 = g1 x g2) of d_pos and d_dir
    V3 dpx, ddx, dpy, ddy;

    __device__ __forceinline__ void init(const BhrMarchArgs &a, int i, int j_local) {
        V3 gx, gy;
        V3 d0 = pixel_ray<DIFF>(a, i, j_local, gx, gy);
        const V3 p0 = ld3(a.cp);
        // L2 exactly as the reference forms it (render.py:2828)
        V3 Lv = cross(d0, p0);
        float L2 = dot(Lv, Lv);
        // tau = (1.5 L2)^(-1/2), v_rsq + one Newton step.  A radial ray (L2 -> 0: no deflection at all) marches with the
        // force of L2 ~ 1e-12: below the rounding of its velocity
        const float kap = fmaxf(1.5f * L2, 1e-12f);
        float tau = q_rsq(kap);
        tau = tau * fmaf(-0.5f * kap, tau * tau, 1.5f);
        hk = a.h_base * (kap * tau);
        // unit normal of the orbital plane; for a radial ray (L = 0) any direction orthogonal to p0
        V3 e3;
        if (L2 > 1e-20f) {
            e3 = (1.0f / sqrtf(L2)) * Lv;
        } else {
            V3 t = fabsf(p0.x) < 0.9f * a.r0 ? mk(1, 0, 0) : mk(0, 1, 0);
            V3 q = cross(p0, t);
            e3 = (1.0f / sqrtf(dot(q, q))) * q;
        }
        // g2 = in-plane part of the disk-plane normal n = (0, -tan_t, 1), g1 = g2 x e3 (line of nodes)
        const V3 n = mk(0.0f, -a.tan_t, 1.0f);
        float ne = dot(n, e3);
        V3 np_ = mk(fmaf(-ne, e3.x, n.x), fmaf(-ne, e3.y, n.y), fmaf(-ne, e3.z, n.z));
        float nn = dot(np_, np_);
        if (nn > 1e-12f) {
            g2 = (1.0f / sqrtf(nn)) * np_;
        } else {  // the ray stays inside the disk plane and never crosses it: any in-plane axis
            g2 = (1.0f / a.r0) * p0;
        }
        g1 = cross(g2, e3);
        Bn = dot(n, g2);
        u = dot(p0, g1);
        w = dot(p0, g2);
        du = tau * dot(d0, g1);
        dw = tau * dot(d0, g2);
        ij = 1.0f / a.r0;
        float i2 = ij * ij;
        c1 = -(i2 * i2 * ij);
        asm volatile("v_mov_b32 %0, %1" : "=v"(esc2) : "s"(a.r_esc2));
        full = false;
        affine = 0.0f;
        sh.accum = mk(0, 0, 0);
        sh.alpha_total = 0.0f;
        sh.unsure = 0;
        n_pend = 0;
        step_count = 0;
        done = a.max_iter <= 0 ? 3 : 0;
        pix = j_local * a.width + i;
        if (DIFF) {
            ddx = mk(tau * dot(gx, g1), tau * dot(gx, g2), tau * dot(gx, e3));
            ddy = mk(tau * dot(gy, g1), tau * dot(gy, g2), tau * dot(gy, e3));
            dpx = mk(0, 0, 0);
            dpy = mk(0, 0, 0);
        }
    }

    // coefficient c = -1 / r^5 and 1/r^2 from i1 = 1/r
    __device__ __forceinline__ float coef(float i1, float &i2) const {
        i2 = i1 * i1;
        return -(i2 * i2 * i1);
    }
    // (The radii of stages 2 and 3 are both known before either coefficient is needed, and so are stage 4's and the new
    // position's: their v_rsq go back to back -- rsq2 -- five transcendentals per step in three groups instead of five.)
    // J(s) delta with delta = (in-plane u, in-plane w, out-of-plane n)
    __device__ __forceinline__ V3 jac(float su, float sw, V3 dl, float c, float i2) const {
        float proj5 = 5.0f * fmaf(su, dl.x, sw * dl.y) * i2;
        return mk(c * fmaf(-proj5, su, dl.x), c * fmaf(-proj5, sw, dl.y), c * dl.z);
    }
    __device__ __forceinline__ void rk4_diff(V3 &dp, V3 &dd, float h, float hh, float h6, float s2u, float s2w,
                                             float s3u, float s3w, float s4u, float s4w, float c2, float c3,
                                             float c4, float i2_1, float i2_2, float i2_3, float i2_4) const {
        V3 j1 = jac(u, w, dp, c1, i2_1);
        V3 e2_ = fma3(hh, dd, dp), w2 = fma3(hh, j1, dd);
        V3 j2 = jac(s2u, s2w, e2_, c2, i2_2);
        V3 e3_ = fma3(hh, w2, dp), w3 = fma3(hh, j2, dd);
        V3 j3 = jac(s3u, s3w, e3_, c3, i2_3);
        V3 e4_ = fma3(h, w3, dp), w4 = fma3(h, j3, dd);
        V3 j4 = jac(s4u, s4w, e4_, c4, i2_4);
        V3 ndp = fma3(h6, (dd + w4) + 2.0f * (w2 + w3), dp);
        V3 ndd = fma3(h6, (j1 + j4) + 2.0f * (j2 + j3), dd);
        dp = ndp;
        dd = ndd;
    }
    __device__ __forceinline__ V3 to3d(float cu, float cw) const {
        return mk(fmaf(cu, g1.x, cw * g2.x), fmaf(cu, g1.y, cw * g2.y), fmaf(cu, g1.z, cw * g2.z));
    }

    // One iteration of the while-loop at render.py:2854-3006.  Statement order keeps every state variable
    // updated in place after its last use; the state is committed unconditionally (a terminated lane leaves
    // the loop, an escaped ray reads (du, dw) back as new_dir).
    __device__ __forceinline__ bool step(const BhrMarchArgs &a) {
        // adaptive step (render.py:2858-2869) from 1/r with ONE transcendental:  q = 1/r_safe, far_scale = min(sqrt(r_safe), 10)
        // = rsq(max(q, 0.01)), near_damp = 1 / (1 + 2 q^3), so far_scale near_damp = rsq(max(q, 0.01) (1 + 2 q^3)^2).  The
        // reference's clamp to [0.2, 10] never binds: q <= 1 / 1.001 gives far_scale >= 1 and near_damp > 1/3, and the
        // product is <= far_scale <= 10.  (Round 3: v_rsq + v_rcp, 12.7 issue cycles each inside this instruction mix.)
        float q = fminf(ij, 1.0f / (BHR_RS + 1e-3f));
        float nd = fmaf(2.0f * q, q * q, 1.0f);
        float dt_fac = q_rsq(fmaxf(q, 0.01f) * (nd * nd));
        float h = dt_fac * hk;             // in the ray's own clock
        float hh = 0.5f * h;
        float h6 = h * (1.0f / 6.0f);

        // RK4 (render.py:2872-2882) on velocities v_k = k_kp / h and accelerations a_k = k_kd / h
        float a1u = c1 * u, a1w = c1 * w;
        float s2u = fmaf(hh, du, u), s2w = fmaf(hh, dw, w);
        float v2u = fmaf(hh, a1u, du), v2w = fmaf(hh, a1w, dw);
        float i2_2, i2_3, i2_4;
        float s3u = fmaf(hh, v2u, u), s3w = fmaf(hh, v2w, w);
        float i1_2, i1_3, i1_4, i1_n;
        rsq2(fmaf(s2u, s2u, s2w * s2w), fmaf(s3u, s3u, s3w * s3w), i1_2, i1_3);
        float c2 = coef(i1_2, i2_2);
        float a2u = c2 * s2u, a2w = c2 * s2w;
        float v3u = fmaf(hh, a2u, du), v3w = fmaf(hh, a2w, dw);
        float c3 = coef(i1_3, i2_3);
        float a3u = c3 * s3u, a3w = c3 * s3w;
        float s4u = fmaf(h, v3u, u), s4w = fmaf(h, v3w, w);
        float v4u = fmaf(h, a3u, du), v4w = fmaf(h, a3w, dw);
        float nu = fmaf(h6, (du + v4u) + 2.0f * (v2u + v3u), u);
        float nw = fmaf(h6, (dw + v4w) + 2.0f * (v2w + v3w), w);
        float r2n = fmaf(nu, nu, nw * nw);
        rsq2(fmaf(s4u, s4u, s4w * s4w), r2n, i1_4, i1_n);
        float c4 = coef(i1_4, i2_4);
        float sdu = fmaf(c4, s4u, a1u) + 2.0f * (a2u + a3u);
        float sdw = fmaf(c4, s4w, a1w) + 2.0f * (a2w + a3w);

        // the affine parameter is kept in units of h_base: one plain v_add per step, compared against max_affine / h_base
        float aff = affine + dt_fac;
        // termination precedes the plane test (render.py:2916-2926); r < r_s  <=>  r^2 < r_s^2 etc.  One v_med3 and one
        // compare for the two radii (a compare costs two plain instructions' issue time): the ray goes on iff
        // r_s^2 <= r^2 <= r_esc^2, the same strict inequalities as the reference's.  Which of the two ended it is worked
        // out once, behind the loop (escaped()).
        const bool ended = __builtin_amdgcn_fmed3f(r2n, BHR_RS * BHR_RS, esc2) != r2n || aff > a.max_affine_u;
        const bool alive = !ended;
        // The plane function is Bn w: its sign changes where w's does, so the loop carries no plane function and no Bn (two
        // registers and a multiplication per step); the reference's own test, on the products, is made inside the
        // wave-uniform branch below (it also keeps a ray that lies IN the disk plane, Bn = 0, from ever crossing it).
        const bool crossing = w * nw < 0;
        const float f_old = Bn * w, f_new = Bn * nw;     // (dead in the kernels that read no guard flag)
        // Discontinuity guard (read by the hybrid kernel only): a step that crosses the disk plane registers the hit only
        // if it does not also end the ray (render.py:2916-2934) -- with a disk wider than the escape sphere that is a hit /
        // no-hit switch at |new_pos| = r_escape.  A crossing step that ends within the guard of a termination radius marks the lane.
        if (f_old * f_new < 0 && (fabsf(r2n - a.r_esc2) < BHR_R2_GUARD * a.r_esc2 || fabsf(r2n - BHR_RS * BHR_RS) < BHR_R2_GUARD)) sh.unsure = 1;
        // ... and a step that ENDS on the plane: the reference tests f_old f_new < 0, so a new_pos whose plane function
        // rounds to exactly 0 is a crossing that no step ever registers (a black pixel inside the disk: ~1e-6 of the
        // crossings, a dozen pixels of a 4k frame), and one a few ulps either side of 0 moves the hit into the next
        // step (which may be the terminating one).  Only the bit-identical arithmetic reproduces these.
        if (f_new * f_new < BHR_F_GUARD * BHR_F_GUARD * r2n) sh.unsure = 1;
        bool hit_now = false;
        if (SRC == 2) {
            if (alive) volume_segment(a, sh, to3d(u, w), to3d(nu, nw), to3d(du, dw), f_old, f_new, q_rcp(ij), r2n * q_rsq(r2n));
        } else if (__builtin_amdgcn_ballot_w64(crossing) != 0ull) {
            // (a wave-uniform branch around the crossing code: `full` is then a uniform value set under uniform control, it
            // stays in a scalar register and the march loop tests it with a scalar compare -- the per-step
            // v_cmp(n_pend == 2) + v_cmp(n_pend > 0) of round 3 cost four plain instructions' issue time.  The branch is on
            // the ONE compare's mask: combined with `alive` hipcc rebuilds the mask through v_cndmask + v_cmp)
            const float bn = fmaf(-a.tan_t, g2.y, g2.z);           // n . g2 again: Bn is not kept across the loop
            const float fo = bn * w, fn = bn * nw;
            if (alive && fo * fn < 0) {
                float t_frac = fo / (fo - fn + 1e-8f);
                float hu = fmaf(t_frac, nu - u, u), hw = fmaf(t_frac, nw - w, w);
                float hx = fmaf(hu, g1.x, hw * g2.x);
                float hy = fmaf(hu, g1.y, hw * g2.y);
                float hr2 = fmaf(hx, hx, hy * hy);
                float hit_r = hr2 * q_rsq(hr2);
                // the annulus test is the other switch: a crossing within the guard of either edge marks the lane
                if (fabsf(hit_r - a.r_outer) < BHR_EDGE_GUARD * a.r_outer || fabsf(hit_r - a.r_inner) < BHR_EDGE_GUARD * a.r_inner) sh.unsure = 1;
                if (a.r_outer >= hit_r && hit_r >= a.r_inner) {   // render.py:2951
                    V3 dir3 = to3d(du, dw);                  // direction at the START of the step (render.py:2954), x tau
                    Pending<DIFF> h;
                    h.hit_x = hx;
                    h.hit_y = hy;
                    h.to_cam = mk(-dir3.x, -dir3.y, -dir3.z);
                    if (DIFF) h.dxx = h.dxy = h.dyx = h.dyy = 0.0f;   // attached below, once the new differentials exist
                    park_store<DIFF>(n_pend, h);                      // a free slot is guaranteed (march_tile_kernel)
                    n_pend += 1;
                    hit_now = true;
                }
            }
            full = __builtin_amdgcn_ballot_w64(n_pend == 2) != 0ull;
        }
        if (DIFF && alive) {
            // variational RK4 at the same four stage positions (render.py:2888-2911); the hit reads the
            // NEW differentials (committed before the plane test, render.py:2928-2932)
            float i2_1 = ij * ij;
            rk4_diff(dpx, ddx, h, hh, h6, s2u, s2w, s3u, s3w, s4u, s4w, c2, c3, c4, i2_1, i2_2, i2_3, i2_4);
            rk4_diff(dpy, ddy, h, hh, h6, s2u, s2w, s3u, s3w, s4u, s4w, c2, c3, c4, i2_1, i2_2, i2_3, i2_4);
            if (hit_now) {                               // hit parked in THIS step: attach its footprint
                V3 e3 = cross(g1, g2);
                const float fxx = dpx.x * g1.x + dpx.y * g2.x + dpx.z * e3.x, fxy = dpx.x * g1.y + dpx.y * g2.y + dpx.z * e3.y;
                const float fyx = dpy.x * g1.x + dpy.y * g2.x + dpy.z * e3.x, fyy = dpy.x * g1.y + dpy.y * g2.y + dpy.z * e3.y;
                const int slot = n_pend - 1, t = threadIdx.x;
                g_park[slot][5][t] = fxx;
                g_park[slot][6][t] = fxy;
                g_park[slot][7][t] = fyx;
                g_park[slot][8][t] = fyy;
            }
        }
        affine = aff;
        du = fmaf(h6, sdu, du);                          // escaped rays read these back as the escape
        dw = fmaf(h6, sdw, dw);                          // direction = new_dir (render.py:2921)
        u = nu;
        w = nw;
        ij = i1_n;
        float i2 = ij * ij;
        c1 = -(i2 * i2 * ij);
        step_count += 1;
        done = ended ? 2 : (step_count >= a.max_iter ? 3 : 0);      // 2 = captured or escaped: escaped() tells
        return true;     // two parking slots: a step never has to be repeated
    }

    // The loop's own termination test once more, on the state a finished lane is left with (the same expressions on the same
    // values): the tile kernels call it behind the march loop instead of reading `done` back -- a value written inside a
    // loop that lanes leave at different trips and read behind it costs three scalar mask instructions per trip and per
    // bit to keep (the exit mask alone is the loop's own).
    __device__ __forceinline__ void settle(const BhrMarchArgs &a) {
        const float r2 = fmaf(u, u, w * w);
        done = (__builtin_amdgcn_fmed3f(r2, BHR_RS * BHR_RS, esc2) != r2 || affine > a.max_affine_u) ? 2 : 3;
    }
    // which of the two radii (or the affine limit) ended the ray: captured = inside r_s, as the loop's own test has it
    __device__ __forceinline__ bool escaped() const { return done == 2 && !(fmaf(u, u, w * w) < BHR_RS * BHR_RS); }

    // shade the oldest parked crossing (lanes that have one), the second slot moves up
    __device__ __forceinline__ void flush_one(const BhrMarchArgs &a) {
        if (n_pend > 0) {
            const Pending<DIFF> h = park_pop<DIFF>(n_pend);
            shade_hit<DIFF, SRC>(a, sh, h.hit_x, h.hit_y, h.to_cam, h.dxx, h.dxy, h.dyx, h.dyy);
        }
    }
    __device__ __forceinline__ void finish(const BhrMarchArgs &a) { write_pixel(a, pix % a.width, pix / a.width, escaped(), to3d(du, dw), sh); }
    __device__ __forceinline__ void finish_at(const BhrMarchArgs &a, int i, int j) { write_pixel(a, i, j, escaped(), to3d(du, dw), sh); }
    __device__ __forceinline__ void values(const BhrMarchArgs &a, float bk[3], float dk[3]) const { pixel_values(a, escaped(), to3d(du, dw), sh, bk, dk); }
};

}  // namespace
