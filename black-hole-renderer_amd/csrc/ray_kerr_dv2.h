// ray_kerr_dv2.h -- the Kerr Ray over the analytic Disk V2 sources (march_kerr_dv2.o; see march_device.h): the spinning hole's
// march with the Disk V2 model in place of the disk texture (bhr_set_kerr_disk_source), as a surface on the plane z = 0 and as
// the finite-thickness emission-absorption volume around it.
//
// The march is the Kerr Ray's, untouched: RK4 on (x, p), step rule, capture at r_plus, escape.  What differs is what is shaded.
// Cylinder coordinates of a Kerr-Schild point x, with r its Kerr-Schild radius (ray_kerr.h: kerr_geom):
//   varpi = sqrt(max(r^2 - z^2, 0))      the Boyer-Lindquist r sin(theta); on the plane sqrt(x^2 + y^2 - a^2), the hit radius
//   zeta  = z,   phi = atan2(y, x)
//   phi_adv = phi + t_offset dv2::omega_field(varpi)        the model's own pattern speed; Kerr's Omega enters through g alone
// The model's parameters, normalisation constants and colour mapping are the Schwarzschild sources' (march_device.h:
// disk_v2_rgba, disk_v2_color, volume_segment), evaluated in binary64 from the f32 point; compositing in f32.
//
// Surface (Ray<false, 0> model redshift, Ray<false, KERR_EXACT> exact): the step is the Kerr Ray's and parks what it parked;
// flush_one shades a parked crossing with disk_v2_rgba's mapping at (varpi, phi_adv), then kerr_shade_hit's opacity, g-factor
// and compositing.  The binary64 code runs in the shade passes, outside the step, where the texture sample ran.
//
// Volume (Ray<false, KERR_DV2_VOLUME>, model redshift): no surface crossing is shaded -- what the base step parks is dropped --
// and every step that does not end the ray is one chord x -> x_new, cut into vol_substeps pieces sampled at their midpoints:
//   rho = max(rho_field(varpi, zeta) F, 0),  T = clamp(t_field(varpi, zeta) F / t_peak, 0, 1),  F = structure_total(varpi, phi_adv)
//   mu = |e_z| / |e| (e the chord),  alpha_eff = Ca rho (1 + kg (1 - mu)),  op = 1 - exp(-alpha_eff ds),  ds = |e| / vol_substeps
//   colour kerr_g_factor<0>(disk_v2_color(T), s_x, s_y, varpi, to_cam),  to_cam = -dx/dl at the START of the step
// A ray stops collecting at BHR_VOLUME_OPAQUE, tested once per chord as volume_segment tests it.
//
// The cull of chords (DESIGN.md "Kerr Disk V2" has the argument).  The volume is r_in <= varpi <= r_out, |zeta| <= H(varpi) <=
// H_max, and r^2 = varpi^2 + zeta^2 exactly, so its points have r_in <= r <= sqrt(r_out^2 + H_max^2) =: R and |z| <= H_max.
//   * z is linear along the chord: both ends beyond H_max on one side of the plane -> no sample inside.
//   * the sets r <= c are ellipsoids, convex: r along a chord is largest at an end -> max(r0, r1) < r_in: no sample inside.
//   * r^2 = |x|^2 - a^2 sin^2(theta), so r <= |x| and |x|^2 <= r^2 + a^2.  A point of the chord is no farther than half its
//     length from the nearer end, so |s| >= min(|x0|, |x1|) - l / 2 >= min(r0, r1) - l / 2; a sample inside has |s|^2 <= R^2 + a^2.
//     min(r0, r1) - 0.51 l > sqrt(R^2 + a^2) =: vol_r_max -> no sample inside (0.51: the f32 rounding of r0, r1 and l).
// The test is per lane and cheap; a wave-uniform ballot around the segment code makes a step far from the slab cost a compare.
#pragma once
#define BHR_RAY_KERR_DV2 1   // ray_kerr.h: the schedules' Ray is the one below, derived from the Kerr one
#include "ray_kerr.h"

namespace {

constexpr int KERR_DV2_VOLUME = 2;   // Ray<false, KERR_DV2_VOLUME>: the volume (model redshift)

// disk_v2_rgba (march_device.h) at the Kerr cylinder coordinates of a crossing of the plane, binary64 from the f32 hit point
__device__ __forceinline__ float4 kerr_dv2_rgba(const BhrMarchArgs &a, float hit_x, float hit_y) {
    const bhr_disk_v2_params &p = *a.dv2;
    const double ka = (double)kerr(a).kerr_a;
    const double w = sqrt(fmax((double)hit_x * hit_x + (double)hit_y * hit_y - ka * ka, 0.0));
    const double phi = atan2((double)hit_y, (double)hit_x) + (double)a.t_offset * dv2::omega_field(w, p);
    const double F = dv2::structure_total(w, phi, p, a.dv2_norm_shear, a.dv2_norm_hotspot);
    const double t = fmin(fmax(dv2::t_mid(w, p) * F / a.dv2_t_peak, 0.0), 1.0);
    const double rho = fmin(fmax(dv2::rho_mid(w, p) * F, 0.0), 1.0);
    const V3 c = disk_v2_color((float)t);
    return make_float4(c.x, c.y, c.z, (float)rho);
}

// kerr_shade_hit (ray_kerr.h) with the model in the texture's place
template <int RS>
__device__ __forceinline__ void kerr_dv2_shade_hit(const BhrMarchArgs &a, Shade &sh, float hit_x, float hit_y, V3 to_cam) {
    const float hit_r = sqrtf(hit_x * hit_x + hit_y * hit_y - kerr(a).kerr_a * kerr(a).kerr_a);
    if (!(a.r_outer >= hit_r && hit_r >= a.r_inner)) return;
    const float4 rgba = kerr_dv2_rgba(a, hit_x, hit_y);
    const float base_alpha = fminf(rgba.w, 0.999f);
    const float disk_alpha = 1.0f - powf(1.0f - base_alpha, BHR_DISK_ALPHA_GAIN);
    const V3 col = kerr_g_factor<RS>(a, a, mk(rgba.x, rgba.y, rgba.z), hit_x, hit_y, hit_r, to_cam);
    const float front = 1.0f - sh.alpha_total;
    const float wgt = disk_alpha * front;
    sh.accum = mk(sh.accum.x + col.x * wgt, sh.accum.y + col.y * wgt, sh.accum.z + col.z * wgt);
    sh.alpha_total = 1.0f - front * (1.0f - disk_alpha);
}

// One chord x0 -> x1 of a ray through the volume (the header has the model); v0 = dx/dl at x0.  The caller has culled.
__device__ __forceinline__ void kerr_dv2_segment(const BhrMarchArgs &a, Shade &sh, V3 x0, V3 x1, V3 v0) {
    const bhr_disk_v2_params &P = *a.dv2;
    const double ka = (double)kerr(a).kerr_a, a2 = ka * ka;
    const double ex = (double)x1.x - (double)x0.x, ey = (double)x1.y - (double)x0.y, ez = (double)x1.z - (double)x0.z;
    const double len = sqrt(ex * ex + ey * ey + ez * ez);
    if (!(len > 0.0)) return;
    const double mu = fabs(ez) / len;
    const double ds = len / (double)a.vol_substeps;
    const V3 to_cam = mk(-v0.x, -v0.y, -v0.z);
    for (int k = 0; k < a.vol_substeps; ++k) {
        const double f = ((double)k + 0.5) / (double)a.vol_substeps;
        const double sx = (double)x0.x + f * ex, sy = (double)x0.y + f * ey, sz = (double)x0.z + f * ez;
        // the Kerr-Schild radius of the sample: r^2 = (w + S) / 2, and varpi^2 = r^2 - z^2
        const double w = sx * sx + sy * sy + sz * sz - a2;
        const double r2 = 0.5 * (w + sqrt(w * w + 4.0 * a2 * (sz * sz)));
        const double vp = sqrt(fmax(r2 - sz * sz, 0.0));
        if (!dv2::volume_mask(vp, sz, P)) continue;
        const double phi = atan2(sy, sx) + (double)a.t_offset * dv2::omega_field(vp, P);
        const double F = dv2::structure_total(vp, phi, P, a.dv2_norm_shear, a.dv2_norm_hotspot);
        const double rho = fmax(dv2::rho_field(vp, sz, P) * F, 0.0);
        const double t = fmin(fmax(dv2::t_field(vp, sz, P) * F / a.dv2_t_peak, 0.0), 1.0);
        const double alpha_eff = a.vol_absorption * rho * (1.0 + a.vol_grazing_gain * (1.0 - mu));
        const float op = (float)(1.0 - exp(-alpha_eff * ds));
        if (!(op > 0.0f)) continue;
        const V3 col = kerr_g_factor<0>(a, a, disk_v2_color((float)t), (float)sx, (float)sy, (float)vp, to_cam);
        const float front = 1.0f - sh.alpha_total;
        const float wgt = op * front;
        sh.accum = mk(sh.accum.x + col.x * wgt, sh.accum.y + col.y * wgt, sh.accum.z + col.z * wgt);
        sh.alpha_total = 1.0f - front * (1.0f - op);
    }
}

template <bool DIFF, int SRC = 0>
struct Ray : KerrRay<false, SRC == KERR_EXACT ? KERR_EXACT : 0> {
    static_assert(!DIFF, "the analytic source has no mip chain: no ray differentials");
    static_assert(SRC == 0 || SRC == KERR_EXACT || SRC == KERR_DV2_VOLUME, "the Kerr Disk V2 Ray: surface with the model or the exact redshift, or the volume");
    typedef KerrRay<false, SRC == KERR_EXACT ? KERR_EXACT : 0> Base;
    static constexpr bool VOL = SRC == KERR_DV2_VOLUME;

    __device__ __forceinline__ bool step(const BhrMarchArgs &a) {
        if (!VOL) return Base::step(a);
        // the volume: the base step between the chord's two ends.  (x, p) at the start are kept for the chord and for dx/dl
        // there, which is made again only where a lane integrates (one right-hand side, the values of the step's first stage)
        const V3 x0 = this->x, p0 = this->p;
        const float r0 = this->r;
        Base::step(a);
        this->n_pend = 0;                                  // no surface: what the step parked is dropped (n_pend never reaches 2)
        const V3 x1 = this->x;
        const float r1 = this->r;
        const float cx = x1.x - x0.x, cy = x1.y - x0.y, cz = x1.z - x0.z;
        const float reach = 0.51f * sqrtf(cx * cx + cy * cy + cz * cz);
        const float h_max = (float)a.vol_h_max;
        const bool near_plane = x0.z * x1.z < 0.0f || fminf(fabsf(x0.z), fabsf(x1.z)) <= h_max;
        const bool cand = this->done != 2 && this->sh.alpha_total < BHR_VOLUME_OPAQUE && near_plane &&
                          (double)(fmaxf(r0, r1) * (1.0f + 1e-6f)) >= a.dv2->r_in && (double)(fminf(r0, r1) - reach) <= a.vol_r_max;
        if (__builtin_amdgcn_ballot_w64(cand) != 0ull) {
            if (cand) {
                V3 v0, d0;
                float rr;
                kerr_rhs(kerr(a).kerr_a, kerr(a).kerr_a * kerr(a).kerr_a, x0, p0, v0, d0, rr);
                kerr_dv2_segment(a, this->sh, x0, x1, v0);
            }
        }
        return true;
    }

    // shade the oldest parked crossing (the Kerr Ray's flush_one with the model in the texture's place); the volume parks none
    __device__ __forceinline__ void flush_one(const BhrMarchArgs &a) {
        if (VOL) return;
        if (this->n_pend > 0) {
            const Pending<false> h = park_pop<false>(this->n_pend);
            kerr_dv2_shade_hit<SRC == KERR_EXACT ? KERR_EXACT : 0>(a, this->sh, h.hit_x, h.hit_y, h.to_cam);
        }
    }
};

}  // namespace
