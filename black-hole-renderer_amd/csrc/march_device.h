// march_device.h -- the fused Schwarzschild ray-march kernel for gfx950 (MI355X): what its two arithmetics share.
//
// One ray per lane.  Everything the reference does per pixel in
// _ray_march_kernel (render.py:2787-3018) happens inside this one kernel:
// pixel -> ray setup, adaptive-step RK4 on d2x/dl2 = -1.5 L^2 x / r^5, the
// optional variational RK4 pair for ray differentials, capture / escape tests,
// tilted-plane crossing, disk texture or mip-LOD lookup, g-factor shading
// (_apply_g_factor, render.py:2439-2516), front-to-back compositing and the
// skybox lookup of the escape direction.  There is no dense contraction, so no
// MFMA: the kernel is FP32 VALU + transcendental bound (DESIGN.md "Rooflines").
//
// Two schedules share the per-ray code:
//  * tile (default): a wave owns one 8x8 pixel tile; lanes leave the loop as their rays terminate (lane
//                efficiency ~0.95 for the default view).  Tiles are launched nearest-to-the-hole first.
//  * persistent (BHR_PERSISTENT): waves pull 8x8 tiles from a global queue; when the
//                number of live lanes drops below a threshold the dead lanes write
//                their pixel and are refilled from the next tile (wave-level
//                __ballot / popcount compaction of the *work*, not of registers).
//                Slower than the tile schedule for the BASELINE views.
// Disk sources (template parameter SRC, own kernel instantiations): 0 texture / mip stack, 1 Disk V2 mid-plane
// fields at each plane crossing, 2 Disk V2 finite-thickness emission-absorption integral (volume_segment).
// Disk crossings are parked in per-lane LDS slots and shaded wave-wide (Pending, flush_one).
//
// The fast build's arithmetic differs from a strict f32 evaluation of the reference only in rounding:
// v_rsq/v_rcp/v_sqrt instead of IEEE sqrt + divide inside the RK4 stages, FMA contraction, and the
// re-use of |new_pos| as the next step's |pos| (same value in the reference).
//
// The march's device source is a header per Ray and per schedule and a translation unit per object (csrc/Makefile):
//   march_device.h      this file: vectors, exact-rounding sequences, samplers, shading, parking slots, pixel stores
//   ray_strict.h        Ray<DIFF, SRC>, strict: every operation of the RK4 loop in the reference's order with IEEE sqrt and
//                       divide, so that positions, step counts and hit points are bit-identical to a strict f32 evaluation
//                       of render.py:2854-3006 (selected with bhr_config.math_mode = 1)
//   ray_fast.h          Ray<DIFF, SRC>, fast: v_rsq/v_rcp/v_sqrt, FMA contraction, in-plane state, the ray's own clock
//   march_tile.h        the tile schedule: march_tile_body, its plain, supersampled and list kernels
//   march_persistent.h  the persistent schedule
//   march.hip            -> march.o             ray_fast.h, both schedules; fast-math
//   march_strict.hip     -> march_strict.o      ray_strict.h, both schedules, detect kernel, self-test; -ffp-contract=off
//   march_strict_ilp.hip -> march_strict_ilp.o  ray_strict.h, tile schedule: the strict texture kernels and the fix kernel of
//                                               a hybrid march; the strict flags and the ILP-first machine scheduler
//   march_raymap.hip     -> march_raymap.o      ray_strict.h: the ray map's build and shade kernels; the ILP object's flags
// and per march variant (bhr_internal.h: bhr_march_variant, with a row of what the host knows of it) a ray_<v>.h with a
// Ray<false, 0> of its own and a march_<v>.hip -> march_<v>.o with the tile schedule's plain and supersampled kernel:
//   kerr       a spinning hole in Kerr-Schild coordinates, RK4 on (x, p), its own sampler and g-factor, model or exact
//              (bhr_set_spin, bhr_set_redshift), and each once more over its Ray<true, RS>: two ray tangents beside (x, p)
//              and the mip level of every crossing (bhr_set_kerr_anti_alias); the Schwarzschild Rays know nothing of it;
//              -ffp-contract=on, no fast-math
//              (and march_kerr_raymap.hip -> march_kerr_raymap.o over the same Ray: the Kerr ray map's build, shade and
//              overflow kernels, with the Kerr object's flags; its table is bhr_march_kernel_kerr_raymap)
//              (and march_kerr_dv2.hip -> march_kerr_dv2.o over ray_kerr_dv2.h's Ray, derived from the Kerr one: the Kerr march over
//              the analytic Disk V2 sources, surface and volume (bhr_set_kerr_disk_source); the Kerr object's flags; its table is
//              bhr_march_kernel_kerr_dv2, picked by march_kernel under the Kerr variants while a Kerr source is set)
//   kerr_observer  the Kerr Ray launched along the aberrated pinhole, equirectangular or fisheye direction of a camera that may
//              move, its Doppler factor in the disk's g and on the sky (bhr_render_kerr_view); the Kerr object's flags;
//              camera_device.h holds what it shares with the next two (the projections' directions, the sky's scaling)
//   observer   the strict Ray launched along the aberrated pixel direction of a moving camera, its Doppler factor in the
//              disk's g and on the sky (bhr_render_observer); the strict flags, as the next two
//   projected  the observer Ray launched along an equirectangular or fisheye pixel direction (bhr_render_projected)
//   delay      the strict Ray with the light's coordinate time beside it, every disk crossing shaded at its emission time
//              (bhr_render_delayed)
// A translation unit includes the one Ray header it marches with (which includes this file), then the schedules it uses,
// defines the kernels that are its own and ends with their table, by which the one host launcher (march_launch.hip) finds
// them: bhr_march_kernel_fast / _strict / _strict_ilp / _raymap, and bhr_march_kernel_<v> through the variant's row.
#pragma once
#include "bhr_internal.h"
#include "disk_v2_device.h"

// The two places where shared code differs by arithmetic (BHR_BILERP, the accumulation in shade_hit) are keyed on
// BHR_RAY_STRICT, which the Ray header sets before it includes this file; never on a command line.
#ifndef BHR_RAY_STRICT
#error "include ray_strict.h, ray_fast.h or ray_kerr.h, not march_device.h"
#endif
#ifndef BHR_WAVE_STAMPS_BUILD
#define BHR_WAVE_STAMPS_BUILD 0
#endif

namespace {

struct V3 {
    float x, y, z;
};
__device__ __forceinline__ V3 mk(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return mk(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// s*a + b, component-wise
__device__ __forceinline__ V3 fma3(float s, V3 a, V3 b) {
    return mk(fmaf(s, a.x, b.x), fmaf(s, a.y, b.y), fmaf(s, a.z, b.z));
}
__device__ __forceinline__ V3 ld3(const float *p) { return mk(p[0], p[1], p[2]); }

__device__ __forceinline__ float q_rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float q_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float q_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// Correctly rounded x / 6 in TWO operations: 1/6 = c_hi + c_lo up to 2^-50 (c_hi = RN(1/6), c_lo = RN(1/6 - c_hi)),
//   q = RN(x c_hi + RN(x c_lo)).
// The argument of the final rounding is within 2^-48 (relative) of x / 6, and x / 6 is never closer than 1/6 ulp to
// a rounding boundary (6 q = integer significand => the fractional position is a multiple of 1/3 of half an ulp),
// so the rounding is the correct one for every normal x.  tests/test_div6.py checks it against IEEE division on
// every f32 significand, bhr_selftest() on the device.  (Round 1 used the generic 3-operation Markstein sequence.)
__device__ __forceinline__ float div6(float x) {
    const float c_hi = 0x1.555556p-3f, c_lo = -0x1.555556p-28f;
    return fmaf(x, c_hi, x * c_lo);
}

// IEEE-754 correctly rounded sqrt, reciprocal and divide for NORMAL-range operands (no overflow or
// underflow of the result), as Newton/Markstein steps on the hardware approximations:
//   sqrt(x): y = v_rsq(x); s = x y; s' = s + (x - s s)(y/2)            5 instructions
//   1/b    : y = v_rcp(b); y' = y + (1 - b y) y                        3 instructions
//   a/b    : q = a y'; q' = q + (a - b q) y'                           6 instructions
// hipcc's own IEEE sequences take 14 / 11 / 11 (they also handle denormals and overflow, which the
// bounded quantities of the march -- r^2 in [0.5, 1e6], |L2|/r^5, 1/r -- never produce).  The
// residuals are exact thanks to FMA; that the final rounding is the correct one was established
// exhaustively on gfx950 (tools/exact_search.hip: every f32 in [2^-80, 2^80) for sqrt and 1/b, 1.7e10
// random + adversarial pairs for a/b, zero mismatches against sqrtf and operator/), and
// bhr_selftest() repeats the check on the device it runs on.  Saves 64 instructions per RK4 step.
__device__ __forceinline__ float sqrt_rn(float x) {
    float y = __builtin_amdgcn_rsqf(x);
    float s = x * y;
    float r = fmaf(-s, s, x);
    return fmaf(r, 0.5f * y, s);
}
__device__ __forceinline__ float rcp_rn(float b) {
    float y = __builtin_amdgcn_rcpf(b);
    return fmaf(fmaf(-b, y, 1.0f), y, y);
}
__device__ __forceinline__ float div_rn(float a, float b) {
    float y = rcp_rn(b);
    float q = a * y;
    return fmaf(fmaf(-b, q, a), y, q);
}
// The same sequences from a seed the caller already holds: the march issues the hardware approximations of independent
// operands back to back (a transcendental costs 8 issue cycles behind another one and ~12.7 behind a plain instruction --
// the stream changes pipes), then refines each.  Same operations on the same values as sqrt_rn / rcp_rn / div_rn.
__device__ __forceinline__ float sqrt_rn_s(float x, float y) {
    float s = x * y;
    float r = fmaf(-s, s, x);
    return fmaf(r, 0.5f * y, s);
}
__device__ __forceinline__ float rcp_rn_s(float b, float y) { return fmaf(fmaf(-b, y, 1.0f), y, y); }
__device__ __forceinline__ float div_rn_s(float a, float b, float y0) {
    float y = rcp_rn_s(b, y0);
    float q = a * y;
    return fmaf(fmaf(-b, q, a), y, q);
}
// (s_nop: a transcendental's result needs one wait state before a VALU reads it; hipcc adds it behind its own, not behind an asm)
__device__ __forceinline__ void rsq2(float x, float y, float &a, float &b) {
    asm("v_rsq_f32 %0, %2\n\tv_rsq_f32 %1, %3\n\ts_nop 0" : "=&v"(a), "=&v"(b) : "v"(x), "v"(y));
}
__device__ __forceinline__ void rcp2(float x, float y, float &a, float &b) {
    asm("v_rcp_f32 %0, %2\n\tv_rcp_f32 %1, %3\n\ts_nop 0" : "=&v"(a), "=&v"(b) : "v"(x), "v"(y));
}
__device__ __forceinline__ void rsq_rcp_rcp(float x, float y, float &rs, float &rx, float &ry) {   // rsq(x), rcp(x), rcp(y)
    asm("v_rsq_f32 %0, %3\n\tv_rcp_f32 %1, %3\n\tv_rcp_f32 %2, %4\n\ts_nop 0" : "=&v"(rs), "=&v"(rx), "=&v"(ry) : "v"(x), "v"(y));
}
// x + 0.5 y and x + 2 y: the products are exact, so one FMA rounds exactly like mul-then-add
__device__ __forceinline__ V3 add_half(V3 x, V3 y) { return mk(fmaf(0.5f, y.x, x.x), fmaf(0.5f, y.y, x.y), fmaf(0.5f, y.z, x.z)); }

// bilinear blend in the reference's evaluation order: c00 (1-fu)(1-fv) + c10 fu (1-fv) + c01 (1-fu) fv + c11 fu fv
#if BHR_RAY_STRICT
#define BHR_BILERP(c00, c10, c01, c11) \
    ((c00) * (1 - fu) * (1 - fv) + (c10) * fu * (1 - fv) + (c01) * (1 - fu) * fv + (c11) * fu * fv)
#else
#define BHR_BILERP(c00, c10, c01, c11) ((c00) * w00 + (c10) * w10 + (c01) * w01 + (c11) * w11)
#endif

// taichi Vector.normalized(): (1/|v|) * v   -- used outside the hot loop, IEEE ops.
__device__ __forceinline__ V3 normalized(V3 v) {
    float inv = 1.0f / sqrtf(dot(v, v));
    return inv * v;
}

__device__ __forceinline__ int pymod(int a, int m) {
    int r = a % m;
    return r < 0 ? r + m : r;
}

// ---- _color_temp_to_tint (render.py:2407-2437) at DISK_COLOR_TEMPERATURE ----
// t = 60 <= 66: r = 1, g = clamp(0.390082 ln 60 - 0.631841), b = clamp(0.543207 ln 50 - 1.19625)
__device__ __forceinline__ V3 disk_tint() {
    const float t = BHR_DISK_COLOR_TEMPERATURE / 100.0f;
    float g = fminf(fmaxf(0.390082f * logf(fmaxf(t, 0.0001f)) - 0.631841f, 0.0f), 1.0f);
    float b = fminf(fmaxf(0.543207f * logf(fmaxf(t - 10.0f, 0.0001f)) - 1.19625f, 0.0f), 1.0f);
    return mk(1.0f, g, b);
}

// ---- _sample_skybox (render.py:2541-2566) ---------------------------------
__device__ __forceinline__ V3 sample_skybox(const BhrScene &sc, V3 d) {
    const int tex_w = sc.sky_w, tex_h = sc.sky_h;
    float theta = acosf(fminf(fmaxf(d.z, -1.0f), 1.0f));
    float phi = atan2f(d.y, d.x);
    if (phi < 0) phi += BHR_TWO_PI_F;
    float u = phi / BHR_TWO_PI_F * (float)tex_w;
    float v = theta / BHR_PI_F * (float)tex_h;
    int u0 = (int)floorf(u);
    int v0 = (int)floorf(v);
    float fu = u - (float)u0;
    float fv = v - (float)v0;
    int u0_w = pymod(u0, tex_w);
    int u1_w = pymod(u0 + 1, tex_w);
    int v0_h = min(max(v0, 0), tex_h - 1);
    int v1_h = min(max(v0 + 1, 0), tex_h - 1);
    const float *c00 = sc.skybox + ((size_t)v0_h * tex_w + u0_w) * 3;
    const float *c10 = sc.skybox + ((size_t)v0_h * tex_w + u1_w) * 3;
    const float *c01 = sc.skybox + ((size_t)v1_h * tex_w + u0_w) * 3;
    const float *c11 = sc.skybox + ((size_t)v1_h * tex_w + u1_w) * 3;
    float w00 = (1 - fu) * (1 - fv), w10 = fu * (1 - fv), w01 = (1 - fu) * fv, w11 = fu * fv;
    (void)w00; (void)w10; (void)w01; (void)w11;
    return mk(BHR_BILERP(c00[0], c10[0], c01[0], c11[0]), BHR_BILERP(c00[1], c10[1], c01[1], c11[1]),
              BHR_BILERP(c00[2], c10[2], c01[2], c11[2]));
}

// ---- _sample_disk / _sample_disk_mip (render.py:2568-2637) -------------------
// lod_i = 0 reproduces _sample_disk exactly (level 0 of the mip stack is the
// texture itself and n / 2^0 = n).
// `staged` (SRC == 3 kernels): the packed levels staged_from .. last of the mip stack, copied into LDS at block start
__device__ __forceinline__ float4 sample_disk_level(const BhrScene &sc, float hit_x, float hit_y, float r_inner,
                                                    float r_outer, float t_offset, int lod_i,
                                                    const float4 *staged = nullptr, int staged_from = 1 << 30) {
    float r = sqrtf(hit_x * hit_x + hit_y * hit_y);
    float phi = atan2f(hit_y, hit_x);
    float r_safe = fmaxf(r, 1e-3f);
    float omega = sqrtf(0.5f / (r_safe * r_safe * r_safe + 1e-6f));
    phi = phi + t_offset * omega;
    while (phi < 0) phi += BHR_TWO_PI_F;
    while (phi >= BHR_TWO_PI_F) phi -= BHR_TWO_PI_F;

    float scale = (float)(1 << lod_i);  // ti.pow(2.0, lod_i), exact
    float tex_w_lod = (float)sc.n_phi / scale;
    float tex_h_lod = (float)sc.n_r / scale;
    float u = phi / BHR_TWO_PI_F * tex_w_lod;
    float v = (r - r_inner) / (r_outer - r_inner) * tex_h_lod;
    int u0 = (int)floorf(u);
    int v0 = (int)floorf(v);
    float fu = u - (float)u0;
    float fv = v - (float)v0;
    int wl = (int)tex_w_lod;
    int u0_w = pymod(u0, wl);
    int u1_w = pymod(u0 + 1, wl);
    int vmax = (int)(tex_h_lod - 1.0f);
    int v0_h = min(max(v0, 0), vmax);
    int v1_h = min(max(v0 + 1, 0), vmax);
    const float4 *t = lod_i >= staged_from ? staged + (sc.mip_off[lod_i] - sc.mip_off[staged_from]) : sc.mips + sc.mip_off[lod_i];
    const int stride = sc.mip_w[lod_i];
    float4 c00 = t[(size_t)v0_h * stride + u0_w];
    float4 c10 = t[(size_t)v0_h * stride + u1_w];
    float4 c01 = t[(size_t)v1_h * stride + u0_w];
    float4 c11 = t[(size_t)v1_h * stride + u1_w];
    float w00 = (1 - fu) * (1 - fv), w10 = fu * (1 - fv), w01 = (1 - fu) * fv, w11 = fu * fv;
    (void)w00; (void)w10; (void)w01; (void)w11;
    return make_float4(BHR_BILERP(c00.x, c10.x, c01.x, c11.x), BHR_BILERP(c00.y, c10.y, c01.y, c11.y),
                       BHR_BILERP(c00.z, c10.z, c01.z, c11.z), BHR_BILERP(c00.w, c10.w, c01.w, c11.w));
}

// ---- _apply_g_factor (render.py:2439-2516) ----------------------------------
// f: the block the frame's camera position (the observer's radius) is read from -- `a` itself in every march; a shutter frame
// from the ray map shades one set of records under several cameras and hands over each sample's (march_raymap.hip).  ONLY f.cp
// may be read through f: that caller sets nothing else in it (see shade_hit).
// obs_d: nu_observed / nu_static of a moving observer for this ray (ray_observer.h), a factor of g ahead of the cap; the
// literal 1 of every other caller folds away.
__device__ __forceinline__ V3 apply_g_factor(const BhrMarchArgs &a, const BhrMarchArgs &f, V3 base_color, V3 hit_pos, float hit_r,
                                             V3 ray_dir_to_cam, float obs_d = 1.0f) {
    const float rs_f = BHR_RS;
    V3 cam_pos = ld3(f.cp);
    // |cam| is the same for every hit, so the compiler hoists it out of the march loop and keeps it in a VGPR for the
    // whole march (the strict AA kernel spilled it at 128 VGPRs).  Shading runs a handful of times per ray: recompute.
    asm volatile("" : "+v"(cam_pos.x));
    float r_obs = sqrtf(dot(cam_pos, cam_pos));
    float r_em = sqrtf(dot(hit_pos, hit_pos));
    float r_safe = fmaxf(r_em, rs_f + 1e-3f);

    float omega = sqrtf(0.5f / (r_safe * r_safe * r_safe + 1e-6f));
    float lorentz = sqrtf(fmaxf(1.0f - rs_f / r_safe, 1e-6f));
    float beta = fminf(r_safe * omega / fmaxf(lorentz, 1e-6f), 0.99f);
    float gamma = 1.0f / sqrtf(fmaxf(1.0f - beta * beta, 1e-6f));

    V3 disk_normal = mk(0.0f, -a.sin_t, a.cos_t);
    V3 r_hat = normalized(hit_pos);
    V3 v_hat = cross(r_hat, disk_normal);
    float v_norm = sqrtf(dot(v_hat, v_hat));
    if (v_norm > 1e-6f) {
        v_hat = mk(v_hat.x / v_norm, v_hat.y / v_norm, v_hat.z / v_norm);
    } else {
        v_hat = mk(0.0f, 1.0f, 0.0f);
    }
    V3 ray_hat = normalized(ray_dir_to_cam);
    float cos_theta = dot(v_hat, ray_hat);
    float denom = fmaxf(1.0f - beta * cos_theta, 1e-3f);
    float g_doppler = 1.0f / (gamma * denom);

    float grav_num = sqrtf(fmaxf(1.0f - rs_f / fmaxf(r_obs, rs_f + 1e-3f), 1e-6f));
    float grav_den = sqrtf(fmaxf(1.0f - rs_f / fmaxf(r_em, rs_f + 1e-3f), 1e-6f));
    float g_grav = grav_num / grav_den;

    float g = fminf(g_doppler * g_grav * obs_d, BHR_G_FACTOR_CAP);
    float intensity = fmaxf(powf(g, BHR_G_LUMINOSITY_POWER), 0.0f);
    float brightness = BHR_G_BRIGHTNESS_GAIN * intensity / (1.0f + intensity / BHR_G_FACTOR_CAP);

    float radial_span = fmaxf(a.r_outer - a.r_inner, 1e-3f);
    float radial_t = (fmaxf(hit_r, a.r_inner) - a.r_inner) / radial_span;
    radial_t = fminf(fmaxf(radial_t, 0.0f), 1.0f);
    float radial_profile = powf(1.0f - radial_t, BHR_DISK_RADIAL_BRIGHTNESS_POWER);
    float radial_boost = BHR_DISK_RADIAL_BRIGHTNESS_MIN +
                         (BHR_DISK_RADIAL_BRIGHTNESS_MAX - BHR_DISK_RADIAL_BRIGHTNESS_MIN) * radial_profile;
    brightness *= radial_boost;

    // Wien colour shift, normalised to the green channel
    float g_safe = fmaxf(g, 0.1f);
    float wien_arg = 1.0f - 1.0f / g_safe;
    float r_scale = expf(2.21f * wien_arg);
    float g_scale = expf(2.72f * wien_arg);
    float b_scale = expf(3.13f * wien_arg);
    r_scale = fminf(r_scale / g_scale, 3.0f);
    b_scale = fminf(b_scale / g_scale, 3.0f);

    V3 tint = disk_tint();
    V3 out = mk(base_color.x * r_scale * tint.x * brightness, base_color.y * 1.0f * tint.y * brightness,
                base_color.z * b_scale * tint.z * brightness);
    out.x = fminf(fmaxf(out.x, 0.0f), 10.0f);
    out.y = fminf(fmaxf(out.y, 0.0f), 10.0f);
    out.z = fminf(fmaxf(out.z, 0.0f), 10.0f);
    return out;
}
__device__ __forceinline__ V3 apply_g_factor(const BhrMarchArgs &a, V3 base_color, V3 hit_pos, float hit_r, V3 ray_dir_to_cam) {
    return apply_g_factor(a, a, base_color, hit_pos, hit_r, ray_dir_to_cam);
}

// Analytic disk source (bhr_set_disk_source, BHR_DISK_V2): emission colour and opacity straight from
// the Disk V2 model in binary64 instead of a texture lookup -- temperature T_mid(r) F(r, phi) and
// density rho_mid(r) F(r, phi) with F = F_mode F_shear F_hotspot (disk_v2/physical_fields.py,
// structure_modulations.py), pattern advected with the model's own Omega(r).  The mapping to RGBA is
// the compose kernel's (render.py:3192-3194, 3243-3257): t = clamp(T / T_peak), T_K = T_min + t (T_max -
// T_min), rgb = blackbody(T_K) sqrt(t) with blue <= red, alpha = clamp(rho).  The reference never wired
// disk_v2 into its renderer (docs/design_ad_v2.md Phase 4), so this mapping is this build's choice.
__device__ __forceinline__ V3 disk_v2_color(float tf) {
    const float t_factor = (BHR_DISK_COLOR_TEMPERATURE - 4500.0f) / (6500.0f - 2700.0f);
    const float T_min = 2000.0f + t_factor * 1000.0f, T_max = 9000.0f + t_factor * 3000.0f;
    float tk = (T_min + tf * (T_max - T_min)) / 100.0f;
    float cr = 1.0f, cg, cb = 1.0f;   // _color_temp_to_tint (render.py:2407-2437)
    if (tk > 66.0f) cr = fminf(fmaxf(1.292936f * powf(fmaxf(tk - 60.0f, 0.0001f), -0.1332047592f), 0.0f), 1.0f);
    if (tk <= 66.0f) cg = fminf(fmaxf(0.390082f * logf(fmaxf(tk, 0.0001f)) - 0.631841f, 0.0f), 1.0f);
    else cg = fminf(fmaxf(1.129891f * powf(fmaxf(tk - 60.0f, 0.0001f), -0.0755148492f), 0.0f), 1.0f);
    if (tk < 66.0f) cb = tk <= 19.0f ? 0.0f : fminf(fmaxf(0.543207f * logf(fmaxf(tk - 10.0f, 0.0001f)) - 1.19625f, 0.0f), 1.0f);
    cb = fminf(cb, cr);
    float lum = fminf(fmaxf(sqrtf(tf), 0.0f), 1.0f);
    return mk(fminf(fmaxf(cr * lum, 0.0f), 1.0f), fminf(fmaxf(cg * lum, 0.0f), 1.0f), fminf(fmaxf(cb * lum, 0.0f), 1.0f));
}
__device__ __forceinline__ float4 disk_v2_rgba(const BhrMarchArgs &a, float hit_x, float hit_y) {
    const bhr_disk_v2_params &p = *a.dv2;
    double r = sqrt((double)hit_x * hit_x + (double)hit_y * hit_y);
    double phi = atan2((double)hit_y, (double)hit_x) + (double)a.t_offset * dv2::omega_field(r, p);
    double F = dv2::structure_total(r, phi, p, a.dv2_norm_shear, a.dv2_norm_hotspot);
    double t = fmin(fmax(dv2::t_mid(r, p) * F / a.dv2_t_peak, 0.0), 1.0);
    double rho = fmin(fmax(dv2::rho_mid(r, p) * F, 0.0), 1.0);
    V3 c = disk_v2_color((float)t);
    return make_float4(c.x, c.y, c.z, (float)rho);
}

// Shared by both builds: shade one disk crossing and composite it front to back
// (render.py:2951-3002).  hit_x/hit_y: crossing point; to_cam: -direction at the START of the
// step (render.py:2954); hdx/hdy: x,y components of the hit differentials (DIFF only).
struct Shade {
    V3 accum;
    float alpha_total;
    int unsure;   // DIFF: some crossing's LOD sat within BHR_LOD_GUARD of a truncation boundary (read by the hybrid AA kernel only)
};
// A disk crossing waiting to be shaded.  Crossings of the lanes of a wave are spread over several
// RK4 steps (measured: ~6 wave-steps per tile see a hit, each with a handful of live lanes), and
// shading is ~700 instructions, so a hit is parked and shaded together with the other lanes' hits.
// Every lane has TWO parking slots: as soon as some lane has filled both, the wave shades the older
// hit of every lane that has one (front-to-back order is kept) and the second slot moves up; the rest
// is shaded when the wave has finished marching.  A lane can therefore always park the hit it finds,
// a step never has to be repeated, and the ray state is committed unconditionally.  Results are
// unchanged -- the same operations run later.
template <bool DIFF>
struct Pending {
    float hit_x, hit_y;
    V3 to_cam;
    float dxx, dxy, dyx, dyy;   // DIFF only
};
// The two parking slots of every lane live in LDS (9 x 2 floats per lane, bank-conflict free: consecutive
// lanes, consecutive words): they are touched a handful of times per ray, and in registers they cost the AA
// kernel a wave of occupancy (128 -> 149 VGPRs).
__shared__ float g_park[2][9][256];
extern __shared__ __attribute__((aligned(16))) float4 g_mip_lds[];   // SRC == 3: the coarse mip levels of the disk texture (dynamic)
template <bool DIFF>
__device__ __forceinline__ void park_store(int slot, const Pending<DIFF> &h) {
    const int t = threadIdx.x;
    g_park[slot][0][t] = h.hit_x;
    g_park[slot][1][t] = h.hit_y;
    g_park[slot][2][t] = h.to_cam.x;
    g_park[slot][3][t] = h.to_cam.y;
    g_park[slot][4][t] = h.to_cam.z;
    if (DIFF) {
        g_park[slot][5][t] = h.dxx;
        g_park[slot][6][t] = h.dxy;
        g_park[slot][7][t] = h.dyx;
        g_park[slot][8][t] = h.dyy;
    }
}
template <bool DIFF>
__device__ __forceinline__ Pending<DIFF> park_load(int slot) {
    const int t = threadIdx.x;
    Pending<DIFF> h;
    h.hit_x = g_park[slot][0][t];
    h.hit_y = g_park[slot][1][t];
    h.to_cam = mk(g_park[slot][2][t], g_park[slot][3][t], g_park[slot][4][t]);
    if (DIFF) {
        h.dxx = g_park[slot][5][t];
        h.dxy = g_park[slot][6][t];
        h.dyx = g_park[slot][7][t];
        h.dyy = g_park[slot][8][t];
    } else {
        h.dxx = h.dxy = h.dyx = h.dyy = 0.0f;
    }
    return h;
}
// the oldest parked crossing of a lane that has one (n_pend > 0) leaves its slot, the second slot moves up
template <bool DIFF>
__device__ __forceinline__ Pending<DIFF> park_pop(int &n_pend) {
    const Pending<DIFF> h = park_load<DIFF>(0);
    if (n_pend == 2) park_store<DIFF>(0, park_load<DIFF>(1));
    n_pend -= 1;
    return h;
}
// f: the block the two fields that are a FRAME's own are read from, t_offset and cp (the disk's roll, the observer) -- `a` itself
// in every march (the overload below).  A shutter frame from the ray map shades one set of records as several frames: it hands
// over a block that holds each sample's two fields and leaves the kernel's argument block, with the mip tables the lanes index,
// where it is (march_raymap.hip).
// ONLY f.t_offset and f.cp may be read through f, here and in apply_g_factor: raymap_shade_shutter_kernel sets those four floats
// and leaves the rest of its block uninitialised; any other field (f.r_inner, f.sc ...) would be garbage in that kernel alone.
// f is a BhrMarchArgs and not a two-field type of its own on purpose: read through the same struct type, the two fields keep
// the access metadata they had as a.t_offset / a.cp, and every existing march kernel compiles to the bytes it had (passing
// them as a float reference and a pointer was tried: the scalar loads of the strict kernels merged differently and their
// .text moved).  That identity is the compiler's doing, not a guarantee: after ANY edit to shade_hit, apply_g_factor or their
// callers re-run tools/code_object_diff.py against the parent build (profiles/raymap_shutter_code_objects.txt is the last run).
template <bool DIFF, int SRC>
__device__ __forceinline__ void shade_hit(const BhrMarchArgs &a, const BhrMarchArgs &f, Shade &sh, float hit_x, float hit_y,
                                          V3 to_cam, float hdx_x, float hdx_y, float hdy_x, float hdy_y, float obs_d = 1.0f) {
    float hit_r = sqrtf(hit_x * hit_x + hit_y * hit_y);
    if (!(a.r_outer >= hit_r && hit_r >= a.r_inner)) return;
    float hit_z = hit_y * a.tan_t;
    int lod_i = 0;
    if (DIFF) {
        // texture-space footprint from the ray differentials (render.py:2964-2988); same evaluation
        // order as the reference in both builds: the LOD is truncated to an integer level
        float hit_r_cyl = sqrtf(hit_x * hit_x + hit_y * hit_y + 1e-6f);
        float den = hit_r_cyl * hit_r_cyl + 1e-6f;
        float w_f = (float)a.sc.n_phi, h_f = (float)a.sc.n_r, span = a.r_outer - a.r_inner;
        float dr_dx = (hit_x * hdx_x + hit_y * hdx_y) / hit_r_cyl;
        float dphi_dx = (-hit_y * hdx_x + hit_x * hdx_y) / den;
        float dudx = dphi_dx * w_f / (2.0f * BHR_PI_F), dvdx = dr_dx * h_f / span;
        float dr_dy = (hit_x * hdy_x + hit_y * hdy_y) / hit_r_cyl;
        float dphi_dy = (-hit_y * hdy_x + hit_x * hdy_y) / den;
        float dudy = dphi_dy * w_f / (2.0f * BHR_PI_F), dvdy = dr_dy * h_f / span;
        float grad_sq = fmaxf(dudx * dudx + dvdx * dvdx, dudy * dudy + dvdy * dvdy);
        float lod = logf(fmaxf(grad_sq, 1.0f)) / logf(2.0f) * a.aa_strength;
        {
            // the level is int(clamp(lod, 0, 3)): it jumps at lod = 1, 2, 3.  A crossing whose lod lies within the guard
            // band of a jump may pick another level under a different rounding of the differentials
            const float fr = lod - floorf(lod);
            if (lod > 0.5f && lod < 3.5f && (fr < BHR_LOD_GUARD || fr > 1.0f - BHR_LOD_GUARD)) sh.unsure = 1;
        }
        lod = fminf(fmaxf(lod, 0.0f), 3.0f);
        lod_i = (int)fminf(fmaxf(lod, 0.0f), (float)(BHR_NUM_MIP_LEVELS - 1));
        // _sample_disk_mip clamps to num_mip_levels - 1 with the levels the chain HAS (render.py:2613): a 4 x 12 texture stops at
        // level 2 (1 x 3), and the levels beyond the last hold nothing -- their offset is the end of the stack.  As an integer
        // minimum with the scalar argument (int(min(x, n)) = min(int(x), n) for x >= 0): the float form keeps (float)mip_last
        // in a VGPR across the march loop
        lod_i = min(lod_i, a.sc.mip_last);
    }
    // SRC == 1 is a separate kernel instantiation: the binary64 model code (and its registers) never
    // touches the texture kernels
    float4 rgba = SRC == 1 ? disk_v2_rgba(a, hit_x, hit_y)
                  : SRC == 3 ? sample_disk_level(a.sc, hit_x, hit_y, a.r_inner, a.r_outer, f.t_offset, lod_i, g_mip_lds, a.mip_lds_from)
                             : sample_disk_level(a.sc, hit_x, hit_y, a.r_inner, a.r_outer, f.t_offset, lod_i);
    float base_alpha = fminf(rgba.w, 0.999f);
    float disk_alpha = 1.0f - powf(1.0f - base_alpha, BHR_DISK_ALPHA_GAIN);
    V3 col = apply_g_factor(a, f, mk(rgba.x, rgba.y, rgba.z), mk(hit_x, hit_y, hit_z), hit_r, to_cam, obs_d);
    float front = 1.0f - sh.alpha_total;
#if BHR_RAY_STRICT
    sh.accum = mk(sh.accum.x + col.x * disk_alpha * front, sh.accum.y + col.y * disk_alpha * front,
                  sh.accum.z + col.z * disk_alpha * front);
#else
    float wgt = disk_alpha * front;
    sh.accum = mk(fmaf(col.x, wgt, sh.accum.x), fmaf(col.y, wgt, sh.accum.y), fmaf(col.z, wgt, sh.accum.z));
#endif
    sh.alpha_total = 1.0f - front * (1.0f - disk_alpha);
}
template <bool DIFF, int SRC>
__device__ __forceinline__ void shade_hit(const BhrMarchArgs &a, Shade &sh, float hit_x, float hit_y, V3 to_cam,
                                          float hdx_x, float hdx_y, float hdy_x, float hdy_y) {
    shade_hit<DIFF, SRC>(a, a, sh, hit_x, hit_y, to_cam, hdx_x, hdx_y, hdy_x, hdy_y);
}

// Finite-thickness Disk V2 (docs/design_ad_v2.md 4.2-4.3, Phase 3 -- specified there, not implemented in
// the reference): emission-absorption through the volume |zeta| <= H(r), r_in <= r <= r_out of the tilted
// disk frame.  One RK4 step = one chord p0 -> p1, cut into vol_substeps pieces sampled at their midpoints:
//   rho = rho(r, zeta) F(r, phi_adv),  T = T(r, zeta) F,  phi_adv = phi + t_offset Omega(r)   (Phase 2)
//   alpha_eff = Ca rho [1 + kg (1 - |d.n|)]                                   (grazing-angle gain, 4.3)
//   opacity of the piece a = 1 - exp(-alpha_eff ds), source colour = black body of T with the g-factor,
// composited front to back exactly like a surface crossing (render.py:3000-3002), which is the design's
// L += exp(-tau) j ds, tau += alpha ds with j = alpha S integrated exactly over each piece.
// Model in binary64 (shared with the field evaluator), compositing in f32.
__device__ __forceinline__ void volume_segment(const BhrMarchArgs &a, Shade &sh, V3 p0, V3 p1, V3 dir0, float f0, float f1,
                                               float r0, float r1) {
    const bhr_disk_v2_params &P = *a.dv2;
    const double ct = (double)a.cos_t, st = (double)a.sin_t;
    const double z0 = (double)f0 * ct, z1 = (double)f1 * ct;           // heights above the disk plane
    const bool near_plane = z0 * z1 < 0.0 || fmin(fabs(z0), fabs(z1)) <= a.vol_h_max;
    // Bounding slab.  A chord that does not cross the plane is nearest to it at an end, and farthest from the origin at an
    // end, so those two tests read the ends alone.  It is NEAREST to the origin in between: two ends beyond vol_r_max can
    // have the volume's rim between them (a chord of length l tangent at radius r dips l^2 / 8r inside its ends: 0.03 at
    // step_size 0.5 and r = 10, twice the 0.015 by which vol_r_max exceeds r_out for the default disk).  No point of the
    // chord is farther than half its length from the nearer end; 0.51 covers the f32 rounding of r0, r1 and the length
    const float cx = p1.x - p0.x, cy = p1.y - p0.y, cz = p1.z - p0.z;
    const float reach = 0.51f * sqrtf(cx * cx + cy * cy + cz * cz);
    if (!(near_plane && (double)fmaxf(r0, r1) >= P.r_in && (double)(fminf(r0, r1) - reach) <= a.vol_r_max)) return;
    if (sh.alpha_total >= BHR_VOLUME_OPAQUE) return;     // what lies behind contributes < 1e-4 of its colour
    const double ex = (double)p1.x - (double)p0.x, ey = (double)p1.y - (double)p0.y, ez = (double)p1.z - (double)p0.z;
    const double len = sqrt(ex * ex + ey * ey + ez * ez);
    if (!(len > 0.0)) return;
    const double mu = fabs((ez * ct - ey * st) / len);
    const double ds = len / (double)a.vol_substeps;
    const V3 to_cam = mk(-dir0.x, -dir0.y, -dir0.z);
    for (int k = 0; k < a.vol_substeps; ++k) {
        const double f = ((double)k + 0.5) / (double)a.vol_substeps;
        const double sx = (double)p0.x + f * ex, sy = (double)p0.y + f * ey, sz = (double)p0.z + f * ez;
        const double zeta = sz * ct - sy * st;
        const double yp = sy * ct + sz * st;
        const double rc = sqrt(sx * sx + yp * yp);
        if (!dv2::volume_mask(rc, zeta, P)) continue;
        const double phi = atan2(yp, sx) + (double)a.t_offset * dv2::omega_field(rc, P);
        const double F = dv2::structure_total(rc, phi, P, a.dv2_norm_shear, a.dv2_norm_hotspot);
        const double rho = fmax(dv2::rho_field(rc, zeta, P) * F, 0.0);
        const double t = fmin(fmax(dv2::t_field(rc, zeta, P) * F / a.dv2_t_peak, 0.0), 1.0);
        const double alpha_eff = a.vol_absorption * rho * (1.0 + a.vol_grazing_gain * (1.0 - mu));
        const float op = (float)(1.0 - exp(-alpha_eff * ds));
        if (!(op > 0.0f)) continue;
        V3 col = apply_g_factor(a, disk_v2_color((float)t), mk((float)sx, (float)sy, (float)sz), (float)rc, to_cam);
        const float front = 1.0f - sh.alpha_total;
        sh.accum = mk(sh.accum.x + col.x * op * front, sh.accum.y + col.y * op * front, sh.accum.z + col.z * op * front);
        sh.alpha_total = 1.0f - front * (1.0f - op);
    }
}

// render.py:3008-3018: background through the accumulated opacity + clamped disk layer -- the two values a ray leaves
__device__ __forceinline__ void pixel_values(const BhrMarchArgs &a, bool escaped, V3 esc_dir, const Shade &sh, float bk[3], float dk[3]) {
    V3 bg = mk(0, 0, 0);
    if (escaped) bg = sample_skybox(a.sc, normalized(esc_dir));
    float k = 1.0f - sh.alpha_total;
    bk[0] = __fmul_rn(bg.x, k);
    bk[1] = __fmul_rn(bg.y, k);
    bk[2] = __fmul_rn(bg.z, k);
    dk[0] = fminf(fmaxf(sh.accum.x, 0.0f), 1.0f);
    dk[1] = fminf(fmaxf(sh.accum.y, 0.0f), 1.0f);
    dk[2] = fminf(fmaxf(sh.accum.z, 0.0f), 1.0f);
}

// Stores the pixel (i, j) = column, local row of a frame `width` pixels wide.
__device__ __forceinline__ void store_pixel(const BhrMarchArgs &a, int i, int j, int width, const float bk[3], const float dk[3]) {
    size_t o = ((size_t)j * width + i) * 3;
    a.bg[o + 0] = bk[0];
    a.bg[o + 1] = bk[1];
    a.bg[o + 2] = bk[2];
    a.disk[o + 0] = dk[0];
    a.disk[o + 1] = dk[1];
    a.disk[o + 2] = dk[2];
    if (a.diskp) {
        // bg + disk as the V pass would form it from the two stored layers (one rounding of the product, one of the sum):
        // its combine reads 12 bytes per pixel instead of 24
        a.sum[o + 0] = __fadd_rn(bk[0], dk[0]);
        a.sum[o + 1] = __fadd_rn(bk[1], dk[1]);
        a.sum[o + 2] = __fadd_rn(bk[2], dk[2]);
        // The disk layer once more for the split-f16 bloom (bloom.hip): every value x 2^14 cut into two f16 halves (hi =
        // RN16, lo = RN16 of the rest: 24 significant bits between them), laid out [channel][half][32-row block][8-pixel
        // group][row][8 pixels] -- the H pass's MFMA operand order.  The 8x8 tile of a wave is ONE 128-byte line of it per
        // channel and half: six fully coalesced 2-byte stores per pixel instead of a 96-byte-per-lane gather and a cut in
        // the H kernel.
        const size_t part = (size_t)a.dp_yb * a.dp_gp * 256;
        _Float16 *q = a.diskp + ((((size_t)(j >> 5)) * a.dp_gp + (i >> 3) + a.dp_g0) * 32 + (j & 31)) * 8 + (i & 7);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = dk[c] * 16384.0f;
            asm volatile("" : "+v"(v));                          // one product, one conversion: the stored half and the one `lo` is
            unsigned int hb = __builtin_bit_cast(unsigned short, (_Float16)v);   // formed against are the same bits (bloom.hip: cut2)
            asm volatile("" : "+v"(hb));
            const _Float16 hi = __builtin_bit_cast(_Float16, (unsigned short)hb);
            q[(size_t)(2 * c) * part] = hi;
            q[(size_t)(2 * c + 1) * part] = (_Float16)(v - (float)hi);
        }
    }
}

__device__ __forceinline__ void write_pixel(const BhrMarchArgs &a, int i, int j, bool escaped, V3 esc_dir, const Shade &sh) {
    float bk[3], dk[3];
    pixel_values(a, escaped, esc_dir, sh, bk, dk);
    store_pixel(a, i, j, a.width, bk, dk);
}

// Supersampling (bhr_set_supersample, a.ss = k > 1): the march runs on the fine frame, k x k rays per output pixel, and
// resolves each group inside the wave.  The values of the group's rays are summed by a butterfly -- lane-xor masks
// 1 .. k/2 along x, then ystride .. ystride k/2 along y (ystride 8 in an 8x8 tile, k on a fix list) -- which is a pairwise
// tree over each sub-sample row and then one over the row sums; both lanes of a pair hold the same sum (f32 addition
// commutes).  The product with 1/k^2 is exact.  Every lane of the wave must be here; `have`: the lane holds a ray, `store`:
// its group is to be stored, by the lane at sub-sample (0, 0); (i, j) is the lane's fine pixel.
template <class RAY>
__device__ __forceinline__ void resolve_store(const BhrMarchArgs &a, const RAY &ray, bool have, bool store, int i, int j, int ystride) {
    float v[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (have) ray.values(a, v, v + 3);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        asm volatile("" : "+v"(v[c]));         // the products are rounded before they are summed (no contraction into the adds)
        for (int m = 1; m < a.ss; m <<= 1) {
            v[c] = v[c] + __shfl_xor(v[c], m, BHR_WAVE);
            asm volatile("" : "+v"(v[c]));     // ... and the tree keeps its order
        }
        for (int m = ystride; m < ystride * a.ss; m <<= 1) {
            v[c] = v[c] + __shfl_xor(v[c], m, BHR_WAVE);
            asm volatile("" : "+v"(v[c]));
        }
        v[c] = v[c] * a.ss_inv;
    }
    const int io = i >> a.ss_log2, jo = j >> a.ss_log2;
    if (store && ((i | j) & (a.ss - 1)) == 0 && io < a.out_width && jo < a.out_rows) store_pixel(a, io, jo, a.out_width, v, v + 3);
}

// Pixel -> ray (render.py:2811-2840).  Returns the unit direction; dx1/dy1 = directions through
// the pixel one to the right / one below (differential seeds).
template <bool DIFF>
__device__ __forceinline__ V3 pixel_ray(const BhrMarchArgs &a, int i, int j_local, V3 &ddx, V3 &ddy) {
    const V3 cp = ld3(a.cp), cr = ld3(a.cr), cu = ld3(a.cu), cf = ld3(a.cf);
    V3 center = cp + 1.0f * cf;
    float half_w = a.pw * (float)a.width / 2;
    float half_h = a.ph * (float)a.height / 2;
    V3 tl = (center - half_w * cr) + half_h * cu;
    float px_f = (float)i, py_f = (float)(j_local + a.row0);
    V3 pixel_pos = (tl + ((px_f + 0.5f) * a.pw) * cr) - ((py_f + 0.5f) * a.ph) * cu;
    V3 ray_dir = normalized(pixel_pos - cp);
    if (DIFF) {
        V3 ppx1 = (tl + ((px_f + 1.5f) * a.pw) * cr) - ((py_f + 0.5f) * a.ph) * cu;
        ddx = normalized(ppx1 - cp) - ray_dir;
        V3 ppy1 = (tl + ((px_f + 0.5f) * a.pw) * cr) - ((py_f + 1.5f) * a.ph) * cu;
        ddy = normalized(ppy1 - cp) - ray_dir;
    }
    return ray_dir;
}

__device__ __forceinline__ unsigned long long wave_sum_u32(unsigned int v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, BHR_WAVE);
    return s;
}

// The wave's index in the launch, one 8x8 tile (or 64 list entries) each: wave-uniform, a scalar register.
__device__ __forceinline__ int wave_slot() { return blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

}  // namespace
