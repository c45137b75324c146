// march_launch.hip -- the host half of the ray march: every march launch goes through bhr_launch_march.
//
// The march's device code is one object per source (the layout: march_device.h): march.hip fast, march_strict.hip,
// march_strict_ilp.hip with the ILP-first scheduler, march_raymap.hip, march_kerr_raymap.hip, and one per march variant (bhr_variant_row_of: its row
// names the object).  Each object hands its kernels over through a table (bhr_march_kernel_fast / _strict / _strict_ilp /
// _raymap, and the variant rows').  This file resolves the arithmetic, builds the kernel arguments -- a variant's block with
// its own words behind the march's (variant_args) -- keeps the tile order, the ray-step counters and the timing events, and
// picks the kernel of a launch (march_kernel).  What a launch works from is in its arguments -- the caller's bhr_march_call
// (camera, flags, stream, timing slot, end-event policy, supersampling factor, variant request) and, for one list of a hybrid
// march, a bhr_march_part -- never in fields a caller left in the context.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <xmmintrin.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "bhr_internal.h"

#ifndef BHR_WAVE_STAMPS_BUILD
#define BHR_WAVE_STAMPS_BUILD 0
#endif

namespace {

// Tile order of this context: 8x8 tiles of the marched frame (bhr_fine with factor ss) sorted by the distance of their centre
// from the centre of the FULL image (the camera looks at the hole, build_camera), nearest first.  Built once per context and
// supersampling factor (bhr_set_supersample releases it).
int32_t ensure_tile_order(bhr_ctx *ctx, int ss, int tiles_x, int n_tiles) {
    if (ctx->d_tile_order && ctx->tile_order_n == n_tiles && ctx->tile_order_ss == ss) return BHR_OK;
    if (ctx->d_tile_order) (void)hipFree(ctx->d_tile_order);
    ctx->d_tile_order = nullptr;
    std::vector<std::pair<float, int>> key((size_t)n_tiles);
    const bhr_fine_frame fr = bhr_fine(ctx, ss);
    const float cx = 0.5f * (float)fr.width, cy = 0.5f * (float)fr.height;
    for (int t = 0; t < n_tiles; ++t) {
        const float x = (float)((t % tiles_x) * 8 + 4) - cx, y = (float)(fr.row0 + (t / tiles_x) * 8 + 4) - cy;
        key[(size_t)t] = {x * x + y * y, t};
    }
    std::stable_sort(key.begin(), key.end(),
                     [](const std::pair<float, int> &l, const std::pair<float, int> &r) { return l.first < r.first; });
    // the host keeps a copy: a hybrid march partitions this order into its strict and fast lists (hybrid.hip)
    free(ctx->h_tile_order);
    ctx->h_tile_order = (int32_t *)malloc((size_t)n_tiles * sizeof(int32_t));
    if (!ctx->h_tile_order) return bhr_fail(BHR_ERR_NOMEM, "tile order: out of host memory");
    for (int t = 0; t < n_tiles; ++t) ctx->h_tile_order[t] = key[(size_t)t].second;
    BHR_HIP(hipMalloc((void **)&ctx->d_tile_order, (size_t)n_tiles * sizeof(int32_t)));
    BHR_HIP(hipMemcpy(ctx->d_tile_order, ctx->h_tile_order, (size_t)n_tiles * sizeof(int32_t), hipMemcpyHostToDevice));
    ctx->tile_order_n = n_tiles;
    ctx->tile_order_ss = ss;
    return BHR_OK;
}

// The fast arithmetic's tilt and |cam| as its launches have always computed them (host code built with -ffast-math): the
// tilt times the folded constant pi / 180, |cam| from the SSE reciprocal-square-root estimate and one Newton step.  Every
// fast ray starts from 1 / |cam| and the tilt's tangent, so these bits reach every pixel of a fast frame.
float fast_tilt_rad(float deg) { return deg * (BHR_PI_F * (1.0f / 180.0f)); }
float fast_sqrt(float s) {
#pragma clang fp contract(off)
    if (fabsf(s) < 1.17549435e-38f) return 0.0f;               // below FLT_MIN the estimate is not used
    const float y = _mm_cvtss_f32(_mm_rsqrt_ss(_mm_set_ss(s)));
    const float sy = s * y;
    return (sy * -0.5f) * (sy * y + -3.0f);
}

// The kernel of a launch and its grid (fn null: the part only records its bracket events).
//
//   arithmetic     request                                              kernel (object)
//   any            a march variant v (call.req.variant), whole block    its row's kernel: kernels(name, 0, ss) of bhr_variant_row_of(v)
//   any            BHR_MV_KERR / _EXACT under a Kerr Disk V2 source      march_kerr_dv2[_exact | _volume][_ss]_kernel (kerr_dv2)
//   any            a Kerr variant, fix list (part->repair == 2)         kerr_raymap_fix_kernel<RS, ss> (kerr_raymap)
//   any            hybrid part with n <= 0, not the fix list            none
//   strict         hybrid fix list (part->repair == 2)                  march_fix_kernel<diff> (strict_ilp)
//   fast / strict  Disk V2 volume source                                march_tile_kernel<false, 2> (own object)
//   fast / strict  Disk V2 analytic source                              march_tile_kernel<diff, 1> (own object)
//   fast / strict  BHR_PERSISTENT, texture, no row costs, no part       march_persistent_kernel<diff> (own object)
//   strict         texture, BHR_PERSISTENT with row costs or a part     march_tile_kernel<diff, 0> (strict)
//   strict         texture, otherwise                                   march_tile_aa_ilp / march_tile_plain_ilp (strict_ilp)
//   fast           hybrid fast list with guards (part->repair == 1)     march_tile_guard_kernel<diff, row costs>
//   fast           row costs                                            march_tile_kernel<diff, 0, true>
//   fast           AA, mip_lds on, no part, a level fits 44 KB          march_tile_mipstaged_kernel (sets ctx->mip_lds_from)
//   fast           AA otherwise                                         march_tile_kernel<true, 0> (ctx->mip_lds_from = -1)
//   fast           plain                                                march_tile_plain_fast
// The refinement of an adaptively supersampled frame (bhr_launch_adaptive) launches, behind the base march's kernels above:
//   strict         the detect kernel                                    adaptive_detect_kernel (strict)
//   fast / strict  Disk V2 volume / analytic source                     march_list_kernel<false, 2> / <diff, 1> (own object)
//   strict         texture (and the strict list of a hybrid frame)      march_list_kernel<diff, 0> (strict_ilp)
//   fast           texture (and the fast list of a hybrid frame)        march_list_kernel<diff, 0> (fast)
//
// part: the bhr_march_part of a hybrid march's launch (null: whole block).  diff: bhr_want_diff.  Grids: blocks of 4 waves, a
// wave per tile of the launch's list; a wave per 64 entries of the fix list's capacity; the persistent kernel enough blocks
// to fill the chip.
struct MarchKernel {
    const void *fn = nullptr;
    dim3 grid;
    size_t lds = 0;
};
MarchKernel march_kernel(bhr_ctx *ctx, BhrMarchArgs &a, const bhr_march_part *part, int math, uint32_t flags, bool diff, bhr_march_variant v) {
    MarchKernel k;
    k.grid = dim3((a.n_list + 3) / 4);
    const bool persistent = (flags & BHR_PERSISTENT) != 0;
    const int ss = a.ss > 1;                                   // the supersampled twins (bhr_render refuses the schedules they lack)
    const auto own = math == BHR_MATH_FAST ? bhr_march_kernel_fast : bhr_march_kernel_strict;
    // a variant: one arithmetic, one schedule, no lists (what it has no form for was refused before anything was launched)
    if (v != BHR_MV_NONE) {
        const bhr_variant_row &r = bhr_variant_row_of(v);
        // the overflow list of a frame from the Kerr ray map (part->repair == 2 under a Kerr variant): kerr_raymap_fix_kernel, its
        // SS form over the whole groups of a supersampled map's list (the grid is sized for the fine capacity)
        if (part && part->repair == 2 && r.kerr) {
            k.fn = bhr_march_kernel_kerr_raymap(BHR_MK_KERR_RAYMAP_FIX, v == BHR_MV_KERR_EXACT, ss);
            k.grid = dim3((a.fix_cap / 64 + 3) / 4);
            return k;
        }
        // the Kerr march's own Disk V2 source (bhr_set_kerr_disk_source): march_kerr_dv2.o's kernel of the source and the redshift
        const bool kerr_dv2 = (v == BHR_MV_KERR || v == BHR_MV_KERR_EXACT) && ctx->kerr_disk_source != BHR_DISK_TEXTURE;
        if (!part && !persistent && !a.row_steps && !a.dv2)
            k.fn = kerr_dv2 ? (diff ? nullptr : bhr_kerr_dv2_kernel(ctx->kerr_disk_source, v == BHR_MV_KERR_EXACT, ss)) : r.kernels(r.name, diff, ss);
        return k;
    }
    if (part && part->n <= 0 && part->repair != 2) return k;
    if (part && part->repair == 2) {
        k.fn = bhr_march_kernel_strict_ilp(BHR_MK_FIX, diff, ss);
        k.grid = dim3((a.fix_cap / 64 + 3) / 4);
        return k;
    }
    if (ctx->disk_source == BHR_DISK_V2_VOLUME) { k.fn = own(BHR_MK_VOLUME, 0, ss); return k; }
    if (a.dv2) { k.fn = own(BHR_MK_DV2, diff, ss); return k; }
    if (persistent && !a.row_steps && !part) {
        k.fn = own(BHR_MK_PERSISTENT, diff, ss);
        k.grid = dim3(std::min(std::max((a.n_tiles + 3) / 4, 1), 256 * 8));
        return k;
    }
    switch (math) {
    case BHR_MATH_STRICT:
        k.fn = persistent ? bhr_march_kernel_strict(BHR_MK_TILE, diff, ss) : bhr_march_kernel_strict_ilp(BHR_MK_TILE_ILP, diff, ss);
        return k;
    case BHR_MATH_FAST:
        if (part && part->repair == 1) {
            k.fn = bhr_march_kernel_fast(a.row_steps ? BHR_MK_GUARD_COSTS : BHR_MK_GUARD, diff, ss);
        } else if (a.row_steps) {
            k.fn = bhr_march_kernel_fast(BHR_MK_TILE_COSTS, diff, ss);
        } else if (diff) {
            // BHR_MIP_LDS=1: the coarse mip levels through LDS where any of them fits 44 KB (see the kernel; not supersampled)
            if (ctx->opt.mip_lds && !part && !ss) {
                const int last = 3;                                     // int(clamp(lod, 0, 3)): the coarsest level ever sampled
                for (int l = last; l >= 1; --l) {
                    if (a.sc.mip_h[last] <= 0 || a.sc.mip_w[last] <= 0) break;                  // a texture too small to have it
                    const size_t bytes = ((size_t)a.sc.mip_off[last] + (size_t)a.sc.mip_h[last] * a.sc.mip_w[last] - (size_t)a.sc.mip_off[l]) * sizeof(float4);
                    if (bytes > 44 * 1024) break;                       // 64 KB per block less the 18 KB of parking slots
                    a.mip_lds_from = l;
                    k.lds = bytes;
                }
            }
            ctx->mip_lds_from = a.mip_lds_from;
            k.fn = bhr_march_kernel_fast(a.mip_lds_from >= 0 ? BHR_MK_MIPSTAGED : BHR_MK_TILE, 1, ss);
        } else {
            k.fn = bhr_march_kernel_fast(BHR_MK_TILE, 0, ss);
        }
        return k;
    }
    return k;
}

}  // namespace

const void *bhr_kerr_dv2_kernel(int32_t source, int32_t mode, int32_t ss) {
    if (source == BHR_DISK_V2_VOLUME) return mode == BHR_REDSHIFT_EXACT ? nullptr : bhr_march_kernel_kerr_dv2(BHR_MK_VOLUME, 0, ss);
    if (source == BHR_DISK_V2) return bhr_march_kernel_kerr_dv2(mode == BHR_REDSHIFT_EXACT ? BHR_MK_KERR_EXACT : BHR_MK_DV2, 0, ss);
    return nullptr;
}

// The arithmetic of a march: the context's math_mode unless the call forces one.  Hybrid is launches over complementary tile
// lists (hybrid.hip); the schedules and disk sources that have no list form run strict.  bhr_frame_begin picks the frame's
// post-pass kernels from the same decision (frame_slot.hip).
int32_t bhr_resolve_math(const bhr_ctx *ctx, uint32_t flags) {
    int32_t mode = ctx->cfg.math_mode;
    if (flags & BHR_FORCE_FAST) mode = BHR_MATH_FAST;
    if (flags & BHR_FORCE_STRICT) mode = BHR_MATH_STRICT;
    if (flags & BHR_FORCE_HYBRID) mode = BHR_MATH_HYBRID;
    if (mode == BHR_MATH_HYBRID && (ctx->disk_source != BHR_DISK_TEXTURE || (flags & BHR_PERSISTENT))) mode = BHR_MATH_STRICT;
    return mode;
}

int32_t bhr_ensure_tile_order(bhr_ctx *ctx, int32_t ss) {
    const bhr_fine_frame fr = bhr_fine(ctx, ss);
    const int tiles_x = (fr.width + 7) / 8;
    return ensure_tile_order(ctx, ss, tiles_x, tiles_x * ((fr.rows + 7) / 8));
}

// {VGPRs, LDS bytes, scratch bytes per lane} of the kernel that marches a whole texture frame (ss: its supersampled twin): variant
// v's own, else the fast object's under fast arithmetic, the ILP object's under strict and hybrid.  No context: host + hipFuncGetAttributes.
int32_t bhr_march_resources(const char *who, bhr_march_variant v, int32_t math, int32_t diff, int32_t ss, int32_t out[3]) {
    if (!out) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    const bhr_variant_row &r = bhr_variant_row_of(v);
    const void *f = v != BHR_MV_NONE         ? r.kernels(r.name, r.kerr ? diff : 0, ss ? 1 : 0)
                    : math == BHR_MATH_FAST ? bhr_march_kernel_fast(BHR_MK_TILE, diff, ss ? 1 : 0)
                                            : bhr_march_kernel_strict_ilp(BHR_MK_TILE_ILP, diff, ss ? 1 : 0);
    if (!f) return bhr_fail(BHR_ERR_STATE, "%s: no such march kernel in this library", who);
    hipFuncAttributes at;
    BHR_HIP(hipFuncGetAttributes(&at, f));
    out[0] = at.numRegs;
    out[1] = (int32_t)at.sharedSizeBytes;
    out[2] = (int32_t)at.localSizeBytes;
    return BHR_OK;
}

// The kernel argument block of a march of the frame bhr_fine(ctx, ss) under the fast or the strict arithmetic: everything but
// the launch's own list, row-cost and diagnostic pointers.  ss: the call's factor for the base march, ada_k for the refinement.
// Reads the context and the active frame slot, writes neither (layers_stored notes what a launch that stores layers changes).
static void march_args(const bhr_ctx *ctx, const bhr_march_call &call, const bhr_march_part *part, int32_t ss, bool fast, BhrMarchArgs &a) {
    const bhr_config &c = ctx->cfg;
    const bhr_camera *cam = call.cam;
    for (int k = 0; k < 3; ++k) {
        a.cp[k] = cam->pos[k];
        a.cr[k] = cam->right[k];
        a.cu[k] = cam->up[k];
        a.cf[k] = cam->forward[k];
    }
    // supersampling: the march marches the fine frame (bhr_fine) at the fine pitch, and stores the resolved output frame
    const bhr_fine_frame fr = bhr_fine(ctx, ss);
    const bhr_camera fcam = bhr_fine_camera(cam, ss);
    a.pw = fcam.pixel_width;
    a.ph = fcam.pixel_height;
    a.r_esc = cam->r_escape;
    a.r_esc2 = a.r_esc * a.r_esc;
    a.h_base = c.step_size;
    a.r_inner = c.r_disk_inner;
    a.r_outer = c.r_disk_outer;
    a.t_offset = cam->t_offset;
    // render.py:2808: tilt_rad = disk_tilt * pi / 180 in f32
    a.tilt_rad = fast ? fast_tilt_rad(c.disk_tilt_deg) : c.disk_tilt_deg * BHR_PI_F / 180.0f;
    a.tan_t = tanf(a.tilt_rad);
    a.sin_t = sinf(a.tilt_rad);
    a.cos_t = cosf(a.tilt_rad);
    a.aa_strength = c.aa_strength;
    // orbital-plane basis shared by all rays (fast build): e1 = cam / |cam|
    const float r0sq = a.cp[0] * a.cp[0] + a.cp[1] * a.cp[1] + a.cp[2] * a.cp[2];
    a.r0 = fast ? fast_sqrt(r0sq) : sqrtf(r0sq);
    for (int k = 0; k < 3; ++k) a.e1[k] = a.cp[k] / a.r0;
    a.A = a.e1[2] - a.e1[1] * a.tan_t;
    // render.py:2817-2818
    a.max_iter = (int32_t)(a.r_esc * 40.0f / a.h_base);
    a.max_affine = a.r_esc * 40.0f;
    a.max_affine_u = a.max_affine / a.h_base;      // fast build: the affine parameter in units of h_base
    a.width = fr.width;
    a.height = fr.height;
    a.row0 = fr.row0;
    a.rows = fr.rows;
    a.ss = ss;
    a.ss_log2 = bhr_log2(ss);
    a.ss_inv = 1.0f / (float)(ss * ss);
    a.out_width = c.width;
    a.out_rows = ctx->rows;
    a.sc.skybox = ctx->d_skybox;
    a.sc.sky_h = ctx->sky_h;
    a.sc.sky_w = ctx->sky_w;
    a.sc.mips = ctx->d_mips;
    for (int l = 0; l < BHR_NUM_MIP_LEVELS; ++l) {
        a.sc.mip_off[l] = ctx->mip_off[l];
        a.sc.mip_h[l] = ctx->mip_h[l];
        a.sc.mip_w[l] = ctx->mip_w[l];
    }
    a.sc.n_r = ctx->n_r;
    a.sc.n_phi = ctx->n_phi;
    a.sc.mip_last = 0;
    for (int l = 1; l < BHR_NUM_MIP_LEVELS && ctx->mip_h[l] > 0 && ctx->mip_w[l] > 0; ++l) a.sc.mip_last = l;
    const bhr_frame_slot &f = bhr_slot(ctx);
    a.bg = f.d_bg;
    a.disk = f.d_disk;
    a.diskp = nullptr;
    a.dp_yb = a.dp_gp = a.dp_g0 = 0;
    a.sum = nullptr;
    if (f.frame_split && f.d_pa && f.d_sum && !(call.flags & BHR_SKIP_BLOOM)) {      // split-f16 post-pass: the march feeds its H pass directly
        bhr_split_geom g;
        bhr_split_geometry(ctx, &g);
        a.diskp = (_Float16 *)f.d_pa;
        a.dp_yb = g.YB;
        a.dp_gp = g.GP;
        a.dp_g0 = g.g0;
        a.sum = f.d_sum;
    }
    // timed launches (bhr_render) count into their ring slot; group launches into the scalar
    a.ray_steps = bhr_steps_cell(ctx, call.slot);
    a.queue = f.d_queue;
    a.dv2 = ctx->disk_source != BHR_DISK_TEXTURE ? ctx->d_dv2_params : nullptr;
    a.vol_absorption = ctx->vol_opts[0];
    a.vol_grazing_gain = ctx->vol_opts[1];
    a.vol_h_max = ctx->vol_opts[2];
    a.vol_r_max = ctx->vol_opts[3];
    a.vol_substeps = ctx->vol_substeps;
    a.dv2_norm_shear = ctx->dv2_norm[0];
    a.dv2_norm_hotspot = ctx->dv2_norm[1];
    a.dv2_t_peak = ctx->dv2_norm[2];
    a.tiles_x = (fr.width + 7) / 8;
    a.n_tiles = a.tiles_x * ((fr.rows + 7) / 8);
    a.n_list = a.n_tiles;
    a.mip_lds_from = -1;
    a.fix_count = part ? part->fix_count : nullptr;
    a.fix_list = part ? part->fix_list : nullptr;
    a.fix_cap = part ? part->fix_cap : 0;
    a.row_steps = nullptr;
    a.wave_stamps = nullptr;
    a.tile_order = nullptr;
}

// What a launch that stores the active slot's BG / DISK layers under the block `a` leaves in the slot: the march, with the list
// refinement behind it, the map shade and the fused shutter shade (the map build stores no layer).
static void layers_stored(bhr_ctx *ctx, const BhrMarchArgs &a) {
    bhr_frame_slot &f = bhr_slot(ctx);
    f.disk_wide = 0;                  // a marched disk layer lies in [0, 1]
    if (a.sum) f.sum_valid = 1;       // the split-f16 post-pass's bg + disk plane comes with the layers
}

// The first kernel argument of a launch: the finished march block `a` itself, or for a variant `a` copied into the variant's own
// block in `b` with its words behind it -- binary64, each rounded once (the variant's kernels take this block; nobody else reads it).
union VariantArgs {
    BhrKerrViewMarchArgs kerr;        // the model kernels read its first sizeof(BhrKerrMarchArgs) bytes, the exact ones' sizeof(BhrKerrExactMarchArgs)
    BhrProjectedMarchArgs observer;   // the observer's kernels its first sizeof(BhrObserverMarchArgs)
    BhrDelayMarchArgs delay;
};
static void *variant_args(const bhr_ctx *ctx, const bhr_variant_request &req, BhrMarchArgs &a, VariantArgs &b) {
    switch (req.variant) {
    case BHR_MV_KERR:
    case BHR_MV_KERR_EXACT:
    case BHR_MV_KERR_VIEW:
    case BHR_MV_KERR_VIEW_EXACT: {
        BhrKerrViewMarchArgs &k = b.kerr;
        static_cast<BhrMarchArgs &>(k) = a;
        // the spinning hole: a = A M with M = r_s / 2 and the horizon's radius
        const double A = (double)ctx->kerr_spin;
        k.kerr_a = (float)(0.5 * A);
        k.kerr_rplus = (float)(0.5 * (1.0 + sqrt(1.0 - A * A)));
        if (ctx->kerr_aa) k.aa_strength = ctx->kerr_aa_strength;       // the Kerr march's own LOD strength (bhr_set_kerr_anti_alias)
        // the Kerr march's own Disk V2 source (bhr_set_kerr_disk_source), for march_kerr_dv2.o's kernels alone: its parameter block,
        // norms and slab in the march block's Disk V2 words -- vol_r_max with the spin in it, sqrt(R^2 + a^2) (ray_kerr_dv2.h: the cull)
        if ((req.variant == BHR_MV_KERR || req.variant == BHR_MV_KERR_EXACT) && ctx->kerr_disk_source != BHR_DISK_TEXTURE) {
            k.dv2 = ctx->d_kerr_dv2_params;
            k.dv2_norm_shear = ctx->kerr_dv2_norm[0];
            k.dv2_norm_hotspot = ctx->kerr_dv2_norm[1];
            k.dv2_t_peak = ctx->kerr_dv2_norm[2];
            k.vol_h_max = ctx->kerr_vol_bound[0];
            k.vol_r_max = sqrt(ctx->kerr_vol_bound[1] * ctx->kerr_vol_bound[1] + 0.25 * A * A);
        }
        // ... and, for the exact-redshift kernels alone, the ISCO of the disk's sense of rotation (prograde for A >= 0) with the
        // energy and angular momentum of its orbit (Bardeen, Press, Teukolsky 1972; M = 1/2, signed a, an orbit in the +phi sense)
        k.isco_r = k.isco_e = k.isco_l = 0.0f;
        if (req.variant == BHR_MV_KERR_EXACT || req.variant == BHR_MV_KERR_VIEW_EXACT) {
            const double M = 0.5, sa = 0.5 * A, q = fabs(A);
            const double z1 = 1.0 + cbrt(1.0 - q * q) * (cbrt(1.0 + q) + cbrt(1.0 - q));
            const double z2 = sqrt(3.0 * q * q + z1 * z1);
            const double root = sqrt(std::max((3.0 - z1) * (3.0 + z1 + 2.0 * z2), 0.0));
            const double r = M * (A >= 0.0 ? 3.0 + z2 - root : 3.0 + z2 + root);
            const double sm = sqrt(M), sr = sqrt(r);
            const double den = pow(r, 0.75) * sqrt(r * sr - 3.0 * M * sr + 2.0 * sa * sm);
            k.isco_r = (float)r;
            k.isco_e = (float)((r * sr - 2.0 * M * sr + sa * sm) / den);
            k.isco_l = (float)(sm * (r * r - 2.0 * sa * sm * sr + sa * sa) / den);
        }
        // ... and, for the Kerr camera's kernels alone, the camera behind that: the observer's words, then the projection's
        // (kind 0: the pinhole)
        if (req.variant == BHR_MV_KERR_VIEW || req.variant == BHR_MV_KERR_VIEW_EXACT) {
            const float *beta = req.observer->beta;
            const double gamma = 1.0 / sqrt(1.0 - ((double)beta[0] * beta[0] + (double)beta[1] * beta[1] + (double)beta[2] * beta[2]));
            for (int c = 0; c < 3; ++c) k.obs_beta[c] = beta[c];
            k.obs_gamma = (float)gamma;
            k.obs_g2 = (float)(gamma * gamma / (gamma + 1.0));
            k.obs_sky_shift = req.observer->sky_shift ? 1 : 0;
            k.proj_kind = 0;
            k.span_h = k.span_v = 0.0f;
            if (const bhr_projection *pr = req.projection) {
                const double rad = 3.14159265358979323846 / 180.0;
                k.proj_kind = pr->kind;
                k.span_h = pr->kind == BHR_PROJ_FISHEYE ? (float)((double)pr->fov_h_deg * rad / 2.0) : (float)((double)pr->fov_h_deg * rad);
                k.span_v = pr->kind == BHR_PROJ_FISHEYE ? 0.0f : (float)((double)pr->fov_v_deg * rad);
            }
        }
        return &k;
    }
    case BHR_MV_OBSERVER:
    case BHR_MV_PROJECTED: {
        BhrProjectedMarchArgs &o = b.observer;
        static_cast<BhrMarchArgs &>(o) = a;
        // the camera's velocity, gamma and gamma^2 / (gamma + 1)
        const float *beta = req.observer->beta;
        const double gamma = 1.0 / sqrt(1.0 - ((double)beta[0] * beta[0] + (double)beta[1] * beta[1] + (double)beta[2] * beta[2]));
        for (int c = 0; c < 3; ++c) o.obs_beta[c] = beta[c];
        o.obs_gamma = (float)gamma;
        o.obs_g2 = (float)(gamma * gamma / (gamma + 1.0));
        o.obs_sky_shift = req.observer->sky_shift ? 1 : 0;
        // a projection: its kind and its spans in radians behind that
        o.proj_kind = 0;
        o.span_h = o.span_v = 0.0f;
        if (req.variant == BHR_MV_PROJECTED) {
            const bhr_projection *pr = req.projection;
            const double rad = 3.14159265358979323846 / 180.0;
            o.proj_kind = pr->kind;
            o.span_h = pr->kind == BHR_PROJ_FISHEYE ? (float)((double)pr->fov_h_deg * rad / 2.0) : (float)((double)pr->fov_h_deg * rad);
            o.span_v = pr->kind == BHR_PROJ_FISHEYE ? 0.0f : (float)((double)pr->fov_v_deg * rad);
        }
        return &o;
    }
    case BHR_MV_DELAYED:
        static_cast<BhrMarchArgs &>(b.delay) = a;
        b.delay.delay_scale = req.delay->scale;
        return &b.delay;
    default:
        return &a;
    }
}

int32_t bhr_launch_march(bhr_ctx *ctx, const bhr_march_call &call, const bhr_march_part *part) {
    const uint32_t flags = call.flags;
    const hipStream_t stream = call.stream;
    const bhr_march_variant variant = call.req.variant;
    // a partial launch (part: one list of a hybrid march) marches the tiles of a caller-made list under the arithmetic the
    // caller chose; the first part records the start event and clears an untimed counter, the last part records the end event
    // a variant's frame is not selected by the context's math mode: one launch of the variant's object, its argument block the
    // strict one's (the post-pass has followed the math mode, bhr_frame_begin)
    const int math = part ? part->math : variant != BHR_MV_NONE ? BHR_MATH_STRICT : bhr_resolve_math(ctx, flags);
    if (math == BHR_MATH_HYBRID) return bhr_launch_march_hybrid(ctx, call);
    const bool fast = math == BHR_MATH_FAST;
    if (!ctx->d_skybox) return bhr_fail(BHR_ERR_STATE, "bhr_render: no skybox set (bhr_set_skybox)");
    if (!ctx->d_mips) return bhr_fail(BHR_ERR_STATE, "bhr_render: no disk texture set (bhr_set_disk_texture)");

    BhrMarchArgs a;
    march_args(ctx, call, part, call.ss, fast, a);
    layers_stored(ctx, a);
    const int slot = call.slot;
    const bool first_part = !part || part->first, last_part = !part || part->last;
    if (flags & BHR_ROW_COSTS) {
        // two profiles side by side: [0, n) the steps taken by the fast arithmetic, [n, 2n) by the strict one (a hybrid frame
        // fills both, from its two tile lists); cleared by the frame's first part, on the stream every other part follows
        const size_t n = (size_t)((ctx->rows + 7) / 8);
        if (!ctx->d_row_steps) BHR_HIP(hipMalloc((void **)&ctx->d_row_steps, 2 * n * sizeof(unsigned long long)));
        if (first_part) BHR_HIP(hipMemsetAsync(ctx->d_row_steps, 0, 2 * n * sizeof(unsigned long long), stream));
        a.row_steps = ctx->d_row_steps + (fast ? 0 : n);
    }
    // diagnostic (builds with -DBHR_WAVE_STAMPS_BUILD=1 only: the stamps cost the plain kernel three spilled registers):
    // BHR_WAVE_STAMPS=<file> dumps per-wave start / end times of THIS launch (tools/wave_timeline.py)
#if BHR_WAVE_STAMPS_BUILD
    const char *stamp_path = getenv("BHR_WAVE_STAMPS");
#else
    const char *stamp_path = nullptr;                          // the shipped library reads no environment on the render path
#endif
    unsigned long long *d_stamps = nullptr;
    if (stamp_path && stamp_path[0]) {
        BHR_HIP(hipMalloc((void **)&d_stamps, (size_t)a.n_tiles * 4 * sizeof(unsigned long long)));
        BHR_HIP(hipMemsetAsync(d_stamps, 0, (size_t)a.n_tiles * 4 * sizeof(unsigned long long), stream));
        a.wave_stamps = d_stamps;
    }
    if (part) {
        a.tile_order = part->d_list;
        a.n_list = part->n;
    } else {
        BHR_TRY(ensure_tile_order(ctx, call.ss, a.tiles_x, a.n_tiles));
        a.tile_order = ctx->d_tile_order;
    }

    // ring cells are cleared ahead of time (at reset, then by the previous frame's last kernel)
    if (slot < 0 && first_part) BHR_HIP(hipMemsetAsync(a.ray_steps, 0, sizeof(unsigned long long) * BHR_STEP_CELL, stream));
    if (flags & BHR_PERSISTENT) BHR_HIP(hipMemsetAsync(bhr_slot(ctx).d_queue, 0, sizeof(unsigned int), stream));
    // timed launches (bhr_render) use their ring slot's events, the others the context's scalar ones
    if (first_part && !call.keep_start) BHR_HIP(hipEventRecord(bhr_march_start_event(ctx, slot), stream));
    const MarchKernel k = march_kernel(ctx, a, part, math, flags, bhr_want_diff(ctx, flags, variant), variant);
    if (!k.fn && !(part && part->n <= 0 && part->repair != 2))
        return bhr_fail(BHR_ERR_STATE, "bhr_render: no march kernel for this launch (supersampling %d, flags %u)", call.ss, flags);
    if (k.fn) {
        int refill_below = 40;                                 // persistent schedule: refill a wave below 40 live lanes
        VariantArgs va;
        void *args[] = {variant_args(ctx, call.req, a, va), &refill_below};   // (the second argument is the persistent kernel's alone)
        (void)hipLaunchKernel(k.fn, k.grid, dim3(256), args, k.lds, stream);
    }
    BHR_HIP(hipGetLastError());
    // group / tile renders (slot < 0) record the march's end only on request: the event is a ~5 us bubble between the march and
    // the H pass of a tile whose whole tail is ~0.12 ms
    const bool timed = slot >= 0 || call.time_untimed;
    if (last_part && !call.defer_end && timed) BHR_HIP(hipEventRecord(bhr_march_end_event(ctx, slot), stream));
    if (d_stamps) {
        std::vector<unsigned long long> h((size_t)a.n_tiles * 4);
        BHR_HIP(hipMemcpyAsync(h.data(), d_stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        BHR_HIP(hipStreamSynchronize(stream));
        (void)hipFree(d_stamps);
        if (FILE *f = fopen(stamp_path, "wb")) { fwrite(h.data(), sizeof(unsigned long long), h.size(), f); fclose(f); }
    }
    return BHR_OK;
}

// Adaptive supersampling (bhr_set_adaptive_supersample), behind the frame's k = 1 march `call` on its stream: clear the counts ->
// [hybrid: flags of the fine frame's tiles] -> detect (mask + lists of fine tiles) -> refine (first list, second list) -> march-end event.  Nothing here
// waits for the device: the refinement's grids are sized for the lists' capacity, and waves beyond what the detect kernel listed exit at once.
int32_t bhr_launch_adaptive(bhr_ctx *ctx, const bhr_march_call &call) {
    const int k = ctx->ada_k, W = ctx->cfg.width, H = ctx->rows;
    const uint32_t flags = call.flags;
    const hipStream_t stream = call.stream;
    const int math = bhr_resolve_math(ctx, flags);
    bhr_frame_slot &f = bhr_slot(ctx);
    const int32_t fine_tiles_x = (W * k + 7) / 8, cap = fine_tiles_x * ((H * k + 7) / 8);   // tiles of the fine frame
    if (!f.d_ada_list) {
        // for every factor: the buffers outlive a change of k, and ceil(k W / 8) ceil(k H / 8) <= W H for k <= 8
        BHR_HIP(hipMalloc((void **)&f.d_ada_list, 2 * (size_t)W * H * sizeof(int32_t)));
        BHR_HIP(hipMalloc((void **)&f.d_ada_mask, (size_t)W * H));
        BHR_HIP(hipMalloc((void **)&f.d_ada_counts, 64));
    }
    if ((long long)cap > (long long)W * H) return bhr_fail(BHR_ERR_STATE, "adaptive supersampling: %d fine tiles for %d x %d pixels", cap, W, H);
    BHR_HIP(hipMemsetAsync(f.d_ada_counts, 0, 4 * sizeof(unsigned int), stream));
    BhrDetectArgs d;
    d.bg = f.d_bg;
    d.disk = f.d_disk;
    d.width = W;
    d.height = H;
    d.threshold = ctx->ada_threshold;
    d.k_log2 = bhr_log2(k);
    d.flags = nullptr;
    d.fine_tiles_x = fine_tiles_x;
    int32_t flag_tiles_x = fine_tiles_x;
    if (math == BHR_MATH_HYBRID) BHR_TRY(bhr_hybrid_fine_flags(ctx, call.cam, k, &d.flags, &flag_tiles_x));
    if (flag_tiles_x != fine_tiles_x) return bhr_fail(BHR_ERR_STATE, "adaptive supersampling: %d flag columns for %d tile columns", flag_tiles_x, fine_tiles_x);
    d.mask = f.d_ada_mask;
    d.list = f.d_ada_list;
    d.cap = cap;
    d.counts = f.d_ada_counts;
    {
        const int blocks = ((W + 7) / 8) * ((H + 7) / 8);            // a wave per 8 x 8 block of output pixels
        void *args[] = {&d};
        (void)hipLaunchKernel(bhr_march_kernel_strict(BHR_MK_DETECT, 0, 0), dim3((blocks + 3) / 4), dim3(256), args, 0, stream);
        BHR_HIP(hipGetLastError());
    }
    // the refinement marches the fine frame: the second argument block of the frame (ss = k, stores into the output frame)
    const bool want_diff = bhr_want_diff(ctx, flags);
    auto refine = [&](bool fast, int which) -> int32_t {
        BhrMarchArgs a;
        march_args(ctx, call, nullptr, k, fast, a);
        // a tile per wave, a grid for the list's capacity (every fine tile): waves beyond the list's length exit at once
        a.tile_order = f.d_ada_list + (size_t)which * cap;
        a.n_list = cap;
        a.fix_count = f.d_ada_counts + which;
        a.fix_list = (int32_t *)f.d_ada_mask;                           // LIST kernels read it as the mask (march_tile.h: list_refined)
        a.fix_cap = 0;
        if (a.n_tiles != cap) return bhr_fail(BHR_ERR_STATE, "adaptive supersampling: %d fine tiles, lists for %d", a.n_tiles, cap);
        const auto own = fast ? bhr_march_kernel_fast : bhr_march_kernel_strict;
        const void *fn = ctx->disk_source == BHR_DISK_V2_VOLUME ? own(BHR_MK_LIST_VOLUME, 0, 1)
                         : a.dv2                                 ? own(BHR_MK_LIST_DV2, want_diff, 1)
                         : fast                                  ? bhr_march_kernel_fast(BHR_MK_LIST, want_diff, 1)
                                                                 : bhr_march_kernel_strict_ilp(BHR_MK_LIST, want_diff, 1);
        if (!fn) return bhr_fail(BHR_ERR_STATE, "bhr_render: no list kernel for the refinement of this frame");
        void *args[] = {&a};
        (void)hipLaunchKernel(fn, dim3((cap + 3) / 4), dim3(256), args, 0, stream);
        BHR_HIP(hipGetLastError());
        return BHR_OK;
    };
    if (math == BHR_MATH_HYBRID) {
        BHR_TRY(refine(false, 0));       // longest rays first, as the base march has it
        BHR_TRY(refine(true, 1));
    } else {
        BHR_TRY(refine(math == BHR_MATH_FAST, 0));
    }
    if (call.slot >= 0 || call.time_untimed) BHR_HIP(hipEventRecord(bhr_march_end_event(ctx, call.slot), stream));
    return BHR_OK;
}

// ---- the ray maps (march_raymap.hip, march_kerr_raymap.hip; api_raymap.hip owns the maps) ------------------------------------------
// The kernels take the march's argument block of the strict frame and the map as a second argument.  A supersampled map (its
// own factor ss, option "raymap_supersample" or a Kerr map's "kerr_raymap_supersample"; the context's factor stays 1) takes the
// block of the fine frame, as a marched supersampled frame does, and the kernels' supersampled twins.  Under a Kerr variant the
// kernels are the Kerr map's, which take the Kerr block of the redshift (variant_args) in the march block's place: no
// differentials.
static const void *raymap_kernel(bhr_march_variant v, bhr_march_kernel plain, bhr_march_kernel kerr, bool diff, int32_t ss) {
    return v == BHR_MV_NONE ? bhr_march_kernel_raymap(plain, diff, ss > 1) : bhr_march_kernel_kerr_raymap(kerr, v == BHR_MV_KERR_EXACT, ss > 1);
}

int32_t bhr_launch_raymap_build(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags, const BhrRayMapArgs &m, int32_t ss, bhr_march_variant v, float *mom) {
    const char *api = v == BHR_MV_NONE ? "bhr_raymap_build" : "bhr_kerr_raymap_build";
    const hipStream_t stream = ctx->stream;
    const bhr_march_call call = {cam, flags | BHR_FORCE_STRICT, stream, /* slot */ -1, false, false, ss, false, {v}};
    BhrMarchArgs a;
    march_args(ctx, call, nullptr, ss, false, a);
    if ((int64_t)a.width * a.rows != m.plane) return bhr_fail(BHR_ERR_STATE, "%s: the map has %lld pixels, the frame %lld", api, (long long)m.plane, (long long)a.width * a.rows);
    if (ss == 1) {
        BHR_TRY(ensure_tile_order(ctx, 1, a.tiles_x, a.n_tiles));
        a.tile_order = ctx->d_tile_order;
    }
    // ss > 1: the fine tiles in plain order (tile_order null).  The context's tile order is keyed by the marched frame's factor,
    // and asking for the fine frame's would drop the order, the hybrid lists and the fix lists bhr_render's frames march over;
    // a build is a one-off, its ragged tail does not matter.
    a.ray_steps = m.stats + 8;                                 // a counter cell of the map's own, behind its totals
    const bool diff = bhr_want_diff(ctx, flags);
    if (m.comps != (diff ? 9 : 5)) return bhr_fail(BHR_ERR_STATE, "%s: %d components per record for differentials %d", api, m.comps, (int)diff);
    if (mom && v == BHR_MV_NONE) return bhr_fail(BHR_ERR_STATE, "%s: momentum planes are a Kerr build's", api);
    const void *fn = raymap_kernel(v, BHR_MK_RAYMAP_BUILD, mom ? BHR_MK_KERR_RAYMAP_BUILD_MOM : BHR_MK_KERR_RAYMAP_BUILD, diff, ss);
    if (!fn) return bhr_fail(BHR_ERR_STATE, "%s: no build kernel in this library", api);
    VariantArgs va;
    BhrRayMapMomArgs mm;               // the plain builds read its first sizeof(BhrRayMapArgs) bytes
    static_cast<BhrRayMapArgs &>(mm) = m;
    mm.mom = mom;
    void *args[] = {variant_args(ctx, call.req, a, va), &mm};
    (void)hipLaunchKernel(fn, dim3((a.n_list + 3) / 4), dim3(256), args, 0, stream);
    BHR_HIP(hipGetLastError());
    return BHR_OK;
}

// What the shade launchers begin with: a scene to shade, the argument block `a` of call's frame at factor ss, and a map that
// fits it.  api: the public call a refusal names.
static int32_t raymap_shade_args(bhr_ctx *ctx, const bhr_march_call &call, const BhrRayMapArgs &m, bool diff, int32_t ss, const char *api, BhrMarchArgs &a) {
    if (!ctx->d_skybox) return bhr_fail(BHR_ERR_STATE, "%s: no skybox set (bhr_set_skybox)", api);
    if (!ctx->d_mips) return bhr_fail(BHR_ERR_STATE, "%s: no disk texture set (bhr_set_disk_texture)", api);
    march_args(ctx, call, nullptr, ss, false, a);
    layers_stored(ctx, a);
    if ((int64_t)a.width * a.rows != m.plane || m.comps != (diff ? 9 : 5)) return bhr_fail(BHR_ERR_STATE, "%s: the map does not fit the frame", api);
    return BHR_OK;
}

// rot_c, rot_s: the turn about z of call.cam from the map's build camera (bhr_raymap_render_view); 1, 0 is no turn and takes the
// kernel without one, whose frame is the marched frame bit for bit.
int32_t bhr_launch_raymap_shade(bhr_ctx *ctx, const bhr_march_call &call, const BhrRayMapArgs &m, bool diff, float rot_c, float rot_s, const float *stars) {
    const char *api = call.req.variant == BHR_MV_NONE ? "bhr_raymap_render" : "bhr_kerr_raymap_render";
    // call.ss: the map's factor -- the block of the fine frame (k W x k rows, k^2 W rows == the map's plane), a wave per fine tile
    BhrMarchArgs a;
    BHR_TRY(raymap_shade_args(ctx, call, m, diff, call.ss, api, a));
    const bool turned = !(rot_c == 1.0f && rot_s == 0.0f);
    // stars: the STARS kernels of either map, which have no supersampled twins (the table then returns none)
    const bhr_march_kernel name = stars ? (turned ? BHR_MK_RAYMAP_SHADE_STARS_ROT : BHR_MK_RAYMAP_SHADE_STARS) : (turned ? BHR_MK_RAYMAP_SHADE_ROT : BHR_MK_RAYMAP_SHADE);
    const bhr_march_kernel kerr_name =
        stars ? (turned ? BHR_MK_KERR_RAYMAP_SHADE_STARS_ROT : BHR_MK_KERR_RAYMAP_SHADE_STARS) : (turned ? BHR_MK_KERR_RAYMAP_SHADE_ROT : BHR_MK_KERR_RAYMAP_SHADE);
    const void *fn = raymap_kernel(call.req.variant, name, kerr_name, diff, call.ss);
    if (!fn) return bhr_fail(BHR_ERR_STATE, "%s: no shade kernel in this library", api);
    // the frame's march bracket opens here; the overflow launch behind this one (bhr_launch_march, last part) closes it
    // (a later sample of a shutter frame from the map keeps the first sample's)
    if (!call.keep_start) BHR_HIP(hipEventRecord(bhr_march_start_event(ctx, call.slot), call.stream));
    VariantArgs va;
    BhrRayMapStarArgs mm;              // the kernels without stars read its first sizeof(BhrRayMapArgs) bytes
    static_cast<BhrRayMapArgs &>(mm) = m;
    mm.rot_c = rot_c;
    mm.rot_s = rot_s;
    mm.stars = stars;
    void *args[] = {variant_args(ctx, call.req, a, va), &mm};
    (void)hipLaunchKernel(fn, dim3((a.n_tiles + 3) / 4), dim3(256), args, 0, call.stream);
    BHR_HIP(hipGetLastError());
    return BHR_OK;
}

// The star plane of the map `m` under the catalogue `st`, seen from `cam` -- the build camera turned about z by (rot_c, rot_s) --
// into `out`: rows W 3 floats, and behind them the gather's three counts, cleared here ahead of the launch (stars.hip).  The
// march's block carries the view's camera and the frame's shape; the kernel reads nothing else of it -- and those are the words a
// Kerr block of the view begins with, so a Kerr map's plane is gathered under the same block by the same kernel.
int32_t bhr_launch_stars_gather(bhr_ctx *ctx, const bhr_stars *st, const bhr_camera *cam, const BhrRayMapArgs &m, float rot_c, float rot_s, float *out, hipStream_t stream) {
    if (!st || st->n <= 0) return bhr_fail(BHR_ERR_STATE, "star gather: no star catalogue (bhr_set_stars, bhr_set_kerr_stars)");
    const bhr_march_call call = {cam, BHR_FORCE_STRICT | BHR_SKIP_BLOOM, stream, /* slot */ -1, false, false, 1, false};
    BhrMarchArgs a;
    march_args(ctx, call, nullptr, 1, false, a);
    if ((int64_t)a.width * a.rows != m.plane) return bhr_fail(BHR_ERR_STATE, "star gather: the map has %lld pixels, the frame %lld", (long long)m.plane, (long long)a.width * a.rows);
    const bool turned = !(rot_c == 1.0f && rot_s == 0.0f);
    const void *fn = bhr_stars_kernel(turned ? 1 : 0);
    if (!fn) return bhr_fail(BHR_ERR_STATE, "star gather: no gather kernel in this library");
    BhrStarsArgs s;
    s.status = m.status;
    s.dir = m.dir;
    s.plane = m.plane;
    s.rot_c = rot_c;
    s.rot_s = rot_s;
    s.rec = st->d_rec;
    s.off = st->d_off;
    s.bins_theta = st->bins_theta;
    s.bins_phi = st->bins_phi;
    s.cos_span = st->cos_span;
    s.max_mag = st->params.max_magnification;
    s.out = out;
    s.counts = (unsigned int *)(out + (size_t)a.width * a.rows * 3);
    BHR_HIP(hipMemsetAsync(s.counts, 0, 4 * sizeof(unsigned int), stream));
    void *args[] = {&a, &s};
    (void)hipLaunchKernel(fn, dim3((a.width + 14) / 15, (a.rows + 14) / 15), dim3(256), args, 0, stream);
    BHR_HIP(hipGetLastError());
    return BHR_OK;
}

// The Stokes pass of a map frame (march_polar.hip, march_kerr_polar.hip; api_polar.hip owns the planes): the Stokes kernel on the
// shade kernel's grid under the block the shade launch of the same frame was given -- the march's block of call's frame, so
// shade_hit sees the values it saw there, or the Kerr block of call's Kerr variant -- then the cell means, one block per cell.
// The Kerr kernel is its redshift's and reads the map's momentum planes `mom` behind the map.  Stores no layer: the slot's
// BG / DISK and what is noted of them stay.
int32_t bhr_launch_stokes(bhr_ctx *ctx, const bhr_march_call &call, const BhrRayMapArgs &m, bool diff, float *mom, const BhrStokesArgs &s) {
    const bhr_march_variant v = call.req.variant;
    const bool kerr = v != BHR_MV_NONE;
    const char *who = kerr ? "Kerr polarisation" : "polarisation";
    if (kerr && v != BHR_MV_KERR && v != BHR_MV_KERR_EXACT) return bhr_fail(BHR_ERR_STATE, "%s: the frame is not a Kerr variant's", who);
    if (call.ss != 1) return bhr_fail(BHR_ERR_STATE, "%s: the Stokes kernel has no supersampled twin (factor %d)", who, call.ss);
    BhrMarchArgs a;
    march_args(ctx, call, nullptr, 1, false, a);
    // the Kerr map: no differentials, and the momentum planes; the Schwarzschild map: none
    if ((int64_t)a.width * a.rows != m.plane || m.comps != (diff ? 9 : 5) || s.width != a.width || s.rows != a.rows || (kerr ? diff || !mom : mom != nullptr))
        return bhr_fail(BHR_ERR_STATE, "%s: the map does not fit the frame", who);
    if (s.cell < 1 || s.gw != (a.width + s.cell - 1) / s.cell || s.gh != (a.rows + s.cell - 1) / s.cell || !s.out || !s.cells)
        return bhr_fail(BHR_ERR_STATE, "%s: a cell grid of %d x %d cells of %d pixels for a %d x %d frame", who, s.gw, s.gh, s.cell, a.width, a.rows);
    const void *fn = kerr ? bhr_kerr_stokes_kernel(v == BHR_MV_KERR_EXACT ? 1 : 0) : bhr_stokes_kernel(diff ? 1 : 0), *fc = bhr_stokes_cells_kernel();
    if (!fn || !fc) return bhr_fail(BHR_ERR_STATE, "%s: no Stokes kernel in this library", who);
    VariantArgs va;
    BhrRayMapMomArgs mm;               // the Schwarzschild kernel reads its first sizeof(BhrRayMapArgs) bytes
    static_cast<BhrRayMapArgs &>(mm) = m;
    mm.mom = mom;
    BhrStokesArgs ss = s;
    void *args[] = {variant_args(ctx, call.req, a, va), &mm, &ss};
    (void)hipLaunchKernel(fn, dim3((a.n_tiles + 3) / 4), dim3(256), args, 0, call.stream);
    BHR_HIP(hipGetLastError());
    void *cargs[] = {&ss};
    // whole waves, no more than the cell has pixels for: one wave for the 8 x 8 cell, four for 16 x 16 and 32 x 32
    const unsigned cell_threads = s.cell * s.cell >= 256 ? 256u : 64u;
    (void)hipLaunchKernel(fc, dim3(s.gw * s.gh), dim3(cell_threads), cargs, 0, call.stream);
    BHR_HIP(hipGetLastError());
    return BHR_OK;
}

// The Kerr line pass of a frame from the k = 1 Kerr map (march_kerr_line.hip; api_kerr_line.hip owns the rows and the planes): the
// kernel of call's redshift and of the emissivity under the Kerr block the shade launch of the same frame was given, over the
// shade kernel's tiles.  The grid is capped at BHR_LINE_MAX_BLOCKS workgroups of four waves, which stride over the tiles: a
// workgroup clears and flushes its n_bins + 4 LDS cells once, however many tiles it walks.  Stores no layer.
#define BHR_LINE_MAX_BLOCKS 1024
int32_t bhr_launch_kerr_line(bhr_ctx *ctx, const bhr_march_call &call, const BhrRayMapArgs &m, const BhrKerrLineArgs &s, bool texture) {
    const char *who = "Kerr line profile";
    const bhr_march_variant v = call.req.variant;
    if (v != BHR_MV_KERR && v != BHR_MV_KERR_EXACT) return bhr_fail(BHR_ERR_STATE, "%s: the frame is not a Kerr variant's", who);
    if (call.ss != 1) return bhr_fail(BHR_ERR_STATE, "%s: the kernel has no supersampled twin (factor %d)", who, call.ss);
    if (texture && !ctx->d_mips) return bhr_fail(BHR_ERR_STATE, "%s: no disk texture set (bhr_set_disk_texture)", who);
    BhrMarchArgs a;
    march_args(ctx, call, nullptr, 1, false, a);
    if ((int64_t)a.width * a.rows != m.plane || m.comps != 5 || m.slots < 1 || m.slots > 8) return bhr_fail(BHR_ERR_STATE, "%s: the map does not fit the frame", who);
    if (s.n_bins < 1 || s.n_bins > BHR_LINE_MAX_BINS || !s.row || (s.g_out == nullptr) != (s.w_out == nullptr))
        return bhr_fail(BHR_ERR_STATE, "%s: %d bins (1 .. %d), a row and both sample planes or none", who, s.n_bins, BHR_LINE_MAX_BINS);
    const void *fn = bhr_kerr_line_kernel(v == BHR_MV_KERR_EXACT ? 1 : 0, texture ? 1 : 0);
    if (!fn) return bhr_fail(BHR_ERR_STATE, "%s: no line kernel in this library", who);
    VariantArgs va;
    BhrRayMapArgs mm = m;
    BhrKerrLineArgs ss = s;
    void *args[] = {variant_args(ctx, call.req, a, va), &mm, &ss};
    const int blocks = (a.n_tiles + 3) / 4;
    const size_t lds = (size_t)(s.n_bins + 4) * sizeof(unsigned long long);
    (void)hipLaunchKernel(fn, dim3(blocks < BHR_LINE_MAX_BLOCKS ? blocks : BHR_LINE_MAX_BLOCKS), dim3(256), args, lds, call.stream);
    BHR_HIP(hipGetLastError());
    return BHR_OK;
}

// All samples of a shutter frame from the map in one launch (the fused route of bhr_raymap_render_shutter and
// bhr_kerr_raymap_render_shutter): the shade kernel's grid, the block of call.cam's frame -- the fields of it that a shade kernel
// reads of a camera, t_offset and the position, are taken from the samples' table inside the kernel instead -- the map, and that
// table by value.  Under a Kerr variant the kernel is the Kerr map's and the block the variant's Kerr block (variant_args: the
// spin, and the ISCO for the exact redshift).  The caller closes the march bracket.
int32_t bhr_launch_raymap_shade_shutter(bhr_ctx *ctx, const bhr_march_call &call, const BhrRayMapArgs &m, bool diff, const BhrShutterArgs &smp, bool turned) {
    const bhr_march_variant v = call.req.variant;
    const char *api = v == BHR_MV_NONE ? "bhr_raymap_render_shutter" : "bhr_kerr_raymap_render_shutter";
    if (v != BHR_MV_NONE && v != BHR_MV_KERR && v != BHR_MV_KERR_EXACT) return bhr_fail(BHR_ERR_STATE, "%s: the frame is not a Kerr variant's", api);
    BhrMarchArgs a;
    BHR_TRY(raymap_shade_args(ctx, call, m, diff, 1, api, a));
    if (smp.n < 1 || smp.n > BHR_SHUTTER_MAX_SAMPLES) return bhr_fail(BHR_ERR_INVALID, "%s: %d samples (1 .. %d)", api, smp.n, BHR_SHUTTER_MAX_SAMPLES);
    if (call.ss != 1) return bhr_fail(BHR_ERR_STATE, "%s: the fused launch has no supersampled kernel (factor %d)", api, call.ss);
    if (a.diskp) return bhr_fail(BHR_ERR_STATE, "%s: the fused launch takes a skip-bloom call (it stores no packed bloom operands)", api);
    const void *fn = raymap_kernel(v, turned ? BHR_MK_RAYMAP_SHUTTER_ROT : BHR_MK_RAYMAP_SHUTTER, turned ? BHR_MK_KERR_RAYMAP_SHUTTER_ROT : BHR_MK_KERR_RAYMAP_SHUTTER, diff, 1);
    if (!fn) return bhr_fail(BHR_ERR_STATE, "%s: no shutter shade kernel in this library", api);
    BHR_HIP(hipEventRecord(bhr_march_start_event(ctx, call.slot), call.stream));
    VariantArgs va;
    BhrRayMapArgs mm = m;
    BhrShutterArgs ss = smp;
    void *args[] = {variant_args(ctx, call.req, a, va), &mm, &ss};
    (void)hipLaunchKernel(fn, dim3((a.n_tiles + 3) / 4), dim3(256), args, 0, call.stream);
    BHR_HIP(hipGetLastError());
    return BHR_OK;
}
