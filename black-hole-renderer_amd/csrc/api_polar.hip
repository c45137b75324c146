// api_polar.hip -- the polarisation's entry points (include/bhr.h): bhr_set_polarization, bhr_read_stokes, bhr_read_stokes_cells,
// bhr_stokes_resources, and what a map frame asks of it (the Stokes pass into the frame slot's own planes).  The kernels are
// march_polar.hip's, their launcher march_launch.hip's; the frame itself is launched from render.hip.
// The Kerr polarisation (bhr_set_kerr_polarization, bhr_kerr_stokes_resources) is a second setting of the same struct for the
// frames from the Kerr ray map: the same planes, cell grid and reads; its kernel is march_kerr_polar.hip's.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "bhr_internal.h"

namespace {

const int32_t kMinCell = 8;

// every stream that may still write a slot's planes
int32_t drain(bhr_ctx *ctx) {
    for (auto &f : ctx->slots) {
        if (f.stream) BHR_HIP(hipStreamSynchronize(f.stream));
        if (f.aux_stream) BHR_HIP(hipStreamSynchronize(f.aux_stream));
    }
    BHR_HIP(hipStreamSynchronize(ctx->scene_stream));
    return BHR_OK;
}

size_t plane_floats(const bhr_ctx *ctx) { return (size_t)ctx->rows * ctx->cfg.width; }
int32_t cells_along(int32_t n, int32_t cell) { return (n + cell - 1) / cell; }

// the slot whose planes a read returns, behind the frame that wrote them
int32_t stokes_source(bhr_ctx *ctx, const char *who, const bhr_frame_slot **src) {
    if (!bhr_have_polar(ctx) && !bhr_have_kerr_polar(ctx)) return bhr_fail(BHR_ERR_STATE, "%s: no polarisation is set (bhr_set_polarization)", who);
    if (ctx->stokes_slot < 0 || !ctx->slots[ctx->stokes_slot].d_stokes || ctx->slots[ctx->stokes_slot].stokes_cell == 0)
        return bhr_fail(BHR_ERR_STATE, "%s: no frame from the ray map has been rendered with the polarisation set (bhr_raymap_render)", who);
    BHR_TRY(bhr_enter(ctx));
    *src = &ctx->slots[ctx->stokes_slot];
    return BHR_OK;
}

// what both setters refuse of the struct itself
int32_t check_struct(const bhr_ctx *ctx, const char *who, const bhr_polarization *p) {
    const double n2 = (double)p->b_r * p->b_r + (double)p->b_phi * p->b_phi + (double)p->b_z * p->b_z;
    if (!(isfinite(p->b_r) && isfinite(p->b_phi) && isfinite(p->b_z)) || !(n2 > 0.0) || !isfinite(n2))
        return bhr_fail(BHR_ERR_INVALID, "%s: polarisation field (%g, %g, %g): finite and not zero", who, (double)p->b_r, (double)p->b_phi, (double)p->b_z);
    if (!(p->fraction >= 0.0f && p->fraction <= 1.0f))      // a NaN fails the comparison too
        return bhr_fail(BHR_ERR_INVALID, "%s: polarisation fraction %g: in [0, 1] and no NaN", who, (double)p->fraction);
    if (p->cell != 8 && p->cell != 16 && p->cell != 32) return bhr_fail(BHR_ERR_INVALID, "%s: polarisation cell %d (8, 16 or 32)", who, p->cell);
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return bhr_fail(BHR_ERR_INVALID, "%s: polarisation with reserved words other than 0", who);
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "%s: polarisation needs a whole-frame context (rows %d of %d): group and tile contexts have no ray map", who, ctx->rows,
                        ctx->cfg.height);
    return BHR_OK;
}

// The pass of either kind into the active slot's planes under `pol`; under call's Kerr variant the launcher takes the Kerr map's
// kernel over its momentum planes.
int32_t stokes_frame(bhr_ctx *ctx, const bhr_march_call &call, const bhr_raymap &rm, const bhr_polarization &pol) {
    bhr_frame_slot &f = bhr_slot(ctx);
    // the slot is the sole owner of its planes; the grid is sized for the smallest cell, so a change of cell size keeps it
    if (!f.d_stokes) BHR_TRY(bhr_dev_alloc(&f.d_stokes, 3 * plane_floats(ctx)));
    if (!f.d_stokes_cells) BHR_TRY(bhr_dev_alloc(&f.d_stokes_cells, (size_t)cells_along(ctx->rows, kMinCell) * cells_along(ctx->cfg.width, kMinCell) * 3));
    BhrStokesArgs s;
    // the field's direction in binary64, rounded once (the setter refused a zero or non-finite one)
    const double b[3] = {pol.b_r, pol.b_phi, pol.b_z};
    const double norm = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    for (int k = 0; k < 3; ++k) s.b[k] = (float)(b[k] / norm);
    s.frac = pol.fraction;
    s.out = f.d_stokes;
    s.cells = f.d_stokes_cells;
    s.cell = pol.cell;
    s.width = ctx->cfg.width;
    s.rows = ctx->rows;
    s.gw = cells_along(s.width, s.cell);
    s.gh = cells_along(s.rows, s.cell);
    f.stokes_cell = 0;                 // until both launches are in the stream
    BHR_TRY(bhr_launch_stokes(ctx, call, rm.a, rm.diff != 0, rm.has_mom ? rm.mom : nullptr, s));
    f.stokes_cell = pol.cell;
    // the Stokes kernel calls shade_hit, so it samples the disk texture and its mips behind the frame's march bracket: it is the
    // frame's last reader of the scene, and a scene write (bhr_enter_scene_write) has to wait for it, not for the march's end
    if (!f.stokes_done) BHR_HIP(hipEventCreateWithFlags(&f.stokes_done, hipEventDisableTiming));
    BHR_HIP(hipEventRecord(f.stokes_done, call.stream));
    f.march_done = f.stokes_done;
    return BHR_OK;
}

}  // namespace

void bhr_polar_invalidate(bhr_ctx *ctx) {
    ctx->stokes_slot = -1;
    for (auto &f : ctx->slots) f.stokes_cell = 0;
}

int32_t bhr_polar_frame(bhr_ctx *ctx, const bhr_march_call &call, const bhr_raymap &rm) { return stokes_frame(ctx, call, rm, ctx->polar); }
int32_t bhr_kerr_polar_frame(bhr_ctx *ctx, const bhr_march_call &call, const bhr_raymap &rm) { return stokes_frame(ctx, call, rm, ctx->kerr_polar); }

extern "C" {

int32_t bhr_set_polarization(bhr_ctx *ctx, const bhr_polarization *p) {
    const char *who = "bhr_set_polarization";
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "%s: null ctx", who);
    if (p) {
        BHR_TRY(check_struct(ctx, who, p));
        if (ctx->kerr_on)
            return bhr_fail(BHR_ERR_INVALID, "%s: polarisation with a spin set (a / M = %g, bhr_set_spin): the transport rule is Schwarzschild's", who, (double)ctx->kerr_spin);
        if (ctx->disk_source != BHR_DISK_TEXTURE)
            return bhr_fail(BHR_ERR_INVALID, "%s: polarisation with the Disk V2 source (%d): a ray map shades the disk texture", who, ctx->disk_source);
    }
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(drain(ctx));               // a frame in flight may be writing the planes this makes unreadable
    bhr_polar_invalidate(ctx);
    if (!p) {
        ctx->polar_on = 0;
        memset(&ctx->polar, 0, sizeof(ctx->polar));
        return BHR_OK;
    }
    ctx->polar = *p;
    ctx->polar_on = 1;
    return BHR_OK;
}

int32_t bhr_set_kerr_polarization(bhr_ctx *ctx, const bhr_polarization *p) {
    const char *who = "bhr_set_kerr_polarization";
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "%s: null ctx", who);
    if (p) {
        BHR_TRY(check_struct(ctx, who, p));
        if (!ctx->kerr_on)
            return bhr_fail(BHR_ERR_STATE, "%s: no spin is set and the Kerr march is not forced (bhr_set_spin); bhr_set_polarization is the polarisation of a hole that does not spin", who);
    }
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(drain(ctx));               // a frame in flight may be writing the planes this makes unreadable
    bhr_polar_invalidate(ctx);
    if (!p) {
        ctx->kerr_polar_on = 0;
        memset(&ctx->kerr_polar, 0, sizeof(ctx->kerr_polar));
        return BHR_OK;
    }
    ctx->kerr_polar = *p;
    ctx->kerr_polar_on = 1;
    return BHR_OK;
}

int32_t bhr_read_stokes(bhr_ctx *ctx, int32_t plane, float *out) {
    const char *who = "bhr_read_stokes";
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    if (plane < 0 || plane > 2) return bhr_fail(BHR_ERR_INVALID, "%s: Stokes plane %d (0 I, 1 Q, 2 U)", who, plane);
    const bhr_frame_slot *f = nullptr;
    BHR_TRY(stokes_source(ctx, who, &f));
    const size_t n = plane_floats(ctx);
    return bhr_download(ctx, out, f->d_stokes + (size_t)plane * n, n * sizeof(float));
}

int32_t bhr_read_stokes_cells(bhr_ctx *ctx, float *out, int32_t dims[2]) {
    const char *who = "bhr_read_stokes_cells";
    if (!ctx || !dims) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    const bhr_frame_slot *f = nullptr;
    BHR_TRY(stokes_source(ctx, who, &f));
    dims[0] = cells_along(ctx->rows, f->stokes_cell);
    dims[1] = cells_along(ctx->cfg.width, f->stokes_cell);
    if (!out) return BHR_OK;
    return bhr_download(ctx, out, f->d_stokes_cells, (size_t)dims[0] * dims[1] * 3 * sizeof(float));
}

int32_t bhr_stokes_resources(int32_t diff, int32_t out[3]) {
    if (!out) return bhr_fail(BHR_ERR_INVALID, "bhr_stokes_resources: null argument");
    const void *f = bhr_stokes_kernel(diff ? 1 : 0);
    if (!f) return bhr_fail(BHR_ERR_STATE, "bhr_stokes_resources: no Stokes kernel in this library");
    hipFuncAttributes at;
    BHR_HIP(hipFuncGetAttributes(&at, f));
    out[0] = at.numRegs;
    out[1] = (int32_t)at.sharedSizeBytes;
    out[2] = (int32_t)at.localSizeBytes;
    return BHR_OK;
}

int32_t bhr_kerr_stokes_resources(int32_t redshift, int32_t out[3]) {
    if (!out) return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_stokes_resources: null argument");
    if (redshift != BHR_REDSHIFT_MODEL && redshift != BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_stokes_resources: unknown mode %d (BHR_REDSHIFT_MODEL = 0, BHR_REDSHIFT_EXACT = 1)", redshift);
    const void *f = bhr_kerr_stokes_kernel(redshift == BHR_REDSHIFT_EXACT ? 1 : 0);
    if (!f) return bhr_fail(BHR_ERR_STATE, "bhr_kerr_stokes_resources: no Kerr Stokes kernel in this library");
    hipFuncAttributes at;
    BHR_HIP(hipFuncGetAttributes(&at, f));
    out[0] = at.numRegs;
    out[1] = (int32_t)at.sharedSizeBytes;
    out[2] = (int32_t)at.localSizeBytes;
    return BHR_OK;
}

}  // extern "C"
