// settings.hip -- what changes the kind of frame a context renders: the spinning hole with its refusals, and the sampling.
#include <math.h>
#include <string.h>

#include "bhr_internal.h"

namespace {

int32_t kerr_state_check(const bhr_ctx *ctx, uint32_t flags, const char *who, double spin) {
    if (ctx->cfg.disk_tilt_deg != 0.0f)
        return bhr_fail(BHR_ERR_INVALID, "%s: spin %g with a disk tilted by %g degrees: the spin axis is the disk normal, tilt must be 0", who, spin, (double)ctx->cfg.disk_tilt_deg);
    if (ctx->cfg.anti_alias != 0)
        return bhr_fail(BHR_ERR_INVALID, "%s: spin %g with anti_alias = 1: ray differentials around a spinning hole need Kerr's variational equations", who, spin);
    if (ctx->disk_source != BHR_DISK_TEXTURE)
        return bhr_fail(BHR_ERR_INVALID, "%s: spin %g with a Disk V2 source (%d): the Kerr march shades the disk texture", who, spin, ctx->disk_source);
    if (ctx->ada_k > 1)
        return bhr_fail(BHR_ERR_INVALID, "%s: spin %g with adaptive supersampling (factor %d): the Kerr march has no refinement kernels; use bhr_set_supersample", who, spin, ctx->ada_k);
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "%s: spin %g on a row-block context (rows %d of %d): group and tile renders march Schwarzschild rays", who, spin, ctx->rows, ctx->cfg.height);
    if (flags & BHR_PERSISTENT)
        return bhr_fail(BHR_ERR_INVALID, "%s: spin %g with BHR_PERSISTENT: the Kerr march has the tile schedule only", who, spin);
    if (flags & BHR_ROW_COSTS)
        return bhr_fail(BHR_ERR_INVALID, "%s: spin %g with BHR_ROW_COSTS: the Kerr march fills no row-cost profile", who, spin);
    return BHR_OK;
}

// {VGPRs, LDS bytes, scratch bytes per lane} of a march kernel of the Kerr object, or of the observer object (ss: its supersampled
// twin).  No context: host + hipFuncGetAttributes.
int32_t kerr_kernel_resources(const char *who, bhr_march_kernel k, int32_t ss, int32_t out[3], int observer = 0) {
    if (!out) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    const void *f = observer == 3 ? bhr_march_kernel_delay(k, 0, ss ? 1 : 0)       // 3: the delay object
                    : observer == 2 ? bhr_march_kernel_projected(k, 0, ss ? 1 : 0)   // 1: the observer object, 2: the projected object
                    : observer  ? bhr_march_kernel_observer(k, 0, ss ? 1 : 0) : bhr_march_kernel_kerr(k, 0, ss ? 1 : 0);
    if (!f) return bhr_fail(BHR_ERR_STATE, "%s: no such march kernel in this library", who);
    hipFuncAttributes at;
    BHR_HIP(hipFuncGetAttributes(&at, f));
    out[0] = at.numRegs;
    out[1] = (int32_t)at.sharedSizeBytes;
    out[2] = (int32_t)at.localSizeBytes;
    return BHR_OK;
}

// Both supersampling settings: `ss` rays per pixel everywhere (ada_k = 0), or one ray per pixel and ada_k x ada_k where the
// neighbours differ by more than T.
int32_t set_sampling(bhr_ctx *ctx, const char *who, int32_t k, int32_t adaptive, float T) {
    if (k != 1 && k != 2 && k != 4 && k != 8) return bhr_fail(BHR_ERR_INVALID, "%s: factor %d (1, 2, 4 or 8)", who, k);
    if (k > 1 && ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "%s: a row-block context (rows %d of %d) renders one sample per pixel", who, ctx->rows, ctx->cfg.height);
    if ((int64_t)k * k * ctx->cfg.width * ctx->cfg.height >= ((int64_t)1 << 31))
        return bhr_fail(BHR_ERR_INVALID, "%s: %d x %d rays of a %dx%d frame exceed 2^31", who, k, k, ctx->cfg.width, ctx->cfg.height);
    const int32_t ss = adaptive ? 1 : k, ada_k = adaptive && k > 1 ? k : 0;
    if (ss == ctx->ss && ada_k == ctx->ada_k && (ada_k == 0 || memcmp(&T, &ctx->ada_threshold, sizeof(T)) == 0)) return BHR_OK;
    // the tile order, the hybrid lists and the fix lists belong to the marched frame: the frames in flight still march over them
    BHR_TRY(bhr_enter(ctx));
    for (auto &f : ctx->slots) {
        if (f.stream) BHR_HIP(hipStreamSynchronize(f.stream));
        if (f.aux_stream) BHR_HIP(hipStreamSynchronize(f.aux_stream));
    }
    BHR_HIP(hipStreamSynchronize(ctx->scene_stream));
    bhr_hybrid_free(ctx);
    if (ctx->d_tile_order) BHR_HIP(hipFree(ctx->d_tile_order));
    ctx->d_tile_order = nullptr;
    ctx->tile_order_n = 0;
    ctx->ss = ss;
    ctx->ada_k = ada_k;
    ctx->ada_threshold = ada_k ? T : 0.0f;
    ctx->ada_info_slot = -1;          // no adaptive frame under the new setting yet: bhr_adaptive_info and the counters' refinement rays
    return BHR_OK;
}

}  // namespace

// ---- the spinning hole (bhr_set_spin; csrc/ray_kerr.h, march_kerr.hip) ----------------------------------------------------------
// What has no Kerr form in this version; every refusal names the combination.
int32_t bhr_kerr_refuse(const bhr_ctx *ctx, const char *who, const char *what) {
    if (!ctx || !ctx->kerr_on) return BHR_OK;
    return bhr_fail(BHR_ERR_INVALID, "%s: a spin is set (bhr_set_spin, a / M = %g) and %s", who, (double)ctx->kerr_spin, what);
}

int32_t bhr_kerr_check(const bhr_ctx *ctx, uint32_t flags, const char *who) {
    if (!ctx || !ctx->kerr_on) return BHR_OK;
    return kerr_state_check(ctx, flags, who, (double)ctx->kerr_spin);
}

// The camera of a Kerr frame stands outside the static limit f = r / S = 1 (and so outside the horizon): the photon that
// leaves it along a pixel direction d has p = s d + f Lam l with s = 1 / sqrt(1 - f (1 - (l.d)^2)) and Lam = (1 + s l.d) / (1 - f)
// (ray_kerr.h: Ray::init), real for every d only where f < 1, and the exact redshift's observer is static.  Evaluated in
// binary64 on the Kerr-Schild radius of the position; refused before anything is launched.
int32_t bhr_kerr_camera_check(const bhr_ctx *ctx, const bhr_camera *cam, const char *who) {
    if (!ctx || !ctx->kerr_on) return BHR_OK;
    const double A = (double)ctx->kerr_spin, a2 = 0.25 * A * A;
    const double x = cam->pos[0], y = cam->pos[1], z = cam->pos[2];
    const double w = (x * x + y * y + z * z) - a2;
    const double S = sqrt(w * w + 4.0 * a2 * z * z);
    const double r = sqrt(0.5 * (w + S)), r_plus = 0.5 * (1.0 + sqrt(1.0 - A * A));
    const double f = S > 0.0 ? r / S : INFINITY;
    if (!(f < 1.0 && r >= r_plus))
        return bhr_fail(BHR_ERR_INVALID, "%s: the camera at (%g, %g, %g) lies inside the static limit of the hole of spin %g (f = r / S = %g with the Kerr-Schild radius r = %g; "
                        "f < 1 is needed, and r >= r_plus = %g): no photon leaves it along every pixel direction", who, x, y, z, A, f, r, r_plus);
    return BHR_OK;
}

extern "C" {

int32_t bhr_set_spin(bhr_ctx *ctx, float a_over_m, int32_t force_kerr) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_set_spin: null ctx");
    if (!(fabsf(a_over_m) <= 0.998f)) return bhr_fail(BHR_ERR_INVALID, "bhr_set_spin: spin a / M = %g (|a / M| <= 0.998)", (double)a_over_m);
    const int32_t on = (a_over_m != 0.0f || force_kerr) ? 1 : 0;
    if (on) BHR_TRY(kerr_state_check(ctx, 0, "bhr_set_spin", (double)a_over_m));
    if (!on && ctx->kerr_redshift == BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_spin: spin 0 without force_kerr while the exact redshift is set (bhr_set_redshift): it is a Kerr kernel's; set BHR_REDSHIFT_MODEL first");
    if (on == ctx->kerr_on && a_over_m == ctx->kerr_spin) return BHR_OK;
    BHR_TRY(bhr_enter(ctx));            // behind the frames in flight, like every other change of what a frame is
    ctx->kerr_on = on;
    ctx->kerr_spin = on ? a_over_m : 0.0f;
    // the counters name the kernel that marches a frame
    int32_t v = 0, l = 0;
    BHR_TRY(bhr_march_resources(on ? (ctx->kerr_redshift == BHR_REDSHIFT_EXACT ? -2 : -1) : ctx->cfg.math_mode, on ? 0 : ctx->cfg.anti_alias, &v, &l));
    ctx->counters.march_vgprs = v;
    ctx->counters.march_lds_bytes = l;
    return BHR_OK;
}

int32_t bhr_set_redshift(bhr_ctx *ctx, int32_t mode) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_set_redshift: null ctx");
    if (mode != BHR_REDSHIFT_MODEL && mode != BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_redshift: unknown mode %d (BHR_REDSHIFT_MODEL = 0, BHR_REDSHIFT_EXACT = 1)", mode);
    if (mode == BHR_REDSHIFT_EXACT && !ctx->kerr_on)
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_redshift: the exact redshift without the Kerr march: set a spin, or force_kerr at spin 0, first (bhr_set_spin)");
    if (mode == ctx->kerr_redshift) return BHR_OK;
    BHR_TRY(bhr_enter(ctx));            // behind the frames in flight
    ctx->kerr_redshift = mode;
    if (ctx->kerr_on) {                 // the counters name the kernel that marches a frame
        int32_t v = 0, l = 0;
        BHR_TRY(bhr_march_resources(mode == BHR_REDSHIFT_EXACT ? -2 : -1, 0, &v, &l));
        ctx->counters.march_vgprs = v;
        ctx->counters.march_lds_bytes = l;
    }
    return BHR_OK;
}

int32_t bhr_observer_resources(int32_t ss, int32_t out[3]) { return kerr_kernel_resources("bhr_observer_resources", BHR_MK_TILE, ss, out, 1); }
int32_t bhr_projected_resources(int32_t ss, int32_t out[3]) { return kerr_kernel_resources("bhr_projected_resources", BHR_MK_TILE, ss, out, 2); }
int32_t bhr_delayed_resources(int32_t ss, int32_t out[3]) { return kerr_kernel_resources("bhr_delayed_resources", BHR_MK_TILE, ss, out, 3); }

int32_t bhr_kerr_resources(int32_t ss, int32_t out[3]) { return kerr_kernel_resources("bhr_kerr_resources", BHR_MK_TILE, ss, out); }
// ... of the kernels of a redshift mode (bhr_set_redshift)
int32_t bhr_kerr_redshift_resources(int32_t mode, int32_t ss, int32_t out[3]) {
    if (mode != BHR_REDSHIFT_MODEL && mode != BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_redshift_resources: unknown mode %d (BHR_REDSHIFT_MODEL = 0, BHR_REDSHIFT_EXACT = 1)", mode);
    return kerr_kernel_resources("bhr_kerr_redshift_resources", mode == BHR_REDSHIFT_EXACT ? BHR_MK_KERR_EXACT : BHR_MK_TILE, ss, out);
}

int32_t bhr_set_supersample(bhr_ctx *ctx, int32_t k) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_set_supersample: null ctx");
    return set_sampling(ctx, "bhr_set_supersample", k, 0, 0.0f);
}

int32_t bhr_set_adaptive_supersample(bhr_ctx *ctx, int32_t k, float threshold) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_set_adaptive_supersample: null ctx");
    if (threshold != threshold) return bhr_fail(BHR_ERR_INVALID, "bhr_set_adaptive_supersample: the threshold is NaN");
    return set_sampling(ctx, "bhr_set_adaptive_supersample", k, 1, threshold);
}

}  // extern "C"
