// settings.hip -- what changes the kind of frame a context renders: the march variants' table with their refusals, the spinning
// hole, and the sampling.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "bhr_internal.h"

namespace {

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

// ---- the march variants (bhr_internal.h: bhr_march_variant) -----------------------------------------------------------------------
const bhr_variant_row &bhr_variant_row_of(bhr_march_variant v) {
    constexpr uint32_t kerr_flags = ~(uint32_t)(BHR_PERSISTENT | BHR_ROW_COSTS), rest_flags = BHR_SKIP_BLOOM | BHR_LENS_FLARE;
    constexpr const char *kerr_diff = "ray differentials around a spinning hole need Kerr's variational equations";
    constexpr const char *kerr_rows = "group and tile renders march Schwarzschild rays", *rest_rows = "needs a whole-frame context";
    constexpr const char *obs_diff = "the differential seeds under aberration are not implemented", *obs_exact = "its observer is static";
    // (a projection's frame is an observer's, at rest if need be, marched by the projected object: the observer's words)
    static const bhr_variant_row rows[BHR_MV_COUNT] = {
        {},                            // BHR_MV_NONE: the marches march_kernel picks by arithmetic, schedule and disk source
        {bhr_march_kernel_kerr, BHR_MK_TILE, "spin %g", "Kerr", kerr_diff, nullptr, kerr_rows, kerr_flags, true},
        {bhr_march_kernel_kerr, BHR_MK_KERR_EXACT, "spin %g", "Kerr", kerr_diff, nullptr, kerr_rows, kerr_flags, true},
        {bhr_march_kernel_observer, BHR_MK_TILE, "a moving observer", "observer", obs_diff, obs_exact, rest_rows, rest_flags, false},
        {bhr_march_kernel_projected, BHR_MK_TILE, "a projection", "observer", obs_diff, obs_exact, rest_rows, rest_flags, false},
        {bhr_march_kernel_delay, BHR_MK_TILE, "light delay", "delayed", "the delayed march has no ray differentials", "the delayed march is Schwarzschild's",
         rest_rows, rest_flags, false},
        // the Kerr camera (bhr_render_kerr_view): the Kerr rows' refusals with the observer's flags and whole-frame context
        {bhr_march_kernel_kerr_view, BHR_MK_TILE, "a Kerr view at spin %g", "Kerr", kerr_diff, nullptr, rest_rows, rest_flags, true},
        {bhr_march_kernel_kerr_view, BHR_MK_KERR_EXACT, "a Kerr view at spin %g", "Kerr", kerr_diff, nullptr, rest_rows, rest_flags, true},
    };
    return rows[v];
}

// The counters name the kernel that marches a frame: the context's variant's, else its arithmetic's.
int32_t bhr_note_frame_kernel(bhr_ctx *ctx) {
    int32_t res[3];
    const bhr_march_variant v = bhr_variant_of(ctx);
    if ((v == BHR_MV_KERR || v == BHR_MV_KERR_EXACT) && ctx->kerr_disk_source != BHR_DISK_TEXTURE)
        BHR_TRY(bhr_kerr_disk_resources(ctx->kerr_disk_source, ctx->kerr_redshift, 0, res));       // the Kerr march's own Disk V2 source: march_kerr_dv2.o's
    else
        BHR_TRY(bhr_march_resources("bhr_note_frame_kernel", v, ctx->cfg.math_mode, bhr_want_diff(ctx, 0, v), 0, res));
    ctx->counters.march_vgprs = res[0];
    ctx->counters.march_lds_bytes = res[1];
    return BHR_OK;
}

bhr_march_variant bhr_variant_of(const bhr_ctx *ctx, bhr_march_variant asked) {
    if (asked != BHR_MV_NONE || !ctx->kerr_on) return asked;
    return ctx->kerr_redshift == BHR_REDSHIFT_EXACT ? BHR_MV_KERR_EXACT : BHR_MV_KERR;
}

// The flags first, then the context's state; every refusal names the combination.
int32_t bhr_variant_frame_check(const bhr_ctx *ctx, bhr_march_variant v, uint32_t flags, const char *who, double spin) {
    if (v == BHR_MV_NONE) return BHR_OK;
    const bhr_variant_row &r = bhr_variant_row_of(v);
    char what[48];
    snprintf(what, sizeof(what), r.noun, spin);
    if (const uint32_t bad = flags & ~r.flags_ok) {
        // (the rows that take the two post-pass flags only say so; the Kerr march's own rows take all but the two they name)
        if ((r.flags_ok | BHR_PERSISTENT | BHR_ROW_COSTS) != ~(uint32_t)0) return bhr_fail(BHR_ERR_INVALID, "%s: %s with flags %u (BHR_SKIP_BLOOM and BHR_LENS_FLARE only)", who, what, flags);
        return bhr_fail(BHR_ERR_INVALID, "%s: %s with %s", who, what,
                        (bad & BHR_PERSISTENT) ? "BHR_PERSISTENT: the Kerr march has the tile schedule only" : "BHR_ROW_COSTS: the Kerr march fills no row-cost profile");
    }
    if (r.kerr && ctx->cfg.disk_tilt_deg != 0.0f)
        return bhr_fail(BHR_ERR_INVALID, "%s: %s with a disk tilted by %g degrees: the spin axis is the disk normal, tilt must be 0", who, what, (double)ctx->cfg.disk_tilt_deg);
    if (ctx->cfg.anti_alias != 0) return bhr_fail(BHR_ERR_INVALID, "%s: %s with anti_alias = 1: %s", who, what, r.no_diff);
    if (ctx->disk_source != BHR_DISK_TEXTURE)
        return bhr_fail(BHR_ERR_INVALID, "%s: %s with a Disk V2 source (%d): the %s march shades the disk texture", who, what, ctx->disk_source, r.march);
    if (ctx->ada_k > 1)
        return bhr_fail(BHR_ERR_INVALID, "%s: %s with adaptive supersampling (factor %d): the %s march has no refinement kernels; use bhr_set_supersample", who, what, ctx->ada_k, r.march);
    if (!r.kerr && ctx->kerr_on && ctx->kerr_redshift == BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "%s: %s with the exact redshift (bhr_set_redshift): %s", who, what, r.no_exact);
    if (!r.kerr && ctx->kerr_on)
        return bhr_fail(BHR_ERR_INVALID, "%s: %s with a spin set or the Kerr march forced (bhr_set_spin, a / M = %g): the %s march is Schwarzschild's", who, what, spin, r.march);
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "%s: %s on a row-block context (rows %d of %d): %s", who, what, ctx->rows, ctx->cfg.height, r.no_rows);
    return BHR_OK;
}

// ---- the spinning hole (bhr_set_spin; csrc/ray_kerr.h, march_kerr.hip) ----------------------------------------------------------
// A call that has no Kerr form at all in this version; the refusal names the combination.
int32_t bhr_kerr_refuse(const bhr_ctx *ctx, const char *who, const char *what) {
    if (!ctx || !ctx->kerr_on) return BHR_OK;
    return bhr_fail(BHR_ERR_INVALID, "%s: a spin is set (bhr_set_spin, a / M = %g) and %s", who, (double)ctx->kerr_spin, what);
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

// A call that has no form over the Kerr march's own Disk V2 source; the refusal names the combination.
int32_t bhr_kerr_disk_refuse(const bhr_ctx *ctx, const char *who, const char *what) {
    if (!ctx || ctx->kerr_disk_source == BHR_DISK_TEXTURE) return BHR_OK;
    return bhr_fail(BHR_ERR_INVALID, "%s: a Kerr Disk V2 source is set (bhr_set_kerr_disk_source, %d) and %s; set BHR_DISK_TEXTURE first", who, ctx->kerr_disk_source, what);
}

extern "C" {

int32_t bhr_set_spin(bhr_ctx *ctx, float a_over_m, int32_t force_kerr) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_set_spin: null ctx");
    if (!(fabsf(a_over_m) <= 0.998f)) return bhr_fail(BHR_ERR_INVALID, "bhr_set_spin: spin a / M = %g (|a / M| <= 0.998)", (double)a_over_m);
    const int32_t on = (a_over_m != 0.0f || force_kerr) ? 1 : 0;
    if (on) BHR_TRY(bhr_variant_frame_check(ctx, BHR_MV_KERR, 0, "bhr_set_spin", (double)a_over_m));
    if (!on && ctx->kerr_redshift == BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_spin: spin 0 without force_kerr while the exact redshift is set (bhr_set_redshift): it is a Kerr kernel's; set BHR_REDSHIFT_MODEL first");
    if (!on && ctx->kerr_aa)
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_spin: spin 0 without force_kerr while the Kerr anti-aliasing is on (bhr_set_kerr_anti_alias): it is a Kerr kernel's; switch it off first");
    if (!on && ctx->kerr_disk_source != BHR_DISK_TEXTURE)
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_spin: spin 0 without force_kerr while a Kerr Disk V2 source is set (bhr_set_kerr_disk_source): it is a Kerr kernel's; set BHR_DISK_TEXTURE first");
    if (on == ctx->kerr_on && a_over_m == ctx->kerr_spin) return BHR_OK;
    BHR_TRY(bhr_enter(ctx));            // behind the frames in flight, like every other change of what a frame is
    ctx->kerr_on = on;
    ctx->kerr_spin = on ? a_over_m : 0.0f;
    if (bhr_have_kerr_polar(ctx)) bhr_polar_invalidate(ctx);   // the Stokes planes of a Kerr map frame are that spin's
    if (bhr_have_kerr_line(ctx)) bhr_kerr_line_invalidate(ctx);   // ... and the line's sample planes
    return bhr_note_frame_kernel(ctx);
}

int32_t bhr_set_redshift(bhr_ctx *ctx, int32_t mode) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_set_redshift: null ctx");
    if (mode != BHR_REDSHIFT_MODEL && mode != BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_redshift: unknown mode %d (BHR_REDSHIFT_MODEL = 0, BHR_REDSHIFT_EXACT = 1)", mode);
    if (mode == BHR_REDSHIFT_EXACT && !ctx->kerr_on)
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_redshift: the exact redshift without the Kerr march: set a spin, or force_kerr at spin 0, first (bhr_set_spin)");
    if (mode == BHR_REDSHIFT_EXACT && ctx->kerr_disk_source == BHR_DISK_V2_VOLUME)
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_redshift: the exact redshift with the Disk V2 volume (bhr_set_kerr_disk_source): gas off the equatorial plane has no four-velocity in this model; "
                        "set the surface source (BHR_DISK_V2) or BHR_DISK_TEXTURE first");
    if (mode == ctx->kerr_redshift) return BHR_OK;
    BHR_TRY(bhr_enter(ctx));            // behind the frames in flight
    ctx->kerr_redshift = mode;
    if (bhr_have_kerr_polar(ctx)) bhr_polar_invalidate(ctx);   // ... and that mode's gas
    if (bhr_have_kerr_line(ctx)) bhr_kerr_line_invalidate(ctx);
    return bhr_note_frame_kernel(ctx);
}

int32_t bhr_set_kerr_anti_alias(bhr_ctx *ctx, int32_t on, float strength) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_set_kerr_anti_alias: null ctx");
    if (!(strength >= 0.0f) || !isfinite(strength))
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_kerr_anti_alias: strength %g (finite and not negative)", (double)strength);
    if (on && !ctx->kerr_on)
        return bhr_fail(BHR_ERR_STATE, "bhr_set_kerr_anti_alias: Kerr anti-aliasing without the Kerr march: set a spin, or force_kerr at spin 0, first (bhr_set_spin)");
    if (on) BHR_TRY(bhr_kerr_disk_refuse(ctx, "bhr_set_kerr_anti_alias", "the analytic source has no mip chain for the Kerr anti-aliasing"));
    const int32_t aa = on ? 1 : 0;
    if (aa == ctx->kerr_aa && (!aa || strength == ctx->kerr_aa_strength)) return BHR_OK;
    BHR_TRY(bhr_enter(ctx));            // behind the frames in flight
    ctx->kerr_aa = aa;
    ctx->kerr_aa_strength = aa ? strength : 0.0f;
    return bhr_note_frame_kernel(ctx);
}

int32_t bhr_kerr_anti_alias_resources(int32_t mode, int32_t ss, int32_t out[3]) {
    if (mode != BHR_REDSHIFT_MODEL && mode != BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_anti_alias_resources: unknown mode %d (BHR_REDSHIFT_MODEL = 0, BHR_REDSHIFT_EXACT = 1)", mode);
    return bhr_march_resources("bhr_kerr_anti_alias_resources", mode == BHR_REDSHIFT_EXACT ? BHR_MV_KERR_EXACT : BHR_MV_KERR, 0, 1, ss, out);
}

int32_t bhr_observer_resources(int32_t ss, int32_t out[3]) { return bhr_march_resources("bhr_observer_resources", BHR_MV_OBSERVER, 0, 0, ss, out); }
int32_t bhr_projected_resources(int32_t ss, int32_t out[3]) { return bhr_march_resources("bhr_projected_resources", BHR_MV_PROJECTED, 0, 0, ss, out); }
int32_t bhr_delayed_resources(int32_t ss, int32_t out[3]) { return bhr_march_resources("bhr_delayed_resources", BHR_MV_DELAYED, 0, 0, ss, out); }

int32_t bhr_kerr_resources(int32_t ss, int32_t out[3]) { return bhr_march_resources("bhr_kerr_resources", BHR_MV_KERR, 0, 0, ss, out); }
// ... of the kernels of a redshift mode (bhr_set_redshift)
int32_t bhr_kerr_redshift_resources(int32_t mode, int32_t ss, int32_t out[3]) {
    if (mode != BHR_REDSHIFT_MODEL && mode != BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_redshift_resources: unknown mode %d (BHR_REDSHIFT_MODEL = 0, BHR_REDSHIFT_EXACT = 1)", mode);
    return bhr_march_resources("bhr_kerr_redshift_resources", mode == BHR_REDSHIFT_EXACT ? BHR_MV_KERR_EXACT : BHR_MV_KERR, 0, 0, ss, out);
}

// ... of the Kerr camera's kernels (bhr_render_kerr_view), by redshift mode
int32_t bhr_kerr_view_resources(int32_t mode, int32_t ss, int32_t out[3]) {
    if (mode != BHR_REDSHIFT_MODEL && mode != BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_view_resources: unknown mode %d (BHR_REDSHIFT_MODEL = 0, BHR_REDSHIFT_EXACT = 1)", mode);
    return bhr_march_resources("bhr_kerr_view_resources", mode == BHR_REDSHIFT_EXACT ? BHR_MV_KERR_VIEW_EXACT : BHR_MV_KERR_VIEW, 0, 0, ss, out);
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
