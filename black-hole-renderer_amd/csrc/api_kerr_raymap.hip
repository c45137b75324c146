// api_kerr_raymap.hip -- the Kerr ray map's entry points (include/bhr.h): build, read, info, free, and the refusals of
// bhr_kerr_raymap_render and bhr_kerr_raymap_render_view (the frames themselves are launched from render.hip, next to
// bhr_raymap_render: they take a frame slot like any other).  The map is a bhr_raymap object of its own, ctx->kerr_raymap, made
// of api_raymap.hip's planes; nothing of the Schwarzschild map's state is shared or touched.
// The kernels are march_kerr_raymap.hip's, their launchers march_launch.hip's.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "bhr_internal.h"

namespace {

// every stream that may still read the map
int32_t drain(bhr_ctx *ctx) {
    for (auto &f : ctx->slots) {
        if (f.stream) BHR_HIP(hipStreamSynchronize(f.stream));
        if (f.aux_stream) BHR_HIP(hipStreamSynchronize(f.aux_stream));
    }
    BHR_HIP(hipStreamSynchronize(ctx->scene_stream));
    return BHR_OK;
}

int32_t fetch(bhr_ctx *ctx, void *dst, const void *d_src, size_t bytes) {
    BHR_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    return BHR_OK;
}

const char *redshift_name(int32_t mode) { return mode == BHR_REDSHIFT_EXACT ? "exact" : "model"; }

// What the Kerr march refuses of a context (tilt, anti-aliasing, Disk V2, adaptive supersampling, row blocks), and supersampling:
// the map holds one Kerr ray per pixel.
int32_t check_context(const bhr_ctx *ctx, const char *who) {
    BHR_TRY(bhr_variant_frame_check(ctx, bhr_variant_of(ctx), 0, who, (double)ctx->kerr_spin));
    if (ctx->ss > 1) return bhr_fail(BHR_ERR_INVALID, "%s: supersampling is on (factor %d); a Kerr ray map holds one ray per pixel", who, ctx->ss);
    return BHR_OK;
}

}  // namespace

void bhr_kerr_raymap_release(bhr_ctx *ctx) {
    if (!ctx->kerr_raymap) return;
    bhr_raymap_free_planes(ctx->kerr_raymap);
    delete ctx->kerr_raymap;
    ctx->kerr_raymap = nullptr;
}

// cam null: bhr_kerr_raymap_render (the build camera, no turn); else bhr_kerr_raymap_render_view, whose camera has to be the
// build's turned rigidly about z.
int32_t bhr_kerr_raymap_check_render(bhr_ctx *ctx, const char *who, const bhr_camera *cam, float t_offset, uint32_t flags, float *rot_c, float *rot_s) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "%s: null ctx", who);
    if (flags & ~(uint32_t)(BHR_SKIP_BLOOM | BHR_LENS_FLARE))
        return bhr_fail(BHR_ERR_INVALID, "%s: flags %u (BHR_SKIP_BLOOM and BHR_LENS_FLARE only)", who, flags);
    if (!isfinite(t_offset)) return bhr_fail(BHR_ERR_INVALID, "%s: t_offset is not finite", who);
    const bhr_raymap *rm = ctx->kerr_raymap;
    if (!rm || !rm->built) return bhr_fail(BHR_ERR_STATE, "%s: no Kerr ray map has been built (bhr_kerr_raymap_build)", who);
    // a Kerr ray's path depends on the spin, a record's meaning on the redshift mode (to_cam or the photon's momentum)
    if (!ctx->kerr_on || ctx->kerr_spin != ctx->kerr_map_spin || ctx->kerr_redshift != ctx->kerr_map_redshift)
        return bhr_fail(BHR_ERR_STATE, "%s: the map was built for spin %g with the %s redshift, the context now has %s %g with the %s redshift; build it again (bhr_kerr_raymap_build)",
                        who, (double)ctx->kerr_map_spin, redshift_name(ctx->kerr_map_redshift), ctx->kerr_on ? "spin" : "no Kerr march, spin",
                        (double)ctx->kerr_spin, redshift_name(ctx->kerr_redshift));
    BHR_TRY(check_context(ctx, who));
    if (cam) BHR_TRY(bhr_raymap_turn_of_build(rm->cam, cam, who, rot_c, rot_s));
    return BHR_OK;
}

extern "C" {

int32_t bhr_kerr_raymap_build(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags) {
    const char *who = "bhr_kerr_raymap_build";
    if (!ctx || !cam) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    if (ctx->rows != ctx->cfg.height)      // (such a context takes no spin either: said first, as what it is)
        return bhr_fail(BHR_ERR_INVALID, "%s: needs a whole-frame context (rows %d of %d)", who, ctx->rows, ctx->cfg.height);
    if (!ctx->kerr_on)
        return bhr_fail(BHR_ERR_STATE, "%s: no spin is set and the Kerr march is not forced (bhr_set_spin, bhr_set_redshift); bhr_raymap_build is the ray map of a hole that does not spin", who);
    if (flags) return bhr_fail(BHR_ERR_INVALID, "%s: flags %u (none are defined)", who, flags);
    BHR_TRY(check_context(ctx, who));
    const int32_t K = ctx->opt.raymap_slots;
    if (K < 1 || K > 8) return bhr_fail(BHR_ERR_INVALID, "%s: raymap_slots %d (1 .. 8)", who, K);
    if (ctx->opt.raymap_ss != 1)
        return bhr_fail(BHR_ERR_INVALID, "%s: raymap_supersample %d; a Kerr ray map has no supersampled form (1 only)", who, ctx->opt.raymap_ss);
    BHR_TRY(bhr_kerr_camera_check(ctx, cam, who));
    const int32_t comps = 5;
    const size_t plane = (size_t)ctx->rows * ctx->cfg.width;

    BHR_TRY(bhr_enter(ctx));           // behind the frames in flight: they may be reading the map this build rewrites
    if (!ctx->kerr_raymap) {
        ctx->kerr_raymap = new bhr_raymap();
        memset(ctx->kerr_raymap, 0, sizeof(bhr_raymap));
    }
    bhr_raymap *rm = ctx->kerr_raymap;
    rm->built = 0;
    if (rm->a.hits && rm->alloc_slots != K) {
        BHR_TRY(drain(ctx));
        bhr_raymap_free_planes(rm);
    }
    if (!rm->a.hits) BHR_TRY(bhr_raymap_alloc_planes(rm, who, K, comps, plane, 1));
    const BhrRayMapArgs &a = rm->a;
    // records beyond a pixel's crossings stay zero
    BHR_HIP(hipMemsetAsync(a.hits, 0, (size_t)K * comps * plane * sizeof(float), ctx->stream));
    BHR_HIP(hipMemsetAsync(a.over_count, 0, 16 * sizeof(unsigned int), ctx->stream));
    BHR_HIP(hipMemsetAsync(a.stats, 0, (8 + BHR_STEP_CELL) * sizeof(unsigned long long), ctx->stream));
    BHR_TRY(bhr_launch_kerr_raymap_build(ctx, cam, bhr_variant_of(ctx), a));
    std::vector<unsigned long long> stats(8 + BHR_STEP_CELL);
    unsigned int over = 0;
    BHR_TRY(fetch(ctx, stats.data(), a.stats, stats.size() * sizeof(unsigned long long)));
    BHR_TRY(fetch(ctx, &over, a.over_count, sizeof(over)));
    unsigned long long steps = 0;
    for (int k = 0; k < BHR_STEP_LANES; ++k) steps += stats[8 + (size_t)k * BHR_STEP_STRIDE];
    rm->ray_steps = steps;
    rm->crossings_stored = stats[0];
    rm->overflow_pixels = over;
    rm->diff = 0;
    rm->slots = K;
    rm->ss = 1;
    rm->cam = *cam;
    ctx->kerr_map_spin = ctx->kerr_spin;
    ctx->kerr_map_redshift = ctx->kerr_redshift;
    rm->built = 1;
    return BHR_OK;
}

int32_t bhr_kerr_raymap_read(bhr_ctx *ctx, int32_t which, void *out, int64_t bytes) {
    const char *who = "bhr_kerr_raymap_read";
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "%s: bad argument", who);
    if (!ctx->kerr_raymap || !ctx->kerr_raymap->built) return bhr_fail(BHR_ERR_STATE, "%s: no Kerr ray map has been built (bhr_kerr_raymap_build)", who);
    const BhrRayMapArgs &a = ctx->kerr_raymap->a;
    const size_t plane = (size_t)a.plane;
    size_t want = 0;
    switch (which) {
    case BHR_RAYMAP_STEPS: case BHR_RAYMAP_STATUS: case BHR_RAYMAP_CROSSINGS: want = plane * 4; break;
    case BHR_RAYMAP_ESCAPE_DIR: want = plane * 12; break;
    case BHR_RAYMAP_HITS: want = (size_t)a.slots * a.comps * plane * 4; break;
    default: return bhr_fail(BHR_ERR_INVALID, "%s: unknown plane %d", who, which);
    }
    if (bytes != (int64_t)want) return bhr_fail(BHR_ERR_INVALID, "%s: plane %d has %zu bytes, caller gave %lld", who, which, want, (long long)bytes);
    BHR_TRY(bhr_enter(ctx));
    if (which == BHR_RAYMAP_STEPS) return fetch(ctx, out, a.steps, want);
    if (which == BHR_RAYMAP_STATUS) return fetch(ctx, out, a.status, want);
    if (which == BHR_RAYMAP_CROSSINGS) return fetch(ctx, out, a.crossings, want);
    // the device planes are [component][pixel]; the caller gets [pixel][component]
    const int nc = which == BHR_RAYMAP_ESCAPE_DIR ? 3 : a.comps, ns = which == BHR_RAYMAP_ESCAPE_DIR ? 1 : a.slots;
    std::vector<float> tmp((size_t)nc * plane);
    float *o = (float *)out;
    for (int s = 0; s < ns; ++s) {
        const float *src = which == BHR_RAYMAP_ESCAPE_DIR ? a.dir : a.hits + (size_t)s * nc * plane;
        BHR_TRY(fetch(ctx, tmp.data(), src, tmp.size() * sizeof(float)));
        float *os = o + (size_t)s * plane * nc;
        for (int c = 0; c < nc; ++c)
            for (size_t p = 0; p < plane; ++p) os[p * nc + c] = tmp[(size_t)c * plane + p];
    }
    return BHR_OK;
}

int32_t bhr_kerr_raymap_info(bhr_ctx *ctx, bhr_kerr_raymap_desc *out) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_raymap_info: bad argument");
    memset(out, 0, sizeof(*out));
    const bhr_raymap *rm = ctx->kerr_raymap;
    if (!rm) return BHR_OK;
    out->built = rm->built;
    out->device_bytes = rm->device_bytes;
    if (!rm->built) return BHR_OK;
    out->slots = rm->slots;
    out->width = ctx->cfg.width;
    out->rows = ctx->rows;
    out->redshift = ctx->kerr_map_redshift;
    out->spin = ctx->kerr_map_spin;
    out->crossings_stored = (int64_t)rm->crossings_stored;
    out->overflow_pixels = (int64_t)rm->overflow_pixels;
    out->ray_steps = rm->ray_steps;
    out->cam = rm->cam;
    return BHR_OK;
}

int32_t bhr_kerr_raymap_free(bhr_ctx *ctx) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_raymap_free: null ctx");
    if (!ctx->kerr_raymap) return BHR_OK;
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(drain(ctx));               // the frames in flight read the map
    bhr_kerr_raymap_release(ctx);
    return BHR_OK;
}

}  // extern "C"
