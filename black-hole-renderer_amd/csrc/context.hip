// context.hip -- the context itself: error plumbing, the options, create / destroy / sync, and the host <-> device copies.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <string>

#include "bhr_internal.h"

namespace {

thread_local char g_err[512] = "";

// the environment, once (bhr_create): nothing on the bhr_render path calls getenv
void read_options(bhr_options *o) {
    memset(o, 0, sizeof(*o));
    auto num = [](const char *name, int dflt) { const char *e = getenv(name); return e && e[0] ? atoi(e) : dflt; };
    o->frame_slots = num("BHR_FRAME_SLOTS", 2);
    if (o->frame_slots < 1 || o->frame_slots > BHR_MAX_FRAME_SLOTS) o->frame_slots = 2;
    o->bloom_split = num("BHR_BLOOM_SPLIT", -1);
    if (o->bloom_split > 1) o->bloom_split = 1;
    o->bloom_tiles = num("BHR_BLOOM_TILES", 0);
    if (o->bloom_tiles < 0 || o->bloom_tiles > 8) o->bloom_tiles = 0;
    o->hybrid_repair = num("BHR_HYBRID_REPAIR", -1);
    if (o->hybrid_repair > 1) o->hybrid_repair = 1;
    o->hybrid_band_set = 0;
    if (const char *e = getenv("BHR_HYBRID_BAND")) {
        double lo = 0, hi = 0;
        if (sscanf(e, "%lf,%lf", &lo, &hi) == 2 && lo >= 0 && hi >= 0) { o->hybrid_band[0] = lo; o->hybrid_band[1] = hi; o->hybrid_band_set = 1; }
    }
    // share of its own span of b a SMALL tile is padded by in the strict-band test (hybrid.hip: tile_pad; tools/exp_hybrid_pad.py)
    o->hybrid_pad = 0.5;
    if (const char *e = getenv("BHR_HYBRID_PAD")) { const double v = atof(e); if (v >= 0.0 && v <= 4.0) o->hybrid_pad = v; }
    o->hybrid_streams = num("BHR_HYBRID_STREAMS", -1);
    if (o->hybrid_streams != 1 && o->hybrid_streams != 2) o->hybrid_streams = -1;
    o->calibrate_streams = num("BHR_CALIBRATE_STREAMS", 1) != 0;
    o->hybrid_classify = num("BHR_HYBRID_CLASSIFY", 1) != 0;
    o->mip_lds = num("BHR_MIP_LDS", 0) != 0;
    o->group_threads = num("BHR_GROUP_THREADS", -1);
    { const char *e = getenv("BHR_GROUP_SCHEDULE"); o->group_schedule = e && e[0] ? (e[0] == 's' ? 0 : 1) : -1; }
    o->png16_menu = num("BHR_PNG16_MENU", 1) != 0;
    o->shutter_timing = num("BHR_SHUTTER_TIMING", 0) != 0;
    o->raymap_shutter_fused = num("BHR_RAYMAP_SHUTTER_FUSED", 1) != 0;
    o->kerr_raymap_shutter_fused = num("BHR_KERR_RAYMAP_SHUTTER_FUSED", 1) != 0;
    o->grade_timing = num("BHR_GRADE_TIMING", 0) != 0;
    o->raymap_slots = num("BHR_RAYMAP_SLOTS", 4);        // outside 1 .. 8: bhr_raymap_build refuses
    o->raymap_ss = num("BHR_RAYMAP_SUPERSAMPLE", 1);     // not 1, 2, 4 or 8: bhr_raymap_build refuses
    o->kerr_raymap_ss = num("BHR_KERR_RAYMAP_SUPERSAMPLE", 1);   // not 1, 2, 4 or 8: bhr_kerr_raymap_build refuses
}

}  // namespace

int32_t bhr_fail(int32_t code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int32_t bhr_ensure_pinned(bhr_ctx *ctx, size_t bytes) {
    if (ctx->h_pinned_bytes >= bytes) return BHR_OK;
    if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
    ctx->h_pinned = nullptr;
    ctx->h_pinned_bytes = 0;
    BHR_HIP(hipHostMalloc((void **)&ctx->h_pinned, bytes, hipHostMallocDefault));
    ctx->h_pinned_bytes = bytes;
    return BHR_OK;
}

// device -> caller memory through the pinned staging buffer (synchronises the stream)
int32_t bhr_download(bhr_ctx *ctx, void *dst, const void *d_src, size_t bytes) {
    BHR_TRY(bhr_ensure_pinned(ctx, bytes));
    BHR_HIP(hipMemcpyAsync(ctx->h_pinned, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(dst, ctx->h_pinned, bytes);
    return BHR_OK;
}

int32_t bhr_upload(bhr_ctx *ctx, void *d_dst, const void *src, size_t bytes) {
    // pageable source: hipMemcpyAsync stages internally and is ordered on the stream
    BHR_HIP(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    return BHR_OK;
}

// Waits by POLLING an event for the first 200 ms, then blocks.  hipStreamSynchronize sleeps on an interrupt, and the wake-up is
// usually 0.1 ms after the GPU is done but every so often 2 ms and more (bench line of a 20-step run: the 20 frames' own event
// span 6.6 ms in both of two runs, the host back after 6.7 and after 8.7 ms -- a quarter of the frame rate of a run that short;
// profiles/r04e_sync_wakeup.txt).  A frame loop that waits once per batch can afford a core for its wait.
int32_t bhr_poll_sync(bhr_ctx *ctx, hipStream_t stream) {
    BHR_HIP(hipEventRecord(ctx->sync_ev, stream));
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ctx->sync_ev);
        if (e == hipSuccess) return BHR_OK;
        if (e != hipErrorNotReady) BHR_HIP(e);
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;
    }
    BHR_HIP(hipStreamSynchronize(stream));
    return BHR_OK;
}

extern "C" {

const char *bhr_last_error(void) { return g_err; }
int32_t bhr_abi_version(void) { return BHR_ABI_VERSION; }

int32_t bhr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int32_t bhr_create(const bhr_config *cfg, bhr_ctx **out) {
    if (!cfg || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_create: null argument");
    *out = nullptr;
    if (cfg->width <= 0 || cfg->height <= 0) return bhr_fail(BHR_ERR_INVALID, "bhr_create: bad image size %dx%d", cfg->width, cfg->height);
    if (cfg->row0 < 0 || cfg->row1 > cfg->height || cfg->row0 >= cfg->row1)
        return bhr_fail(BHR_ERR_INVALID, "bhr_create: bad row block [%d,%d) for height %d", cfg->row0, cfg->row1, cfg->height);
    if (!(cfg->step_size > 0.0f)) return bhr_fail(BHR_ERR_INVALID, "bhr_create: step_size must be positive");
    if (!(cfg->r_disk_inner < cfg->r_disk_outer)) return bhr_fail(BHR_ERR_INVALID, "bhr_create: r_disk_inner must be < r_disk_outer");
    int ndev = bhr_device_count();
    if (ndev <= 0) return bhr_fail(BHR_ERR_NO_DEVICE, "bhr_create: no HIP device visible (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return bhr_fail(BHR_ERR_NO_DEVICE, "bhr_create: device %d out of range (have %d)", cfg->device, ndev);

    bhr_ctx *ctx = new bhr_ctx();
    memset(ctx, 0, sizeof(*ctx));
    ctx->cfg = *cfg;
    ctx->rows = cfg->row1 - cfg->row0;
    ctx->bloom_R = (int32_t)(cfg->width * 0.02);  // int(self.width * 0.02), render.py:3914
    ctx->mip_lds_from = -1;
    ctx->ss = 1;
    ctx->ada_info_slot = -1;
    ctx->stokes_slot = -1;
    bhr_kerr_line_invalidate(ctx);

    auto bail = [&](int32_t rc) { bhr_destroy(ctx); return rc; };
    if (hipSetDevice(cfg->device) != hipSuccess) return bail(bhr_fail(BHR_ERR_HIP, "hipSetDevice(%d) failed", cfg->device));
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return bail(bhr_fail(BHR_ERR_HIP, "hipStreamCreate failed"));
    ctx->scene_stream = ctx->stream;
    read_options(&ctx->opt);
    ctx->n_slots = ctx->opt.frame_slots;                 // 2 (default): frames alternate between two slots / streams
    ctx->split_ok = bhr_split_nt(ctx->bloom_R) <= 12;    // the split-f16 bloom's table: radius <= 176 (widths to 8849)
    ctx->out_want = BHR_OUT_F32;
    if (hipEventCreateWithFlags(&ctx->scene_ev, hipEventDisableTiming) != hipSuccess) return bail(bhr_fail(BHR_ERR_HIP, "hipEventCreate failed"));
    if (hipEventCreateWithFlags(&ctx->sync_ev, hipEventDisableTiming) != hipSuccess) return bail(bhr_fail(BHR_ERR_HIP, "hipEventCreate failed"));
    for (auto &e : ctx->ev)
        if (hipEventCreate(&e) != hipSuccess) return bail(bhr_fail(BHR_ERR_HIP, "hipEventCreate failed"));
    for (auto &e : ctx->ring_ev)
        if (hipEventCreate(&e) != hipSuccess) return bail(bhr_fail(BHR_ERR_HIP, "hipEventCreate failed"));

    const size_t W = cfg->width, H = cfg->height, R = ctx->bloom_R;
    int32_t rc;
    if ((rc = bhr_activate_slot(ctx, 0))) return bail(rc);
    if ((rc = bhr_dev_alloc(&ctx->d_wtab, 3 * (R + 1 + 64)))) return bail(rc);
    if ((rc = bhr_dev_alloc(&ctx->d_wext, 3 * (2 * (R + 4) + 8)))) return bail(rc);
    if ((rc = bhr_dev_alloc(&ctx->d_wsum_h, 6 * W))) return bail(rc);
    if ((rc = bhr_dev_alloc(&ctx->d_wsum_v, 6 * H))) return bail(rc);
    if ((rc = bhr_dev_alloc(&ctx->d_ray_steps, BHR_STEP_CELL))) return bail(rc);
    if ((rc = bhr_dev_alloc(&ctx->d_steps_ring, (size_t)BHR_TIMING_RING * BHR_STEP_CELL))) return bail(rc);
    if ((rc = bhr_dev_alloc(&ctx->d_steps_fold, BHR_TIMING_RING))) return bail(rc);
    if (hipMemsetAsync(ctx->d_ray_steps, 0, sizeof(unsigned long long) * BHR_STEP_CELL, ctx->stream) != hipSuccess ||
        hipMemsetAsync(ctx->d_steps_ring, 0, sizeof(unsigned long long) * BHR_TIMING_RING * BHR_STEP_CELL, ctx->stream) != hipSuccess)
        return bail(bhr_fail(BHR_ERR_HIP, "hipMemsetAsync failed"));
    if (cfg->math_mode != BHR_MATH_FAST && cfg->math_mode != BHR_MATH_STRICT && cfg->math_mode != BHR_MATH_HYBRID)
        return bail(bhr_fail(BHR_ERR_INVALID, "bhr_create: math_mode %d", cfg->math_mode));
    (void)bhr_note_frame_kernel(ctx);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return bail(bhr_fail(BHR_ERR_HIP, "stream sync failed"));
    *out = ctx;
    return BHR_OK;
}

void bhr_destroy(bhr_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->cfg.device);
    for (auto &f : ctx->slots) {
        if (f.stream) (void)hipStreamSynchronize(f.stream);
        if (f.aux_stream) (void)hipStreamSynchronize(f.aux_stream);
    }
    if (ctx->scene_stream) (void)hipStreamSynchronize(ctx->scene_stream);
    ctx->stream = ctx->scene_stream;
    bhr_free_scene(ctx);
    bhr_free_bg(ctx);
    for (int k = 0; k < BHR_MAX_FRAME_SLOTS; ++k) bhr_free_slot(ctx, k);
    bhr_png_dev_free(ctx);
    bhr_jpeg_dev_free(ctx);
    bhr_shutter_free(ctx);
    bhr_grade_free(ctx);
    bhr_raymap_release(ctx, &ctx->raymap);
    bhr_raymap_release(ctx, &ctx->kerr_raymap);
    bhr_stars_release(ctx, BHR_RAYMAP_SCHWARZSCHILD);
    bhr_stars_release(ctx, BHR_RAYMAP_KERR);
    bhr_kerr_line_release(ctx);
    bhr_population_free(ctx);
    bhr_hybrid_free(ctx);
    bhr_pipe_free(ctx);
    for (int q = 0; q < ctx->n_calib_idle; ++q) (void)hipStreamDestroy(ctx->calib_idle[q]);
    ctx->n_calib_idle = 0;
    if (ctx->d_gather_u8) (void)hipFree(ctx->d_gather_u8);
    free(ctx->h_tile_order);
    if (ctx->scene_ev) (void)hipEventDestroy(ctx->scene_ev);
    if (ctx->sync_ev) (void)hipEventDestroy(ctx->sync_ev);
    void *bufs[] = {ctx->d_skybox,
                    ctx->d_wtab, ctx->d_wsum_h, ctx->d_wsum_v, ctx->d_ray_steps, ctx->d_noise_in,
                    ctx->d_noise_out, ctx->d_steps_ring, ctx->d_steps_fold, ctx->d_pool, ctx->d_pairs, ctx->d_stats_scratch, ctx->d_wext, ctx->d_w16, ctx->d_dv2_params, ctx->d_kerr_dv2_params,
                    ctx->d_flare_prog, ctx->d_tile_order, ctx->d_row_steps, ctx->d_gather, ctx->d_dither};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : ctx->ring_ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int32_t bhr_sync(bhr_ctx *ctx) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "null ctx");
    BHR_TRY(bhr_enter(ctx));
    return bhr_poll_sync(ctx, ctx->stream);
}

int32_t bhr_set_option(bhr_ctx *ctx, const char *name, double value) {
    if (!ctx || !name) return bhr_fail(BHR_ERR_INVALID, "bhr_set_option: bad argument");
    const std::string n(name);
    const int v = (int)value;
    bhr_options &o = ctx->opt;
    if (n == "bloom_split") o.bloom_split = v < 0 ? -1 : (v ? 1 : 0);
    else if (n == "bloom_tiles") o.bloom_tiles = v < 0 || v > 8 ? 0 : v;
    else if (n == "hybrid_repair") o.hybrid_repair = v < 0 ? -1 : (v ? 1 : 0);
    else if (n == "hybrid_band_lo") { if (!o.hybrid_band_set) o.hybrid_band[1] = 0.36; o.hybrid_band[0] = value; o.hybrid_band_set = 1; }
    else if (n == "hybrid_band_hi") { if (!o.hybrid_band_set) o.hybrid_band[0] = 0.085; o.hybrid_band[1] = value; o.hybrid_band_set = 1; }
    else if (n == "hybrid_band_default") o.hybrid_band_set = 0;
    else if (n == "hybrid_pad") { if (value >= 0.0 && value <= 4.0) o.hybrid_pad = value; }
    else if (n == "hybrid_streams") o.hybrid_streams = v == 1 ? 1 : (v == 2 ? 2 : -1);
    else if (n == "calibrate_streams") o.calibrate_streams = v != 0;
    else if (n == "hybrid_classify") o.hybrid_classify = v != 0;
    else if (n == "mip_lds") o.mip_lds = v != 0;
    else if (n == "group_threads") o.group_threads = v < 0 ? -1 : (v ? 1 : 0);
    else if (n == "group_schedule") o.group_schedule = v < 0 ? -1 : (v ? 1 : 0);
    else if (n == "shutter_timing") o.shutter_timing = v != 0;
    else if (n == "raymap_shutter_fused") o.raymap_shutter_fused = v != 0;
    else if (n == "kerr_raymap_shutter_fused") o.kerr_raymap_shutter_fused = v != 0;
    else if (n == "grade_timing") o.grade_timing = v != 0;
    else if (n == "raymap_slots") {   // read by the next bhr_raymap_build; the map in memory keeps its own
        if (!(value >= 1.0 && value <= 8.0)) return bhr_fail(BHR_ERR_INVALID, "bhr_set_option: raymap_slots %g (1 .. 8)", value);
        o.raymap_slots = v;
    }
    else if (n == "raymap_supersample") {   // the next map's own factor; the context's bhr_set_supersample stays at 1 for every map call
        if (!(value == 1.0 || value == 2.0 || value == 4.0 || value == 8.0))
            return bhr_fail(BHR_ERR_INVALID, "bhr_set_option: raymap_supersample %g (1, 2, 4 or 8)", value);
        o.raymap_ss = v;
    }
    else if (n == "kerr_raymap_supersample") {   // the next Kerr map's own factor, a name of its own: "raymap_supersample" stays the Schwarzschild map's
        if (!(value == 1.0 || value == 2.0 || value == 4.0 || value == 8.0))
            return bhr_fail(BHR_ERR_INVALID, "bhr_set_option: kerr_raymap_supersample %g (1, 2, 4 or 8)", value);
        o.kerr_raymap_ss = v;
    }
    else if (n == "kerr_line_row") {   // read by the next bhr_kerr_raymap_render under a Kerr line, which refuses a row that is not reserved
        if (!(value >= 0.0 && value <= 65535.0)) return bhr_fail(BHR_ERR_INVALID, "bhr_set_option: kerr_line_row %g (0 .. 65535)", value);
        o.kerr_line_row = v;
    }
    else if (n == "kerr_line_samples") o.kerr_line_samples = v != 0;
    else if (n == "png16_menu") {   // the tables are rebuilt at the next encode; no encode may be running on the old ones
        BHR_TRY(bhr_enter(ctx));
        BHR_HIP(hipStreamSynchronize(ctx->scene_stream));
        o.png16_menu = v != 0;
        bhr_png_dev_free(ctx);
    }
    else return bhr_fail(BHR_ERR_INVALID, "bhr_set_option: unknown option '%s'", name);
    return BHR_OK;
}

int32_t bhr_set_outputs(bhr_ctx *ctx, uint32_t mask) {
    if (!ctx || !(mask & (BHR_OUTPUT_F32 | BHR_OUTPUT_BLUR | BHR_OUTPUT_U8)) || (mask & ~(BHR_OUTPUT_F32 | BHR_OUTPUT_BLUR | BHR_OUTPUT_U8)))
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_outputs: mask %u", mask);
    ctx->out_want = mask;
    return BHR_OK;
}

}  // extern "C"
