// scene.hip -- the scene's entry points: skybox, disk texture and mips, background layer, component planes, compose, noise.
#include <math.h>

#include <vector>

#include "bhr_internal.h"

namespace {

// Allocates the packed mip stack for an (n_r, n_phi) texture.
int32_t alloc_mips(bhr_ctx *ctx, int32_t n_r, int32_t n_phi) {
    int64_t off = 0;
    int32_t h = n_r, w = n_phi;
    for (int l = 0; l < BHR_NUM_MIP_LEVELS; ++l) {
        ctx->mip_off[l] = (int32_t)off;
        ctx->mip_h[l] = h;
        ctx->mip_w[l] = w;
        off += (int64_t)h * w;
        // generate_disk_mipmaps stops when h < 2 or w < 2 (render.py:1118-1119)
        if (h < 2 || w < 2) { h = 0; w = 0; } else { h /= 2; w /= 2; }
    }
    if (off >= (1ll << 31)) return bhr_fail(BHR_ERR_INVALID, "disk texture too large (%d x %d)", n_r, n_phi);
    ctx->mip_texels = off;
    ctx->n_r = n_r;
    ctx->n_phi = n_phi;
    BHR_TRY(bhr_dev_alloc(&ctx->d_mips, (size_t)off));
    BHR_HIP(hipMemsetAsync(ctx->d_mips, 0, (size_t)off * sizeof(float4), ctx->stream));
    return BHR_OK;
}

}  // namespace

void bhr_free_scene(bhr_ctx *ctx) {
    if (ctx->d_mips) (void)hipFree(ctx->d_mips);
    ctx->d_mips = nullptr;
}

void bhr_free_bg(bhr_ctx *ctx) {
    if (ctx->d_comp) (void)hipFree(ctx->d_comp);
    if (ctx->d_edge) (void)hipFree(ctx->d_edge);
    if (ctx->d_omega) (void)hipFree(ctx->d_omega);
    if (ctx->d_row_stats) (void)hipFree(ctx->d_row_stats);
    ctx->d_comp = ctx->d_edge = ctx->d_omega = ctx->d_row_stats = nullptr;
    ctx->bg_ready = 0;
}

extern "C" {

int32_t bhr_set_skybox(bhr_ctx *ctx, const float *rgb, int32_t tex_h, int32_t tex_w) {
    if (!ctx || !rgb || tex_h <= 0 || tex_w <= 0) return bhr_fail(BHR_ERR_INVALID, "bhr_set_skybox: bad argument");
    BHR_TRY(bhr_enter(ctx));
    if (ctx->d_skybox && (ctx->sky_h != tex_h || ctx->sky_w != tex_w)) {
        BHR_HIP(hipStreamSynchronize(ctx->stream));
        (void)hipFree(ctx->d_skybox);
        ctx->d_skybox = nullptr;
    }
    if (!ctx->d_skybox) BHR_TRY(bhr_dev_alloc(&ctx->d_skybox, (size_t)tex_h * tex_w * 3));
    ctx->sky_h = tex_h;
    ctx->sky_w = tex_w;
    return bhr_upload(ctx, ctx->d_skybox, rgb, (size_t)tex_h * tex_w * 3 * sizeof(float));
}

int32_t bhr_set_disk_texture(bhr_ctx *ctx, const float *rgba, int32_t n_r, int32_t n_phi) {
    if (!ctx || !rgba || n_r <= 0 || n_phi <= 0) return bhr_fail(BHR_ERR_INVALID, "bhr_set_disk_texture: bad argument");
    BHR_TRY(bhr_enter(ctx));
    if (ctx->d_mips && (ctx->n_r != n_r || ctx->n_phi != n_phi))
        return bhr_fail(BHR_ERR_INVALID, "Texture size mismatch: expected %dx%d, got %dx%d", ctx->n_r, ctx->n_phi, n_r, n_phi);
    if (!ctx->d_mips) BHR_TRY(alloc_mips(ctx, n_r, n_phi));
    BHR_TRY(bhr_upload(ctx, ctx->d_mips, rgba, (size_t)n_r * n_phi * sizeof(float4)));
    return bhr_launch_build_mips(ctx);
}

int32_t bhr_get_disk_texture(bhr_ctx *ctx, float *rgba_out) { return bhr_get_disk_mip(ctx, 0, rgba_out); }

int32_t bhr_get_disk_mip(bhr_ctx *ctx, int32_t level, float *rgba_out) {
    if (!ctx || !rgba_out) return bhr_fail(BHR_ERR_INVALID, "bhr_get_disk_mip: bad argument");
    if (!ctx->d_mips) return bhr_fail(BHR_ERR_STATE, "bhr_get_disk_mip: no disk texture");
    if (level < 0 || level >= BHR_NUM_MIP_LEVELS) return bhr_fail(BHR_ERR_INVALID, "bhr_get_disk_mip: level %d", level);
    BHR_TRY(bhr_enter(ctx));
    size_t n = (size_t)ctx->mip_h[level] * ctx->mip_w[level];
    if (n == 0) return BHR_OK;
    return bhr_download(ctx, rgba_out, ctx->d_mips + ctx->mip_off[level], n * sizeof(float4));
}

int32_t bhr_num_mip_levels(bhr_ctx *ctx) {
    if (!ctx || !ctx->d_mips) return 0;
    int n = 0;
    for (int l = 0; l < BHR_NUM_MIP_LEVELS; ++l)
        if (ctx->mip_h[l] > 0 && ctx->mip_w[l] > 0) ++n;
    return n;
}

int32_t bhr_bg_init(bhr_ctx *ctx, int32_t n_r, int32_t n_phi, int32_t az_freq, float az_shear, const float *edge,
                    const float *omega_rows) {
    if (!ctx || !edge || !omega_rows || n_r <= 0 || n_phi <= 0) return bhr_fail(BHR_ERR_INVALID, "bhr_bg_init: bad argument");
    BHR_TRY(bhr_enter(ctx));
    if (ctx->d_mips && (ctx->n_r != n_r || ctx->n_phi != n_phi))
        return bhr_fail(BHR_ERR_INVALID, "bhr_bg_init: (%d,%d) does not match the disk texture (%d,%d)", n_r, n_phi, ctx->n_r, ctx->n_phi);
    if (!ctx->d_mips) BHR_TRY(alloc_mips(ctx, n_r, n_phi));
    const size_t plane = (size_t)n_r * n_phi;
    if (!ctx->d_comp || ctx->bg_n_r != n_r || ctx->bg_n_phi != n_phi) {
        BHR_HIP(hipStreamSynchronize(ctx->stream));
        bhr_free_bg(ctx);
        BHR_TRY(bhr_dev_alloc(&ctx->d_comp, 13 * plane));
        BHR_TRY(bhr_dev_alloc(&ctx->d_edge, (size_t)n_r));
        BHR_TRY(bhr_dev_alloc(&ctx->d_omega, (size_t)n_r));
        BHR_TRY(bhr_dev_alloc(&ctx->d_row_stats, (size_t)n_r * 2));
        BHR_HIP(hipMemsetAsync(ctx->d_comp, 0, 13 * plane * sizeof(float), ctx->stream));
    }
    ctx->bg_n_r = n_r;
    ctx->bg_n_phi = n_phi;
    ctx->az_freq = az_freq;
    ctx->az_shear = az_shear;
    BHR_TRY(bhr_upload(ctx, ctx->d_edge, edge, (size_t)n_r * sizeof(float)));
    BHR_TRY(bhr_upload(ctx, ctx->d_omega, omega_rows, (size_t)n_r * sizeof(float)));
    // initial stats (render.py:3531-3542): stats (0.5, 0.5); row stats from the undisturbed
    // temp_base profile max(tb, 0.25), max(0.8 tb, 0.10) with tb = clip(1 - r, 0, 1)^1.3 * 0.25
    ctx->stats[0] = 0.5f;
    ctx->stats[1] = 0.5f;
    std::vector<float> rs((size_t)n_r * 2);
    for (int i = 0; i < n_r; ++i) {
        double rn = n_r > 1 ? (double)i / (double)(n_r - 1) : 0.0;  // np.linspace(0, 1, n_r)
        double c = 1.0 - rn;
        if (c < 0) c = 0;
        if (c > 1) c = 1;
        double tb = pow(c, 1.3) * 0.25;
        double a = tb > 0.25 ? tb : 0.25;
        double b = tb * 0.8 > 0.10 ? tb * 0.8 : 0.10;
        rs[(size_t)i * 2 + 0] = (float)a;
        rs[(size_t)i * 2 + 1] = (float)b;
    }
    BHR_TRY(bhr_upload(ctx, ctx->d_row_stats, rs.data(), rs.size() * sizeof(float)));
    ctx->bg_ready = 1;
    return BHR_OK;
}

int32_t bhr_generate_background(bhr_ctx *ctx, float t) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "null ctx");
    if (!ctx->bg_ready) return bhr_fail(BHR_ERR_STATE, "Must call init_background_layer() first");
    BHR_TRY(bhr_enter_components(ctx));          // writes comp only: runs beside the frame in flight
    BHR_HIP(hipEventRecord(ctx->ev[4], ctx->stream));
    BHR_TRY(bhr_launch_background(ctx, t));
    BHR_HIP(hipEventRecord(ctx->ev[5], ctx->stream));
    return BHR_OK;
}

int32_t bhr_set_entity_staging(bhr_ctx *ctx, const float *staging) {
    if (!ctx || !staging) return bhr_fail(BHR_ERR_INVALID, "bhr_set_entity_staging: bad argument");
    if (!ctx->bg_ready) return bhr_fail(BHR_ERR_STATE, "Must call init_background_layer() first");
    BHR_TRY(bhr_enter(ctx));
    const size_t plane = (size_t)ctx->bg_n_r * ctx->bg_n_phi;
    return bhr_upload(ctx, ctx->d_comp + 5 * plane, staging, 6 * plane * sizeof(float));
}

int32_t bhr_set_comp(bhr_ctx *ctx, const float *comp13) {
    if (!ctx || !comp13) return bhr_fail(BHR_ERR_INVALID, "bhr_set_comp: bad argument");
    if (!ctx->bg_ready) return bhr_fail(BHR_ERR_STATE, "bhr_set_comp: call bhr_bg_init first");
    BHR_TRY(bhr_enter(ctx));
    const size_t plane = (size_t)ctx->bg_n_r * ctx->bg_n_phi;
    return bhr_upload(ctx, ctx->d_comp, comp13, 13 * plane * sizeof(float));
}

int32_t bhr_read_comp(bhr_ctx *ctx, float *comp13_out) {
    if (!ctx || !comp13_out) return bhr_fail(BHR_ERR_INVALID, "bhr_read_comp: bad argument");
    if (!ctx->bg_ready) return bhr_fail(BHR_ERR_STATE, "bhr_read_comp: call bhr_bg_init first");
    BHR_TRY(bhr_enter(ctx));
    const size_t plane = (size_t)ctx->bg_n_r * ctx->bg_n_phi;
    return bhr_download(ctx, comp13_out, ctx->d_comp, 13 * plane * sizeof(float));
}

int32_t bhr_fill_comp_slice(bhr_ctx *ctx, int32_t idx, float value) {
    if (!ctx || idx < 0 || idx >= 13) return bhr_fail(BHR_ERR_INVALID, "bhr_fill_comp_slice: bad argument");
    if (!ctx->bg_ready) return bhr_fail(BHR_ERR_STATE, "bhr_fill_comp_slice: call bhr_bg_init first");
    BHR_TRY(bhr_enter(ctx));
    const size_t plane = (size_t)ctx->bg_n_r * ctx->bg_n_phi;
    return bhr_launch_fill(ctx, ctx->d_comp + idx * plane, (int64_t)plane, value);
}

int32_t bhr_set_compose_stats(bhr_ctx *ctx, float density_p98, float struct_scale, const float *row_stats) {
    if (!ctx || !row_stats) return bhr_fail(BHR_ERR_INVALID, "bhr_set_compose_stats: bad argument");
    if (!ctx->bg_ready) return bhr_fail(BHR_ERR_STATE, "bhr_set_compose_stats: call bhr_bg_init first");
    BHR_TRY(bhr_enter(ctx));
    ctx->stats[0] = density_p98;
    ctx->stats[1] = struct_scale;
    return bhr_upload(ctx, ctx->d_row_stats, row_stats, (size_t)ctx->bg_n_r * 2 * sizeof(float));
}

int32_t bhr_compose_texture(bhr_ctx *ctx, float t_offset, int32_t enable_rt, float color_temp) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "null ctx");
    if (!ctx->bg_ready) return bhr_fail(BHR_ERR_STATE, "Must call upload_parametric_state() / init_background_layer() before composing");
    BHR_TRY(bhr_enter_scene_write(ctx));
    BHR_HIP(hipEventRecord(ctx->ev[6], ctx->stream));
    BHR_TRY(bhr_launch_compose(ctx, t_offset, enable_rt, color_temp));
    BHR_HIP(hipEventRecord(ctx->ev[7], ctx->stream));
    return BHR_OK;
}

int32_t bhr_eval_noise(bhr_ctx *ctx, const float *coords, int64_t n, int32_t mode, int32_t octaves,
                       float persistence, float lacunarity, float *out) {
    if (!ctx || !coords || !out || n < 0) return bhr_fail(BHR_ERR_INVALID, "bhr_eval_noise: bad argument");
    if (n == 0) return BHR_OK;
    BHR_TRY(bhr_enter(ctx));
    if (ctx->noise_cap < n) {
        BHR_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->d_noise_in) (void)hipFree(ctx->d_noise_in);
        if (ctx->d_noise_out) (void)hipFree(ctx->d_noise_out);
        ctx->d_noise_in = ctx->d_noise_out = nullptr;
        ctx->noise_cap = 0;
        BHR_TRY(bhr_dev_alloc(&ctx->d_noise_in, (size_t)n * 3));
        BHR_TRY(bhr_dev_alloc(&ctx->d_noise_out, (size_t)n));
        ctx->noise_cap = n;
    }
    BHR_TRY(bhr_upload(ctx, ctx->d_noise_in, coords, (size_t)n * 3 * sizeof(float)));
    BHR_TRY(bhr_launch_noise(ctx, n, mode, octaves, persistence, lacunarity));
    return bhr_download(ctx, out, ctx->d_noise_out, (size_t)n * sizeof(float));
}

}  // extern "C"
