// frame_slot.hip -- a frame slot's life: its buffers, entering and leaving its stream, its post-pass, and reading its layers.
#include <float.h>
#include <string.h>

#include "bhr_internal.h"

namespace {

// The bloom intermediates of slot k, on first use of either post-pass: the planar f32 H-blur planes of the exact kernels, or
// the packed f16 operands of the split kernels (bloom.hip).  Zero filled: halo rows outside the image stay zero for the
// life of the context, and so do the padding groups of the packed layouts.
int32_t ensure_bloom_buffers(bhr_ctx *ctx, int k, bool split) {
    bhr_frame_slot &f = ctx->slots[k];
    const size_t W = ctx->cfg.width, rows = ctx->rows, R = ctx->bloom_R;
    if (split) {
        if (f.d_pa && f.d_pb) return BHR_OK;
        bhr_split_geom g;
        bhr_split_geometry(ctx, &g);
        _Float16 *pa = nullptr, *pb = nullptr;
        int32_t rc = BHR_OK;
        if ((rc = bhr_dev_alloc(&pa, g.pa_halfs)) || (rc = bhr_dev_alloc(&pb, g.pb_halfs)) || (rc = bhr_dev_alloc(&f.d_sum, rows * W * 3))) {
            if (pa) (void)hipFree(pa);                       // a later retry starts clean
            if (pb) (void)hipFree(pb);
            return rc;                                       // (d_sum is the last one: null when it failed)
        }
        f.d_pa = pa;
        f.d_pb = pb;
        BHR_HIP(hipMemsetAsync(f.d_pa, 0, g.pa_halfs * 2, ctx->scene_stream));
        BHR_HIP(hipMemsetAsync(f.d_pb, 0, g.pb_halfs * 2, ctx->scene_stream));
    } else {
        if (f.d_hblur_base) return BHR_OK;
        const size_t n = 3 * (rows + 2 * R) * W + 2 * BHR_HBLUR_PAD_ROWS * W;
        BHR_TRY(bhr_dev_alloc(&f.d_hblur_base, n));
        f.d_hblur = f.d_hblur_base + BHR_HBLUR_PAD_ROWS * W;
        BHR_HIP(hipMemsetAsync(f.d_hblur_base, 0, n * sizeof(float), ctx->scene_stream));
    }
    BHR_HIP(hipStreamSynchronize(ctx->scene_stream));
    return BHR_OK;
}

__global__ void quantize_u8_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    // save_image: (np.clip(x, 0, 1) * 255).astype(np.uint8) -- truncation (render.py:423)
    for (; i < n; i += stride) dst[i] = (uint8_t)(int)(fminf(fmaxf(src[i], 0.0f), 1.0f) * 255.0f);
}

}  // namespace

int32_t bhr_alloc_slot(bhr_ctx *ctx, int k) {
    bhr_frame_slot &f = ctx->slots[k];
    if (f.allocated) return BHR_OK;
    const size_t px3 = (size_t)ctx->rows * ctx->cfg.width * 3;
    if (!f.stream) {
        if (k == 0 && ctx->n_slots == 1) f.stream = ctx->scene_stream;
        else BHR_HIP(hipStreamCreateWithFlags(&f.stream, hipStreamNonBlocking));
    }
    if (!f.done) BHR_HIP(hipEventCreateWithFlags(&f.done, hipEventDisableTiming));
    int32_t rc = BHR_OK;
    if ((rc = bhr_dev_alloc(&f.d_bg, px3)) || (rc = bhr_dev_alloc(&f.d_disk, px3)) || (rc = bhr_dev_alloc(&f.d_blur, px3)) ||
        (rc = bhr_dev_alloc(&f.d_final, px3)) || (rc = bhr_dev_alloc(&f.d_final_u8, px3)) || (rc = bhr_dev_alloc(&f.d_queue, 1))) {
        void *bufs[] = {f.d_bg, f.d_disk, f.d_blur, f.d_final, f.d_final_u8, f.d_queue};   // a later retry starts clean
        for (void *b : bufs)
            if (b) (void)hipFree(b);
        f.d_bg = f.d_disk = f.d_blur = f.d_final = nullptr;
        f.d_final_u8 = nullptr;
        f.d_queue = nullptr;
        return rc;
    }
    f.allocated = 1;
    return BHR_OK;
}

void bhr_free_slot(bhr_ctx *ctx, int k) {
    bhr_frame_slot &f = ctx->slots[k];
    void *bufs[] = {f.d_bg, f.d_disk, f.d_blur, f.d_final, f.d_final_u8, f.d_final_u16, f.d_hblur_base, f.d_pa, f.d_pb, f.d_sum, f.d_queue,
                    f.d_glow_hw, f.d_glow_wh, f.d_flare_c0, f.d_flare_c12, f.d_flare_sums, f.d_ada_list, f.d_ada_mask, f.d_ada_counts, f.d_acc_bg, f.d_acc_disk, f.d_hdr, f.d_star_plane, f.d_stokes, f.d_stokes_cells, f.d_line_samples};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (f.done) (void)hipEventDestroy(f.done);
    if (f.stokes_done) (void)hipEventDestroy(f.stokes_done);
    if (f.line_done) (void)hipEventDestroy(f.line_done);
    if (f.stream &&f.stream != ctx->scene_stream) (void)hipStreamDestroy(f.stream);
    if (f.aux_stream) (void)hipStreamDestroy(f.aux_stream);      // idle: bhr_destroy has waited for every slot's
    if (f.aux_fork) (void)hipEventDestroy(f.aux_fork);
    if (f.aux_done) (void)hipEventDestroy(f.aux_done);
    memset(&f, 0, sizeof(f));
}

// group / tile renders and the stand-alone passes work on slot 0 whatever bhr_render left active
int32_t bhr_activate_slot(bhr_ctx *ctx, int32_t k) {
    if (k < 0 || k >= BHR_MAX_FRAME_SLOTS) return bhr_fail(BHR_ERR_INVALID, "frame slot %d", k);
    BHR_TRY(bhr_alloc_slot(ctx, k));
    ctx->active_slot = k;
    return BHR_OK;
}

int32_t bhr_enter(bhr_ctx *ctx) {
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    for (int k = 0; k < BHR_MAX_FRAME_SLOTS; ++k) {
        bhr_frame_slot &f = ctx->slots[k];
        if (f.in_flight && f.stream != ctx->scene_stream) BHR_HIP(hipStreamWaitEvent(ctx->scene_stream, f.done, 0));
        f.in_flight = 0;
    }
    ctx->stream = ctx->scene_stream;
    return BHR_OK;
}

int32_t bhr_enter_components(bhr_ctx *ctx) {
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    ctx->stream = ctx->scene_stream;
    return BHR_OK;
}

int32_t bhr_enter_scene_write(bhr_ctx *ctx) {
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    for (int k = 0; k < BHR_MAX_FRAME_SLOTS; ++k) {
        bhr_frame_slot &f = ctx->slots[k];
        if (f.in_flight && f.stream != ctx->scene_stream && f.march_done) BHR_HIP(hipStreamWaitEvent(ctx->scene_stream, f.march_done, 0));
    }
    ctx->stream = ctx->scene_stream;
    return BHR_OK;
}

int32_t bhr_enter_frame(bhr_ctx *ctx) {
    bhr_frame_slot &f = bhr_slot(ctx);
    if (!f.allocated || !f.stream || f.stream == ctx->scene_stream) return bhr_enter(ctx);
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    BHR_HIP(hipEventRecord(ctx->scene_ev, ctx->scene_stream));      // e.g. a bhr_write_layer(FINAL) since the render
    BHR_HIP(hipStreamWaitEvent(f.stream, ctx->scene_ev, 0));
    ctx->stream = f.stream;
    return BHR_OK;
}

int32_t bhr_leave_frame(bhr_ctx *ctx) {
    bhr_frame_slot &f = bhr_slot(ctx);
    if (ctx->stream != ctx->scene_stream && ctx->stream == f.stream) {
        BHR_HIP(hipEventRecord(f.done, f.stream));                  // joins now wait for this work too
        f.in_flight = 1;
    }
    ctx->stream = ctx->scene_stream;
    return BHR_OK;
}

int32_t bhr_aux_fork(bhr_ctx *ctx) {
    if (!ctx->slots[0].aux_stream) {
        // normal priority, one stream per frame slot, all created now
        for (auto &q : ctx->slots) {
            BHR_HIP(hipStreamCreateWithPriority(&q.aux_stream, hipStreamNonBlocking, 0));
            BHR_HIP(hipEventCreateWithFlags(&q.aux_fork, hipEventDisableTiming));
            BHR_HIP(hipEventCreateWithFlags(&q.aux_done, hipEventDisableTiming));
        }
    }
    bhr_frame_slot &f = bhr_slot(ctx);
    BHR_HIP(hipEventRecord(f.aux_fork, ctx->stream));
    BHR_HIP(hipStreamWaitEvent(f.aux_stream, f.aux_fork, 0));
    return BHR_OK;
}

int32_t bhr_aux_join(bhr_ctx *ctx) {
    bhr_frame_slot &f = bhr_slot(ctx);
    BHR_HIP(hipEventRecord(f.aux_done, f.aux_stream));
    BHR_HIP(hipStreamWaitEvent(ctx->stream, f.aux_done, 0));
    return BHR_OK;
}

int32_t bhr_frame_begin(bhr_ctx *ctx, uint32_t flags, bool exact) {
    const int mode = bhr_resolve_math(ctx, flags);
    // the frame's post-pass follows its march: exact f32 chains under strict, the split-f16 matrix-core kernels (bloom.hip)
    // under fast and hybrid; BHR_BLOOM_SPLIT=0 / 1 forces either for every arithmetic
    int split = ctx->opt.bloom_split >= 0 ? ctx->opt.bloom_split : (mode != BHR_MATH_STRICT ? 1 : 0);
    if (exact || !ctx->split_ok || (flags & BHR_SKIP_BLOOM)) split = 0;
    if (!(flags & BHR_SKIP_BLOOM)) BHR_TRY(ensure_bloom_buffers(ctx, ctx->active_slot, split != 0));
    bhr_frame_slot &f = bhr_slot(ctx);
    f.have = 0;
    f.sum_valid = 0;
    f.frame_split = split;
    f.frame_with_bloom = (flags & BHR_SKIP_BLOOM) ? 0 : 1;
    return BHR_OK;
}

int32_t bhr_frame_post(bhr_ctx *ctx, int32_t with_bloom, uint32_t want, unsigned long long *zero_cell) {
    BHR_TRY(bhr_launch_bloom_v_rows(ctx, with_bloom, 0, ctx->rows, want, nullptr, nullptr, zero_cell));
    bhr_slot(ctx).have = want;
    return BHR_OK;
}

int32_t bhr_frame_flare(bhr_ctx *ctx, bool hdr) {
    BHR_TRY(bhr_launch_flare_glow(ctx, true));
    BHR_TRY(bhr_launch_flare_sums(ctx));
    return bhr_launch_flare_apply(ctx, nullptr, hdr);
}

// the u8 rows (BHR_OUT_U8) are already in d_final_u8 when the frame's V pass stored them, else FINAL -> u8
int32_t bhr_ensure_outputs(bhr_ctx *ctx, uint32_t need) {
    bhr_frame_slot &f = bhr_slot(ctx);
    uint32_t missing = need & ~f.have;
    if (!missing) return BHR_OK;
    // the quantisers of their own (quantize.hip) read the f32 frame: the 16-bit rows always, the u8 rows while dither is on
    const uint32_t from_f32 = missing & (BHR_OUT_U16 | (ctx->dither ? BHR_OUT_U8 : 0u));
    if (from_f32) {
        BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_F32));
        if (from_f32 & BHR_OUT_U16) BHR_TRY(bhr_launch_quantize_u16(ctx));
        if (from_f32 & BHR_OUT_U8) BHR_TRY(bhr_launch_quantize_dither(ctx));
        f.have |= from_f32;
        missing = need & ~f.have;
        if (!missing) return BHR_OK;
    }
    if ((missing & BHR_OUT_U8) && ((f.have | missing) & BHR_OUT_F32)) {
        // the f32 frame is (or is about to be) the authority -- it may carry a lens flare the V pass knows nothing of
        if (missing & BHR_OUT_F32) BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_F32));
        const long long n = (long long)ctx->rows * ctx->cfg.width * 3;
        hipLaunchKernelGGL(quantize_u8_kernel, dim3(2048), dim3(256), 0, ctx->stream, f.d_final, f.d_final_u8, n);
        BHR_HIP(hipGetLastError());
        f.have |= BHR_OUT_U8;
        missing &= ~(BHR_OUT_U8 | BHR_OUT_F32);
        if (!missing) return BHR_OK;
    }
    // re-run the frame's V pass for what nobody asked for up front (its inputs -- bg, disk, the H-blur planes -- are still the
    // slot's, and it records which post-pass the frame ran): same kernels, same bits
    BHR_TRY(bhr_launch_bloom_v_rows(ctx, f.frame_with_bloom, 0, ctx->rows, missing, nullptr, nullptr, nullptr));
    f.have |= missing;
    return BHR_OK;
}

extern "C" {

int32_t bhr_read_layer(bhr_ctx *ctx, int32_t layer, float *out) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_read_layer: bad argument");
    BHR_TRY(bhr_enter(ctx));
    const float *src = nullptr;
    const bhr_frame_slot &f = bhr_slot(ctx);
    switch (layer) {
        case BHR_LAYER_FINAL: src = f.d_final; BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_F32)); break;
        case BHR_LAYER_BG: src = f.d_bg; break;
        case BHR_LAYER_DISK: src = f.d_disk; break;
        case BHR_LAYER_BLUR: src = f.d_blur; BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_BLUR)); break;
        case BHR_LAYER_HDR:
            if (!(f.have & BHR_OUT_HDR) || !f.d_hdr)
                return bhr_fail(BHR_ERR_STATE, "bhr_read_layer: the frame kept no HDR plane (bhr_set_grade with keep_hdr, then render or bhr_grade_frame)");
            src = f.d_hdr;
            break;
        default: return bhr_fail(BHR_ERR_INVALID, "bhr_read_layer: unknown layer %d", layer);
    }
    return bhr_download(ctx, out, src, (size_t)ctx->rows * ctx->cfg.width * 3 * sizeof(float));
}

int32_t bhr_write_layer(bhr_ctx *ctx, int32_t layer, const float *in) {
    if (!ctx || !in) return bhr_fail(BHR_ERR_INVALID, "bhr_write_layer: bad argument");
    BHR_TRY(bhr_enter(ctx));
    if (layer == BHR_LAYER_HDR) return bhr_fail(BHR_ERR_INVALID, "bhr_write_layer: BHR_LAYER_HDR is read only");
    float *dst = nullptr;
    bhr_frame_slot &f = bhr_slot(ctx);
    const size_t n = (size_t)ctx->rows * ctx->cfg.width * 3;
    int32_t wide = 0;
    if (layer == BHR_LAYER_DISK) {
        // the bloom folds the reference's `lum > 0` test away (bloom.hip), which holds for non-negative layers only; values
        // above what the split kernels' f16 halves carry send the stand-alone pass to the exact kernels (bhr_bloom)
        for (size_t k = 0; k < n; ++k) {
            const float v = in[k];
            if (!(v >= 0.0f && v <= FLT_MAX))
                return bhr_fail(BHR_ERR_INVALID, "bhr_write_layer: disk value %g at row %zu, column %zu (finite values >= 0 only)",
                                (double)v, k / 3 / ctx->cfg.width, k / 3 % ctx->cfg.width);
            wide |= v > BHR_SPLIT_DISK_MAX;
        }
    }
    switch (layer) {
        case BHR_LAYER_FINAL: dst = f.d_final; f.have = (f.have | BHR_OUT_F32) & ~(BHR_OUT_U8 | BHR_OUT_U16); break;   // the u8 / u16 rows follow the written frame
        case BHR_LAYER_BG: dst = f.d_bg; f.sum_valid = 0; break;      // a later V pass adds the two layers itself
        case BHR_LAYER_DISK: dst = f.d_disk; f.sum_valid = 0; f.disk_wide = wide; break;
        case BHR_LAYER_BLUR: dst = f.d_blur; f.have |= BHR_OUT_BLUR; break;
        default: return bhr_fail(BHR_ERR_INVALID, "bhr_write_layer: unknown layer %d", layer);
    }
    return bhr_upload(ctx, dst, in, n * sizeof(float));
}

int32_t bhr_bloom(bhr_ctx *ctx) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_bloom: null ctx");
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "bhr_bloom: needs a whole-frame context (rows %d of %d)", ctx->rows, ctx->cfg.height);
    BHR_TRY(bhr_enter(ctx));
    // the context's arithmetic decides the kernels, as for a rendered frame -- except for a written disk layer the split
    // kernels cannot carry: the pass stays one function of its input whatever the arithmetic
    BHR_TRY(bhr_frame_begin(ctx, 0, bhr_slot(ctx).disk_wide != 0));
    if (bhr_slot(ctx).frame_split) BHR_TRY(bhr_launch_bloom_pack(ctx)); // the disk layer may be the caller's (bhr_write_layer)
    BHR_TRY(bhr_launch_bloom_h(ctx, nullptr, 0));
    return bhr_frame_post(ctx, 1, BHR_OUT_F32 | BHR_OUT_BLUR, nullptr);
}

int32_t bhr_lens_flare(bhr_ctx *ctx) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_lens_flare: null ctx");
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "bhr_lens_flare: needs a whole-frame context (rows %d of %d)", ctx->rows, ctx->cfg.height);
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_F32));
    bhr_slot(ctx).have &= ~(BHR_OUT_U8 | BHR_OUT_U16);          // the u8 / u16 rows follow the flared frame
    return bhr_frame_flare(ctx, false);
}

int32_t bhr_lens_flare_sums(bhr_ctx *ctx, double *out3) {
    if (!ctx || !out3) return bhr_fail(BHR_ERR_INVALID, "bhr_lens_flare_sums: bad argument");
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "bhr_lens_flare_sums: needs a whole-frame context (rows %d of %d)", ctx->rows, ctx->cfg.height);
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(bhr_launch_flare_glow(ctx, true));
    BHR_TRY(bhr_launch_flare_sums(ctx));
    return bhr_download(ctx, out3, bhr_slot(ctx).d_flare_sums, 3 * sizeof(double));
}

int32_t bhr_read_gathered(bhr_ctx *ctx, float *out) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_read_gathered: bad argument");
    if (!ctx->d_gather) return bhr_fail(BHR_ERR_STATE, "bhr_read_gathered: no bhr_group_render(..., BHR_GATHER_PEER) has gathered into this context");
    BHR_TRY(bhr_enter(ctx));
    return bhr_download(ctx, out, ctx->d_gather, (size_t)ctx->cfg.height * ctx->cfg.width * 3 * sizeof(float));
}

int32_t bhr_read_final_u8(bhr_ctx *ctx, uint8_t *out) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_read_final_u8: bad argument");
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_U8));
    return bhr_download(ctx, out, bhr_slot(ctx).d_final_u8, (size_t)ctx->rows * ctx->cfg.width * 3);
}

}  // extern "C"
