// counters.hip -- what a context reports about the frames it has launched: counters, the timing ring, row costs, diagnostics.
#include <algorithm>
#include <utility>
#include <vector>

#include "bhr_internal.h"

namespace {

// sum of the lanes of `n` counter cells -> host
__global__ void steps_fold_kernel(const unsigned long long *__restrict__ cells, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long sh[BHR_STEP_LANES];
    sh[threadIdx.x] = cells[(size_t)blockIdx.x * BHR_STEP_CELL + (size_t)threadIdx.x * BHR_STEP_STRIDE];
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < BHR_STEP_LANES; ++k) t += sh[k];
        out[blockIdx.x] = t;
    }
}

// The refined pixels of the last adaptive frame: {tiles in the two lists, refined pixels in them} of its slot's counts.  Synchronises.
int32_t adaptive_counts(bhr_ctx *ctx, unsigned int n[4]) {
    n[0] = n[1] = n[2] = n[3] = 0;
    return bhr_download(ctx, n, ctx->slots[ctx->ada_info_slot].d_ada_counts, 4 * sizeof(unsigned int));
}
bool adaptive_on_record(const bhr_ctx *ctx) { return ctx->ada_info_slot >= 0 && ctx->slots[ctx->ada_info_slot].d_ada_counts; }

// What both row-cost read-outs check before they copy: the band count, and that the last frame filled the profile.
int32_t row_costs_check(const bhr_ctx *ctx, const char *who, int32_t n, int32_t *bands) {
    *bands = (ctx->rows + 7) / 8;
    if (n != *bands) return bhr_fail(BHR_ERR_INVALID, "%s: the context has %d 8-row bands, caller asked for %d", who, *bands, n);
    if (!ctx->d_row_steps || !(ctx->last.flags & BHR_ROW_COSTS))
        return bhr_fail(BHR_ERR_STATE, "%s: the last bhr_render did not carry BHR_ROW_COSTS", who);
    return BHR_OK;
}

// bhr_debug_read's timing reports (options "shutter_timing", "grade_timing"): geom[0] = the n bracketed launches of the last
// such frame, geom[1] = their time in ns, from n (start, end) event pairs
int32_t bracket_report(bhr_ctx *ctx, const hipEvent_t *ev, int32_t n, const char *what, int32_t *geom) {
    if (!geom) return bhr_fail(BHR_ERR_INVALID, "bhr_debug_read: %s timing needs geom", what);
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    double ms = 0.0;
    for (int j = 0; j < n; ++j) ms += (double)bhr_ev_ms(ev[2 * j], ev[2 * j + 1]);
    geom[0] = n;
    geom[1] = (int32_t)(ms * 1e6 + 0.5);
    return BHR_OK;
}

}  // namespace

float bhr_ev_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return -1.0f;
    return ms;
}

int32_t bhr_fold_cells(bhr_ctx *ctx, const unsigned long long *cells, int n, unsigned long long *host_out) {
    hipLaunchKernelGGL(steps_fold_kernel, dim3(n), dim3(BHR_STEP_LANES), 0, ctx->stream, cells, ctx->d_steps_fold);
    BHR_HIP(hipGetLastError());
    BHR_HIP(hipMemcpyAsync(host_out, ctx->d_steps_fold, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    return BHR_OK;
}

extern "C" {

int32_t bhr_get_counters(bhr_ctx *ctx, bhr_counters *out) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_get_counters: bad argument");
    BHR_TRY(bhr_enter(ctx));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    const bhr_last_frame &last = ctx->last;
    if (last.valid) {
        unsigned long long steps = 0;
        BHR_TRY(bhr_fold_cells(ctx, bhr_steps_cell(ctx, last.ring), 1, &steps));
        ctx->counters.ray_steps = steps;
        ctx->counters.rays = last.rays;
        // the last launch's three events: its ring slot's (bhr_render) or the context's scalar ones (group render)
        const hipEvent_t *e = last.ring >= 0 ? ctx->ring_ev + last.ring * 3 : ctx->ev;
        ctx->counters.march_ms = last.march_timed ? bhr_ev_ms(e[0], e[1]) : -1.0f;      // a group render without BHR_GROUP_TIME_MARCH: not timed
        ctx->counters.bloom_ms = last.march_timed ? bhr_ev_ms(e[1], e[2]) : -1.0f;
        ctx->counters.frame_ms = bhr_ev_ms(e[0], e[2]);
    }
    {
        // the cells after the head have been cleared for the frames to come: at most RING - MAX_SLOTS frames are on record
        const int64_t n = ctx->ring_head < BHR_TIMING_RING - BHR_MAX_FRAME_SLOTS ? ctx->ring_head : BHR_TIMING_RING - BHR_MAX_FRAME_SLOTS;
        float ms_m = 0.0f, ms_b = 0.0f;
        unsigned long long steps_sum = 0;
        if (n > 0) {
            std::vector<unsigned long long> hs(BHR_TIMING_RING);
            BHR_TRY(bhr_fold_cells(ctx, ctx->d_steps_ring, BHR_TIMING_RING, hs.data()));
            for (int64_t k = 0; k < n; ++k) {
                const int slot = (int)((ctx->ring_head - 1 - k) % BHR_TIMING_RING);
                ms_m += bhr_ev_ms(ctx->ring_ev[slot * 3 + 0], ctx->ring_ev[slot * 3 + 1]);
                ms_b += bhr_ev_ms(ctx->ring_ev[slot * 3 + 1], ctx->ring_ev[slot * 3 + 2]);
                steps_sum += hs[slot];
            }
        }
        // union of the march intervals, on the clock of the oldest timed frame's start event (events of the two
        // slot streams are comparable: hipEventElapsedTime works across streams of one device)
        float busy = 0.0f, span = 0.0f;
        if (n > 0) {
            const int first = (int)((ctx->ring_head - n) % BHR_TIMING_RING);
            const hipEvent_t origin = ctx->ring_ev[first * 3 + 0];
            std::vector<std::pair<float, float>> iv((size_t)n);
            for (int64_t k = 0; k < n; ++k) {
                const int slot = (int)((ctx->ring_head - n + k) % BHR_TIMING_RING);
                iv[(size_t)k] = {bhr_ev_ms(origin, ctx->ring_ev[slot * 3 + 0]), bhr_ev_ms(origin, ctx->ring_ev[slot * 3 + 1])};
                span = std::max(span, bhr_ev_ms(origin, ctx->ring_ev[slot * 3 + 2]));
            }
            std::sort(iv.begin(), iv.end());
            float lo = iv[0].first, hi = iv[0].second;
            for (size_t k = 1; k < iv.size(); ++k) {
                if (iv[k].first > hi) { busy += hi - lo; lo = iv[k].first; hi = iv[k].second; }
                else hi = std::max(hi, iv[k].second);
            }
            busy += hi - lo;
        }
        ctx->counters.march_busy_ms = busy;
        ctx->counters.span_ms = span;
        ctx->counters.frames_timed = (int32_t)n;
        ctx->counters.march_ms_sum = ms_m;
        ctx->counters.bloom_ms_sum = ms_b;
        ctx->counters.ray_steps_sum = steps_sum;
    }
    if (ctx->bg_ready) {
        if (hipEventQuery(ctx->ev[5]) == hipSuccess) ctx->counters.background_ms = bhr_ev_ms(ctx->ev[4], ctx->ev[5]);
        if (hipEventQuery(ctx->ev[7]) == hipSuccess) ctx->counters.compose_ms = bhr_ev_ms(ctx->ev[6], ctx->ev[7]);
    }
    *out = ctx->counters;
    if (last.adaptive && adaptive_on_record(ctx)) {
        // an adaptive frame: the base march's rays on record and k^2 per refined pixel
        unsigned int n[4];
        BHR_TRY(adaptive_counts(ctx, n));
        out->rays += ((uint64_t)n[2] + n[3]) * (uint64_t)(ctx->ada_k * ctx->ada_k);
    }
    return BHR_OK;
}

// {refined pixels of the last adaptive frame, those of them marched strict, pixels of the frame}.  Synchronises.
int32_t bhr_adaptive_info(bhr_ctx *ctx, int64_t out[3]) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_adaptive_info: bad argument");
    if (ctx->ada_k <= 1 || !adaptive_on_record(ctx))
        return bhr_fail(BHR_ERR_STATE, "bhr_adaptive_info: no adaptively supersampled frame has been rendered (bhr_set_adaptive_supersample)");
    BHR_TRY(bhr_enter(ctx));
    unsigned int n[4];            // tiles in the two lists, refined pixels in them
    BHR_TRY(adaptive_counts(ctx, n));
    out[0] = (int64_t)n[2] + (int64_t)n[3];
    out[1] = ctx->ada_info_math == BHR_MATH_FAST ? 0 : (int64_t)n[2];
    out[2] = (int64_t)ctx->cfg.width * ctx->rows;
    return BHR_OK;
}

int32_t bhr_timing_dump(bhr_ctx *ctx, float *out, int32_t n) {
    if (!ctx || !out || n <= 0) return bhr_fail(BHR_ERR_INVALID, "bhr_timing_dump: bad argument");
    BHR_TRY(bhr_enter(ctx));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t have = ctx->ring_head < BHR_TIMING_RING - BHR_MAX_FRAME_SLOTS ? ctx->ring_head : BHR_TIMING_RING - BHR_MAX_FRAME_SLOTS;
    if (n > have) return bhr_fail(BHR_ERR_INVALID, "bhr_timing_dump: %d frames asked, %lld on record", n, (long long)have);
    const hipEvent_t origin = ctx->ring_ev[(int)((ctx->ring_head - n) % BHR_TIMING_RING) * 3];
    for (int k = 0; k < n; ++k) {
        const int slot = (int)((ctx->ring_head - n + k) % BHR_TIMING_RING);
        for (int e = 0; e < 3; ++e) out[k * 3 + e] = bhr_ev_ms(origin, ctx->ring_ev[slot * 3 + e]);
    }
    return BHR_OK;
}

int32_t bhr_timing_reset(bhr_ctx *ctx) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "null ctx");
    BHR_TRY(bhr_enter(ctx));
    BHR_HIP(hipMemsetAsync(ctx->d_steps_ring, 0, sizeof(unsigned long long) * BHR_TIMING_RING * BHR_STEP_CELL, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    ctx->ring_head = 0;
    return BHR_OK;
}

int32_t bhr_get_row_costs(bhr_ctx *ctx, uint64_t *out, int32_t n) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_get_row_costs: bad argument");
    int32_t bands = 0;
    BHR_TRY(row_costs_check(ctx, "bhr_get_row_costs", n, &bands));
    BHR_TRY(bhr_enter(ctx));
    std::vector<uint64_t> both((size_t)2 * bands);
    BHR_TRY(bhr_download(ctx, both.data(), ctx->d_row_steps, both.size() * sizeof(uint64_t)));
    for (int32_t k = 0; k < bands; ++k) out[k] = both[(size_t)k] + both[(size_t)bands + k];
    return BHR_OK;
}

int32_t bhr_get_row_costs_split(bhr_ctx *ctx, uint64_t *fast_out, uint64_t *strict_out, int32_t n) {
    if (!ctx || !fast_out || !strict_out) return bhr_fail(BHR_ERR_INVALID, "bhr_get_row_costs_split: bad argument");
    int32_t bands = 0;
    BHR_TRY(row_costs_check(ctx, "bhr_get_row_costs_split", n, &bands));
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(bhr_download(ctx, fast_out, ctx->d_row_steps, (size_t)bands * sizeof(uint64_t)));
    return bhr_download(ctx, strict_out, ctx->d_row_steps + bands, (size_t)bands * sizeof(uint64_t));
}

int32_t bhr_selftest(bhr_ctx *ctx, uint64_t out[4]) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_selftest: bad argument");
    BHR_TRY(bhr_enter(ctx));
    unsigned long long *d = nullptr;
    BHR_TRY(bhr_dev_alloc(&d, 4));
    int32_t rc = bhr_selftest_strict(ctx, d);
    if (rc == BHR_OK) rc = bhr_download(ctx, out, d, 4 * sizeof(unsigned long long));
    (void)hipFree(d);
    return rc;
}

int32_t bhr_mip_lds_level(bhr_ctx *ctx) { return ctx ? ctx->mip_lds_from : -1; }

int32_t bhr_debug_read(bhr_ctx *ctx, int32_t which, void *out, int64_t bytes, int32_t *geom) {
    if (!ctx || bytes < 0) return bhr_fail(BHR_ERR_INVALID, "bhr_debug_read: bad argument");
    BHR_TRY(bhr_enter(ctx));
    bhr_split_geom g;
    bhr_split_geometry(ctx, &g);
    if (geom) { geom[0] = g.NT; geom[1] = g.n_tx; geom[2] = g.WP; geom[3] = g.YB; geom[4] = g.GP; geom[5] = g.g0; geom[6] = g.t_first; geom[7] = g.n_ty; geom[8] = g.pbr; geom[9] = g.GR; }
    if (which == 4) {                                   // slot 1's stream calibration: geom[0] = done, [1] = candidate kept, [2..7] = candidates' fps
        if (!geom) return bhr_fail(BHR_ERR_INVALID, "bhr_debug_read: calibration report needs geom");
        geom[0] = ctx->streams_calibrated; geom[1] = ctx->calib_choice;
        for (int c = 0; c < 6; ++c) geom[2 + c] = ctx->calib_fps[c];
        return BHR_OK;
    }
    if (which == 5) return bracket_report(ctx, ctx->shutter_ev, ctx->shutter_ev_n, "shutter", geom);   // the last shutter frame's accumulation launches
    if (which == 6) return bracket_report(ctx, ctx->grade_ev, ctx->grade_ev_n, "grade", geom);         // the last graded frame's grade stage
    if (which == 3) {                                   // geom[0..9]: do pairs of the context's streams share a hardware queue (-1: no such stream)
        if (!geom) return bhr_fail(BHR_ERR_INVALID, "bhr_debug_read: stream map needs geom");
        hipStream_t st[5] = {ctx->scene_stream, ctx->slots[0].stream, ctx->n_slots > 1 ? ctx->slots[1].stream : nullptr, ctx->slots[0].aux_stream, ctx->slots[1].aux_stream};
        int q = 0;                                      // pairs in the order (0,1) (0,2) (0,3) (0,4) (1,2) (1,3) (1,4) (2,3) (2,4) (3,4); 0 scene, 1 / 2 frame slots, 3 / 4 second march streams
        for (int i = 0; i < 5; ++i)
            for (int j = i + 1; j < 5; ++j, ++q) {
                geom[q] = -1;
                if (st[i] && st[j]) BHR_TRY(bhr_streams_share_queue(st[i], st[j], &geom[q]));
            }
        return BHR_OK;
    }
    if (which == 2) {                                   // the partitioned launch order of the last hybrid march (int32 tile indices)
        const int32_t *list = nullptr;
        int32_t n = 0;
        BHR_TRY(bhr_hybrid_active_list(ctx, &list, &n));
        if (geom) geom[0] = n;
        if (!out || bytes == 0) return BHR_OK;
        if (bytes > (int64_t)n * 4) return bhr_fail(BHR_ERR_INVALID, "bhr_debug_read: %lld bytes asked, the list holds %d tiles", (long long)bytes, n);
        return bhr_download(ctx, out, list, (size_t)bytes);
    }
    const void *src = which == 0 ? bhr_slot(ctx).d_pa : which == 1 ? bhr_slot(ctx).d_pb : nullptr;
    const size_t have = which == 0 ? g.pa_halfs * 2 : g.pb_halfs * 2;
    if (!out || bytes == 0) return BHR_OK;
    if (!src) return bhr_fail(BHR_ERR_STATE, "bhr_debug_read: buffer %d does not exist (no split-f16 frame yet)", which);
    if ((size_t)bytes > have) return bhr_fail(BHR_ERR_INVALID, "bhr_debug_read: %lld bytes asked, the buffer holds %zu", (long long)bytes, have);
    return bhr_download(ctx, out, src, (size_t)bytes);
}

}  // extern "C"
