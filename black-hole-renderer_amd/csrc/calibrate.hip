// calibrate.hip -- which hardware queues the frame slots' streams sit on: the probe, and the choice of slot 1's stream by timing.
#include <chrono>

#include "bhr_internal.h"

namespace {

// ---- do two streams sit on ONE hardware queue? ------------------------------------------------------------------------------
// HIP hands its streams to a small pool of hardware queues (four per priority by default) by rules of its own; two streams
// on one queue run their kernels strictly one after the other, two on different queues side by side -- which decides how the
// two frame slots' launches interleave.  The probe: a one-lane kernel on `a` that spins until released (or 4 ms
// of the 100 MHz real-time counter), a one-lane kernel on `b` that raises a flag in pinned memory.  The flag rises while the
// spinner is still held -> different queues.
__global__ void probe_spin_kernel(volatile int *release, volatile int *spinning) {
    const unsigned long long t0 = __builtin_readcyclecounter();
    *spinning = 1;
    __threadfence_system();
    const unsigned long long r0 = wall_clock64();
    while (*release == 0 && wall_clock64() - r0 < 400000ull) __builtin_amdgcn_s_sleep(8);
    (void)t0;
}
__global__ void probe_flag_kernel(volatile int *flag) { *flag = 1; __threadfence_system(); }

}  // namespace

int32_t bhr_streams_share_queue(hipStream_t a, hipStream_t b, int32_t *share) {
    if (a == b) { *share = 1; return BHR_OK; }
    volatile int *h = nullptr;
    BHR_HIP(hipHostMalloc((void **)&h, 3 * sizeof(int), hipHostMallocDefault));
    h[0] = h[1] = h[2] = 0;                               // release, spinning, flag
    hipLaunchKernelGGL(probe_spin_kernel, dim3(1), dim3(1), 0, a, h + 0, h + 1);
    const auto t0 = std::chrono::steady_clock::now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    while (h[1] == 0 && ms() < 3.0) {}                    // the spinner is on the chip
    hipLaunchKernelGGL(probe_flag_kernel, dim3(1), dim3(1), 0, b, h + 2);
    const double t1 = ms();
    while (h[2] == 0 && ms() - t1 < 1.0) {}               // a kernel on a free queue lands in ~10 us
    *share = h[2] == 0;
    h[0] = 1;
    const hipError_t e1 = hipStreamSynchronize(a), e2 = hipStreamSynchronize(b);
    (void)hipHostFree((void *)h);
    BHR_HIP(e1);
    BHR_HIP(e2);
    return BHR_OK;
}

// Which stream should frame slot 1 submit to?  Two slots keep two frames in flight so that one frame's post-pass and the
// ragged end of its march run under the next frame's march -- and how well they do is decided by which HARDWARE queues HIP
// gave the two slots' streams: measured on one binary, 2200-2360 fps (pairs of queues on which the second frame's
// workgroups interleave with the first's from the start) or 2740-2770 (pairs on which they fill in behind), by nothing but
// the number of idle streams the process had created before (profiles/r04_stream_mapping.txt; round 3 shipped whatever the library's
// own creation order happened to give).  HIP does not tell which queue a stream got and the good pairs are not simply
// "different queues" (bhr_streams_share_queue finds those): so the context MEASURES.  Once eight two-slot frames have been
// asked for, six candidate streams (created back to back: they go round HIP's queues) take turns as slot 1's stream for 24
// frames of the caller's own view, three times; the fastest (by its worst turn) stays, the rest idle.  ~0.2 s, once per context, frames
// identical to the one asked for; BHR_CALIBRATE_STREAMS=0 / option "calibrate_streams" 0 keeps the first stream, and so does a
// context whose frames take more than 4 ms (the first turn tells: 4k / 8k frames would spend seconds here for a per cent).
int32_t bhr_calibrate_slot_streams(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags) {
    constexpr int NC = 6, FRAMES = 24;
    ctx->calibrating = 1;
    const auto head0 = ctx->ring_head;
    const int slot0 = ctx->next_slot;
    hipStream_t cand[NC] = {};
    double best_ms[NC];
    int32_t rc = bhr_alloc_slot(ctx, 0);
    if (rc == BHR_OK) rc = bhr_alloc_slot(ctx, 1);
    if (rc != BHR_OK) { ctx->calibrating = 0; return rc; }
    cand[0] = ctx->slots[1].stream;
    int n_cand = 1;
    for (; n_cand < NC; ++n_cand)
        if (hipStreamCreateWithFlags(&cand[n_cand], hipStreamNonBlocking) != hipSuccess) break;
    for (int c = 0; c < NC; ++c) best_ms[c] = 1e30;
    // Between turns everything is waited for and the timing ring is put back where the caller's frames had brought it: a turn
    // runs at most 64 frames through the cells in front of the caller's, never round the ring into the ones his own frames are
    // on record in (with the ring left to run, three turns of six candidates are 628 frames of a ring of 512).  The next
    // frames' counter cells are cleared as the V pass of their predecessors would have left them.
    auto drain = [&]() -> int32_t {
        for (int k = 0; k < 2; ++k) BHR_TRY(bhr_poll_sync(ctx, ctx->slots[k].stream));      // (polled: a turn is 8 ms, an interrupt's wake-up up to 2)
        for (int q = 0; q < BHR_MAX_FRAME_SLOTS; ++q)
            BHR_HIP(hipMemsetAsync(ctx->d_steps_ring + (size_t)((head0 + q) % BHR_TIMING_RING) * BHR_STEP_CELL, 0, sizeof(unsigned long long) * BHR_STEP_CELL, ctx->scene_stream));
        BHR_TRY(bhr_poll_sync(ctx, ctx->scene_stream));
        ctx->ring_head = head0;
        ctx->next_slot = slot0;
        return BHR_OK;
    };
    auto frames = [&](int n) -> int32_t {
        for (int i = 0; i < n; ++i) BHR_TRY(bhr_render(ctx, cam, flags));
        return BHR_OK;
    };
    // frames of several milliseconds (4k, 8k) gain little from which pair of queues the two slots got and would make this a
    // matter of seconds: one turn tells, the first stream stays
    bool long_frames = false;
    for (int pass = 0; pass < 3 && rc == BHR_OK && !long_frames; ++pass)
        for (int c = 0; c < n_cand && rc == BHR_OK; ++c) {
            rc = drain();
            if (rc != BHR_OK) break;
            ctx->slots[1].stream = cand[c];
            rc = frames(pass == 0 && c == 0 ? 40 : 6);                 // the first candidate also brings the clocks up
            if (rc == BHR_OK) rc = drain();
            const auto t0 = std::chrono::steady_clock::now();
            if (rc == BHR_OK) rc = frames(FRAMES);
            if (rc == BHR_OK) rc = drain();
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rc == BHR_OK && (pass == 0 || ms > best_ms[c])) best_ms[c] = ms;      // the WORST of its three turns: a pair has to be good every time
            if (pass == 0 && c == 0 && ms > 4.0 * FRAMES) { long_frames = true; break; }
        }
    // the level a good pair reaches: the fastest single turn of any candidate
    double good_ms = 1e30;
    for (int c = 0; c < n_cand; ++c) good_ms = best_ms[c] < good_ms ? best_ms[c] : good_ms;
    int best = 0;
    for (int tries = 0; tries < 4 && rc == BHR_OK && !long_frames; ++tries) {
        best = 0;
        // the fastest, with no preference for the earlier ones: a candidate within 1 % of the fastest was, in 8 of 8 bench runs
        // that kept it over the fastest, a pair that later dropped to its slow state (2400 instead of 2900 fps) -- the stream
        // that measures best is also the one that stays there (18 of 18 runs)
        for (int c = 1; c < n_cand; ++c)
            if (best_ms[c] < best_ms[best]) best = c;
        // a longer turn with the one chosen: kept if it holds the good level (a pair can sit 3 % under it for a while; the
        // next candidate then gets its chance)
        rc = drain();
        if (rc != BHR_OK) break;
        ctx->slots[1].stream = cand[best];
        rc = frames(6);
        if (rc == BHR_OK) rc = drain();
        const auto t0 = std::chrono::steady_clock::now();
        if (rc == BHR_OK) rc = frames(2 * FRAMES);
        if (rc == BHR_OK) rc = drain();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / 2;
        if (rc != BHR_OK || ms <= good_ms * 1.015) break;
        best_ms[best] = ms > best_ms[best] ? ms : best_ms[best] * 1.02;
    }
    if (rc != BHR_OK) best = 0;
    (void)drain();
    ctx->slots[1].stream = cand[best];
    // the others stay, idle, until the context goes: the choice was measured with them in place (with them destroyed -- HIP
    // then gives up hardware queues nobody references -- the kept pair ran 12 % slower than it had been measured, on one of
    // twelve stream layouts)
    for (int c = 0; c < n_cand; ++c)
        if (c != best && cand[c]) ctx->calib_idle[ctx->n_calib_idle++] = cand[c];
    ctx->calib_choice = best;
    for (int c = 0; c < 8; ++c) ctx->calib_fps[c] = c < n_cand && best_ms[c] < 1e29 ? (int32_t)(FRAMES * 1e3 / best_ms[c]) : 0;
    // (the last drain() has left the timing ring where the caller's frames had brought it)
    ctx->ring_head = head0;
    ctx->next_slot = slot0;
    ctx->calibrating = 0;
    ctx->streams_calibrated = 1;
    return rc;
}
