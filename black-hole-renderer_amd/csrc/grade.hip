// grade.hip -- the grading stage between the combine and the quantisers (include/bhr.h: bhr_set_grade, bhr_grade_frame).
//
// Per value, all in f32, every operation rounded once (the object is compiled without contraction and without fast-math):
//   x = (bg + disk) + blur                       the combine's own order -- or the flared HDR plane of the frame slot
//   h = fminf(fmaxf(x, 0), 65504)                the HDR value: NaN -> 0 as in the quantisers, +inf -> 65504
//   v = h * gain                                 gain = (float)exp2((double)exposure_stops), from the host
//   clip      y = fminf(v, 1)
//   reinhard  y = fminf((v * (1 + v * iw2)) / (1 + v), 1)                               iw2 = (float)(1 / ((double)white * white))
//   aces      y = fminf(fmaxf((v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f), 0), 1)
//   linear    FINAL = y
//   srgb      FINAL = y <= 0.0031308f ? 12.92f * y : 1.055f * powf(y, 1.0f / 2.4f) - 0.055f
// The kernel stores FINAL, the plane h where the frame keeps it, and -- where the frame's consumers want undithered u8 rows --
// those rows as well, by frame_slot.hip's quantize_u8_kernel's expression of FINAL.  tests/grade_ref.py restates all of it in NumPy.
// Streaming, like shutter.hip: every lane moves 16 bytes per f32 access (4 bytes of u8 rows), consecutive lanes consecutive
// float4s, grid-stride over at most 2048 blocks, the count's remainder mod 4 by scalar accesses; no LDS, no scratch.
#include <algorithm>
#include <cmath>

#include "bhr_internal.h"

namespace {

struct GradeArgs {
    const float *bg, *disk, *blur;   // the layers (src null)
    float *src;                      // non-null: x is read from this plane (the flared HDR plane; may be `hdr` itself)
    float *fin;                      // FINAL
    float *hdr;                      // null: h is not stored
    uint8_t *u8;                     // null: no u8 rows
    long long n4, n;                 // float4s, floats
    float gain, iw2;
};

template <int OP, int TRANSFER>
__device__ __forceinline__ float grade_value(float x, float gain, float iw2, float *h_out) {
#pragma clang fp contract(off)
    const float h = fminf(fmaxf(x, 0.0f), 65504.0f);
    *h_out = h;
    const float v = h * gain;
    float y;
    if (OP == BHR_GRADE_CLIP) y = fminf(v, 1.0f);
    else if (OP == BHR_GRADE_REINHARD) y = fminf((v * (1.0f + v * iw2)) / (1.0f + v), 1.0f);
    else y = fminf(fmaxf((v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f), 0.0f), 1.0f);
    if (TRANSFER == BHR_TRANSFER_SRGB) y = y <= 0.0031308f ? 12.92f * y : 1.055f * powf(y, 1.0f / 2.4f) - 0.055f;
    return y;
}

// quantize_u8_kernel's expression (frame_slot.hip), bit for bit
__device__ __forceinline__ uint32_t grade_q8(float f) { return (uint32_t)(uint8_t)(int)(fminf(fmaxf(f, 0.0f), 1.0f) * 255.0f); }

__device__ __forceinline__ float grade_sum(float bg, float disk, float blur) {
#pragma clang fp contract(off)
    return (bg + disk) + blur;
}

// No __restrict__: src and hdr are one plane for a flared frame (every value is read and written by the one lane that owns it).
template <int OP, int TRANSFER>
__global__ __launch_bounds__(256) void grade_kernel(GradeArgs a) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const float4 *bg4 = reinterpret_cast<const float4 *>(a.bg), *disk4 = reinterpret_cast<const float4 *>(a.disk);
    const float4 *blur4 = reinterpret_cast<const float4 *>(a.blur), *src4 = reinterpret_cast<const float4 *>(a.src);
    float4 *fin4 = reinterpret_cast<float4 *>(a.fin), *hdr4 = reinterpret_cast<float4 *>(a.hdr);
    uint32_t *u8w = reinterpret_cast<uint32_t *>(a.u8);
    for (long long i = t; i < a.n4; i += stride) {
        float4 x;
        if (a.src) {
            x = src4[i];
        } else {
            const float4 b = bg4[i], d = disk4[i], l = blur4[i];
            x = make_float4(grade_sum(b.x, d.x, l.x), grade_sum(b.y, d.y, l.y), grade_sum(b.z, d.z, l.z), grade_sum(b.w, d.w, l.w));
        }
        float4 h, y;
        y.x = grade_value<OP, TRANSFER>(x.x, a.gain, a.iw2, &h.x);
        y.y = grade_value<OP, TRANSFER>(x.y, a.gain, a.iw2, &h.y);
        y.z = grade_value<OP, TRANSFER>(x.z, a.gain, a.iw2, &h.z);
        y.w = grade_value<OP, TRANSFER>(x.w, a.gain, a.iw2, &h.w);
        fin4[i] = y;
        if (a.hdr) hdr4[i] = h;
        if (a.u8) u8w[i] = grade_q8(y.x) | (grade_q8(y.y) << 8) | (grade_q8(y.z) << 16) | (grade_q8(y.w) << 24);   // little endian: byte k is value 4 i + k
    }
    for (long long i = 4 * a.n4 + t; i < a.n; i += stride) {
        const float x = a.src ? a.src[i] : grade_sum(a.bg[i], a.disk[i], a.blur[i]);
        float h;
        const float y = grade_value<OP, TRANSFER>(x, a.gain, a.iw2, &h);
        a.fin[i] = y;
        if (a.hdr) a.hdr[i] = h;
        if (a.u8) a.u8[i] = (uint8_t)grade_q8(y);
    }
}

// s = (bg + disk) + blur into the HDR plane: what the flare's apply kernel adds its term to ahead of the grade
__global__ __launch_bounds__(256) void grade_sum_kernel(const float *__restrict__ bg, const float *__restrict__ disk, const float *__restrict__ blur,
                                                        float *__restrict__ hdr, long long n4, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const float4 *bg4 = reinterpret_cast<const float4 *>(bg), *disk4 = reinterpret_cast<const float4 *>(disk), *blur4 = reinterpret_cast<const float4 *>(blur);
    float4 *hdr4 = reinterpret_cast<float4 *>(hdr);
    for (long long i = t; i < n4; i += stride) {
        const float4 b = bg4[i], d = disk4[i], l = blur4[i];
        hdr4[i] = make_float4(grade_sum(b.x, d.x, l.x), grade_sum(b.y, d.y, l.y), grade_sum(b.z, d.z, l.z), grade_sum(b.w, d.w, l.w));
    }
    for (long long i = 4 * n4 + t; i < n; i += stride) hdr[i] = grade_sum(bg[i], disk[i], blur[i]);
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

unsigned grid_for(long long work) { return (unsigned)std::min<long long>(std::max<long long>((work + 255) / 256, 1), 2048); }

int32_t ensure_hdr(bhr_ctx *ctx) {
    bhr_frame_slot &f = bhr_slot(ctx);
    if (f.d_hdr) return BHR_OK;
    const size_t bytes = (size_t)ctx->rows * ctx->cfg.width * 3 * sizeof(float);
    const hipError_t e = hipMalloc((void **)&f.d_hdr, bytes);
    if (e != hipSuccess) {
        f.d_hdr = nullptr;
        return bhr_fail(BHR_ERR_NOMEM, "hipMalloc(%zu bytes) for the HDR plane failed: %s", bytes, hipGetErrorString(e));
    }
    return BHR_OK;
}

// option "grade_timing": launch `slot` (0 or 1) of the frame's grade stage is bracketed by a pair of the context's events
int32_t timing_begin(bhr_ctx *ctx, int slot) {
    if (!ctx->opt.grade_timing) return BHR_OK;
    if (!ctx->grade_ev[0])
        for (auto &e : ctx->grade_ev) BHR_HIP(hipEventCreate(&e));
    if (slot == 0) ctx->grade_ev_n = 0;
    BHR_HIP(hipEventRecord(ctx->grade_ev[2 * slot], ctx->stream));
    return BHR_OK;
}

int32_t timing_end(bhr_ctx *ctx, int slot) {
    if (!ctx->opt.grade_timing) return BHR_OK;
    BHR_HIP(hipEventRecord(ctx->grade_ev[2 * slot + 1], ctx->stream));
    ctx->grade_ev_n = slot + 1;
    return BHR_OK;
}

typedef void (*grade_fn)(GradeArgs);
grade_fn grade_kernel_for(int op, int transfer) {
    static const grade_fn table[3][2] = {
        {grade_kernel<BHR_GRADE_CLIP, BHR_TRANSFER_LINEAR>, grade_kernel<BHR_GRADE_CLIP, BHR_TRANSFER_SRGB>},
        {grade_kernel<BHR_GRADE_REINHARD, BHR_TRANSFER_LINEAR>, grade_kernel<BHR_GRADE_REINHARD, BHR_TRANSFER_SRGB>},
        {grade_kernel<BHR_GRADE_ACES, BHR_TRANSFER_LINEAR>, grade_kernel<BHR_GRADE_ACES, BHR_TRANSFER_SRGB>},
    };
    return table[op][transfer];
}

}  // namespace

int32_t bhr_launch_grade_sum(bhr_ctx *ctx) {
    BHR_TRY(ensure_hdr(ctx));
    bhr_frame_slot &f = bhr_slot(ctx);
    const long long n = (long long)ctx->rows * ctx->cfg.width * 3;
    const bool wide = aligned16(f.d_bg) && aligned16(f.d_disk) && aligned16(f.d_blur) && aligned16(f.d_hdr);
    const long long n4 = wide ? n / 4 : 0;
    BHR_TRY(timing_begin(ctx, 0));
    hipLaunchKernelGGL(grade_sum_kernel, dim3(grid_for(n4 > 0 ? n4 : n)), dim3(256), 0, ctx->stream, f.d_bg, f.d_disk, f.d_blur, f.d_hdr, n4, n);
    BHR_HIP(hipGetLastError());
    return timing_end(ctx, 0);
}

int32_t bhr_launch_grade(bhr_ctx *ctx, bool from_hdr, bool store_hdr, bool store_u8) {
    if (!ctx->grade_on) return bhr_fail(BHR_ERR_STATE, "grade: no grade is set (bhr_set_grade)");
    if (from_hdr || store_hdr) BHR_TRY(ensure_hdr(ctx));
    bhr_frame_slot &f = bhr_slot(ctx);
    GradeArgs a;
    a.bg = f.d_bg; a.disk = f.d_disk; a.blur = f.d_blur;
    a.src = from_hdr ? f.d_hdr : nullptr;
    a.fin = f.d_final;
    a.hdr = (from_hdr || store_hdr) ? f.d_hdr : nullptr;   // a flared plane is clamped in place: the plane is h
    a.u8 = store_u8 ? f.d_final_u8 : nullptr;
    a.n = (long long)ctx->rows * ctx->cfg.width * 3;
    // 16-byte accesses where every plane starts on a 16-byte boundary (hipMalloc's do), else the scalar loop takes it all
    const bool wide = aligned16(a.bg) && aligned16(a.disk) && aligned16(a.blur) && aligned16(a.fin) && aligned16(f.d_hdr) && aligned16(f.d_final_u8);
    a.n4 = wide ? a.n / 4 : 0;
    a.gain = ctx->grade_gain;
    a.iw2 = ctx->grade_iw2;
    const int slot = from_hdr ? 1 : 0;                    // a flared frame's sum kernel came first
    BHR_TRY(timing_begin(ctx, slot));
    hipLaunchKernelGGL(grade_kernel_for(ctx->grade.op, ctx->grade.transfer), dim3(grid_for(a.n4 > 0 ? a.n4 : a.n)), dim3(256), 0, ctx->stream, a);
    BHR_HIP(hipGetLastError());
    return timing_end(ctx, slot);
}

void bhr_grade_free(bhr_ctx *ctx) {
    for (auto &e : ctx->grade_ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    ctx->grade_ev_n = 0;
}

extern "C" {

int32_t bhr_set_grade(bhr_ctx *ctx, const bhr_grade *g) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_set_grade: null ctx");
    if (g) {
        if (g->op < BHR_GRADE_CLIP || g->op > BHR_GRADE_ACES) return bhr_fail(BHR_ERR_INVALID, "bhr_set_grade: op %d (0 clip, 1 reinhard, 2 aces)", g->op);
        if (g->transfer != BHR_TRANSFER_LINEAR && g->transfer != BHR_TRANSFER_SRGB)
            return bhr_fail(BHR_ERR_INVALID, "bhr_set_grade: transfer %d (0 linear, 1 srgb)", g->transfer);
        if (!(g->exposure_stops >= -16.0f && g->exposure_stops <= 16.0f))
            return bhr_fail(BHR_ERR_INVALID, "bhr_set_grade: exposure of %g stops (finite, -16 .. 16)", (double)g->exposure_stops);
        if (!(g->white > 0.0f && g->white <= 65504.0f)) return bhr_fail(BHR_ERR_INVALID, "bhr_set_grade: white %g (finite, in (0, 65504])", (double)g->white);
    }
    BHR_TRY(bhr_enter(ctx));                                       // behind the frames in flight ...
    BHR_HIP(hipStreamSynchronize(ctx->stream));                    // ... which are drained; the frames in memory keep their outputs
    if (!g) {
        ctx->grade_on = 0;
        return BHR_OK;
    }
    ctx->grade = *g;
    ctx->grade.keep_hdr = g->keep_hdr != 0;
    ctx->grade_gain = (float)exp2((double)g->exposure_stops);
    ctx->grade_iw2 = (float)(1.0 / ((double)g->white * (double)g->white));
    ctx->grade_on = 1;
    return BHR_OK;
}

int32_t bhr_grade_frame(bhr_ctx *ctx) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_grade_frame: null ctx");
    if (!ctx->grade_on) return bhr_fail(BHR_ERR_STATE, "bhr_grade_frame: no grade is set (bhr_set_grade)");
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_BLUR));                // a frame that did not keep its blur layer gets it from its V pass
    const bool keep = ctx->grade.keep_hdr != 0;
    BHR_TRY(bhr_launch_grade(ctx, false, keep, false));
    bhr_frame_slot &f = bhr_slot(ctx);
    f.have = (f.have | BHR_OUT_F32) & ~(BHR_OUT_U8 | BHR_OUT_U16 | BHR_OUT_HDR);   // the u8 / u16 rows follow the graded frame
    if (keep) f.have |= BHR_OUT_HDR;
    return BHR_OK;
}

}  // extern "C"
