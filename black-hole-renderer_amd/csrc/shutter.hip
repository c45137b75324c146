// shutter.hip -- the accumulation of a shutter frame (bhr_render_shutter, render.hip).
//
// A shutter frame is the mean of n marches: every sample is marched into the frame slot's own d_bg / d_disk by the march
// kernels as they are, and one launch of the kernel below follows each march on the slot's stream:
//   sample 0            acc = L                           (copy: the march launcher stays as it is)
//   sample 0 < j < n-1  acc = acc + L                     (one f32 addition per channel)
//   sample n - 1        L   = (acc + L) * (1.0f / n)      (the reciprocal rounded once, the product once)
// for L in {BG, DISK}, both layers in the one launch.  n = 1 launches nothing: the frame is L_0 itself.  The sums are two
// f32 planes of the frame slot (d_acc_bg, d_acc_disk: allocated here on first use, freed with the slot, never shared
// between slots).  Streaming: every lane moves 16 bytes per access, consecutive lanes consecutive float4s (a wave touches
// 1 KiB per instruction), grid-stride over at most 2048 blocks, the count's remainder mod 4 by scalar accesses; no LDS.
#include <algorithm>

#include "bhr_internal.h"

namespace {

enum { SH_FIRST = 0, SH_ADD = 1, SH_LAST = 2 };

template <int MODE>
__device__ __forceinline__ float sh_value(float acc, float l, float inv) {
#pragma clang fp contract(off)
    if (MODE == SH_FIRST) return l;
    const float s = acc + l;
    if (MODE == SH_ADD) return s;
    return s * inv;
}

// one plane: n4 float4s, then the floats [4 n4, n).  SH_FIRST / SH_ADD store into acc, SH_LAST into the layer.
template <int MODE>
__device__ __forceinline__ void sh_plane(float *__restrict__ acc, float *__restrict__ layer, long long n4, long long n, float inv) {
#pragma clang fp contract(off)
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float4 *acc4 = reinterpret_cast<float4 *>(acc);
    float4 *layer4 = reinterpret_cast<float4 *>(layer);
    for (long long i = t; i < n4; i += stride) {
        const float4 l = layer4[i];
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (MODE != SH_FIRST) a = acc4[i];
        float4 r;
        r.x = sh_value<MODE>(a.x, l.x, inv);
        r.y = sh_value<MODE>(a.y, l.y, inv);
        r.z = sh_value<MODE>(a.z, l.z, inv);
        r.w = sh_value<MODE>(a.w, l.w, inv);
        if (MODE == SH_LAST) layer4[i] = r;
        else acc4[i] = r;
    }
    for (long long i = 4 * n4 + t; i < n; i += stride) {
        const float r = sh_value<MODE>(MODE != SH_FIRST ? acc[i] : 0.0f, layer[i], inv);
        if (MODE == SH_LAST) layer[i] = r;
        else acc[i] = r;
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void shutter_accumulate_kernel(float *__restrict__ acc_bg, float *__restrict__ acc_disk, float *__restrict__ bg,
                                                                 float *__restrict__ disk, long long n4, long long n, float inv) {
    sh_plane<MODE>(acc_bg, bg, n4, n, inv);
    sh_plane<MODE>(acc_disk, disk, n4, n, inv);
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

int32_t bhr_launch_shutter_accumulate(bhr_ctx *ctx, int32_t j, int32_t n_samples) {
    if (n_samples < 2 || j < 0 || j >= n_samples) return bhr_fail(BHR_ERR_INVALID, "shutter accumulation: sample %d of %d", j, n_samples);
    bhr_frame_slot &f = bhr_slot(ctx);
    const long long n = (long long)ctx->rows * ctx->cfg.width * 3;
    if (!f.d_acc_bg) BHR_HIP(hipMalloc((void **)&f.d_acc_bg, (size_t)n * sizeof(float)));
    if (!f.d_acc_disk) BHR_HIP(hipMalloc((void **)&f.d_acc_disk, (size_t)n * sizeof(float)));
    // 16-byte accesses where every plane starts on a 16-byte boundary (hipMalloc's do), else the scalar loop takes it all
    const bool wide = aligned16(f.d_acc_bg) && aligned16(f.d_acc_disk) && aligned16(f.d_bg) && aligned16(f.d_disk);
    const long long n4 = wide ? n / 4 : 0;
    const long long work = n4 > 0 ? n4 : n;
    const unsigned blocks = (unsigned)std::min<long long>(std::max<long long>((work + 255) / 256, 1), 2048);
    const float inv = 1.0f / (float)n_samples;
    const bool timed = ctx->opt.shutter_timing != 0;
    if (timed && !ctx->shutter_ev[0])
        for (auto &e : ctx->shutter_ev) BHR_HIP(hipEventCreate(&e));
    if (j == 0) ctx->shutter_ev_n = 0;
    if (timed) BHR_HIP(hipEventRecord(ctx->shutter_ev[2 * j], ctx->stream));
    const dim3 grid(blocks), block(256);
    if (j == 0) hipLaunchKernelGGL(shutter_accumulate_kernel<SH_FIRST>, grid, block, 0, ctx->stream, f.d_acc_bg, f.d_acc_disk, f.d_bg, f.d_disk, n4, n, inv);
    else if (j < n_samples - 1) hipLaunchKernelGGL(shutter_accumulate_kernel<SH_ADD>, grid, block, 0, ctx->stream, f.d_acc_bg, f.d_acc_disk, f.d_bg, f.d_disk, n4, n, inv);
    else hipLaunchKernelGGL(shutter_accumulate_kernel<SH_LAST>, grid, block, 0, ctx->stream, f.d_acc_bg, f.d_acc_disk, f.d_bg, f.d_disk, n4, n, inv);
    BHR_HIP(hipGetLastError());
    if (timed) {
        BHR_HIP(hipEventRecord(ctx->shutter_ev[2 * j + 1], ctx->stream));
        ctx->shutter_ev_n = j + 1;
    }
    return BHR_OK;
}

void bhr_shutter_free(bhr_ctx *ctx) {
    for (auto &e : ctx->shutter_ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    ctx->shutter_ev_n = 0;
}
