// quantize.hip -- the two quantisers of the f32 FINAL frame that are kernels of their own (include/bhr.h: bhr_read_final_u16,
// bhr_set_dither), beside save_image's truncation, which the V pass fuses into its store (bloom.hip) and frame_slot.hip's
// quantize_u8_kernel repeats for a flared frame.  Both are reached through bhr_ensure_outputs.
//
//   16 bit:   q16 = (uint16)(int)(clip(x, 0, 1) * 65535.0f)              the same truncation, 65536 levels
//   dither:   q8  = (uint8)floorf(clip(x, 0, 1) * 255.0f + t(c, X, Y))   t = (M[(Y + oy_c) & 63][(X + ox_c) & 63] + 0.5) / 4096
// with M the 64 x 64 blue-noise rank matrix of blue_noise_64.h (tools/make_blue_noise.py), (X, Y) the pixel's coordinates in
// the FULL image (a row block dithers as the whole frame does) and the channel offsets (0, 0), (21, 37), (43, 11).  The product
// and the sum are rounded to f32 once each (no FMA); 255 + 4095.5 / 4096 < 256, so nothing is clamped afterwards.  NaN -> 0
// through fmaxf, as in the 8-bit path.  tests/quant_ref.py restates both in NumPy.
#include "bhr_internal.h"
#include "blue_noise_64.h"

#include <cstring>

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void quantize_u16_kernel(const float *__restrict__ src, uint16_t *__restrict__ dst, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = (uint16_t)(int)__fmul_rn(fminf(fmaxf(src[i], 0.0f), 1.0f), 65535.0f);
}

// One thread per value, the matrix in LDS (8 KB): every value of a block's rows looks up three scattered entries.
__global__ __launch_bounds__(kBlock) void quantize_u8_dither_kernel(const float *__restrict__ src, uint8_t *__restrict__ dst, long long n,
                                                                    int w, int row0, const uint16_t *__restrict__ matrix) {
    __shared__ uint16_t m[4096];
    for (int k = threadIdx.x; k < 2048; k += kBlock) ((uint32_t *)m)[k] = ((const uint32_t *)matrix)[k];
    __syncthreads();
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long w3 = 3ll * w;
    for (; i < n; i += stride) {
        const long long j = i / w3;
        const int rem = (int)(i - j * w3), x = rem / 3, c = rem - 3 * x;
        const int ox = c == 0 ? 0 : (c == 1 ? 21 : 43), oy = c == 0 ? 0 : (c == 1 ? 37 : 11);
        const int X = (x + ox) & 63, Y = (int)((row0 + j + oy) & 63);
        const float t = ((float)m[64 * Y + X] + 0.5f) / 4096.0f;       // exact: 13 significant bits, a power of two
        const float v = __fmul_rn(fminf(fmaxf(src[i], 0.0f), 1.0f), 255.0f);
        dst[i] = (uint8_t)(int)floorf(__fadd_rn(v, t));
    }
}

int grid_for(long long n) {
    const long long blocks = (n + kBlock - 1) / kBlock;
    return (int)(blocks < 4096 ? blocks : 4096);
}

}  // namespace

int32_t bhr_launch_quantize_u16(bhr_ctx *ctx) {
    bhr_frame_slot &f = bhr_slot(ctx);
    const long long n = (long long)ctx->rows * ctx->cfg.width * 3;
    if (!f.d_final_u16) {
        const hipError_t e = hipMalloc((void **)&f.d_final_u16, (size_t)n * sizeof(uint16_t));
        if (e != hipSuccess) {
            f.d_final_u16 = nullptr;
            return bhr_fail(BHR_ERR_NOMEM, "hipMalloc(%lld bytes) for the 16-bit rows failed: %s", n * 2, hipGetErrorString(e));
        }
    }
    hipLaunchKernelGGL(quantize_u16_kernel, dim3(grid_for(n)), dim3(kBlock), 0, ctx->stream, f.d_final, f.d_final_u16, n);
    BHR_HIP(hipGetLastError());
    return BHR_OK;
}

int32_t bhr_launch_quantize_dither(bhr_ctx *ctx) {
    bhr_frame_slot &f = bhr_slot(ctx);
    if (!ctx->d_dither) return bhr_fail(BHR_ERR_STATE, "dithered quantiser: the matrix was not uploaded (bhr_set_dither)");
    const long long n = (long long)ctx->rows * ctx->cfg.width * 3;
    hipLaunchKernelGGL(quantize_u8_dither_kernel, dim3(grid_for(n)), dim3(kBlock), 0, ctx->stream, f.d_final, f.d_final_u8, n,
                       ctx->cfg.width, ctx->cfg.row0, ctx->d_dither);
    BHR_HIP(hipGetLastError());
    return BHR_OK;
}

extern "C" {

int32_t bhr_dither_matrix(uint16_t *out) {
    if (!out) return bhr_fail(BHR_ERR_INVALID, "bhr_dither_matrix: null argument");
    memcpy(out, kBlueNoise64, sizeof(kBlueNoise64));
    return BHR_OK;
}

int32_t bhr_set_dither(bhr_ctx *ctx, int32_t mode) {
    if (!ctx || (mode != BHR_DITHER_NONE && mode != BHR_DITHER_BLUE))
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_dither: mode %d (0 none, 1 blue)", mode);
    BHR_TRY(bhr_enter(ctx));                                       // behind the frames in flight ...
    if (mode && !ctx->d_dither) {
        BHR_HIP(hipMalloc((void **)&ctx->d_dither, sizeof(kBlueNoise64)));
        BHR_HIP(hipMemcpyAsync(ctx->d_dither, kBlueNoise64, sizeof(kBlueNoise64), hipMemcpyHostToDevice, ctx->stream));
    }
    BHR_HIP(hipStreamSynchronize(ctx->stream));                    // ... which are drained: none of them quantises under the old mode later
    if (mode == ctx->dither) return BHR_OK;
    ctx->dither = mode;
    for (auto &f : ctx->slots) f.have &= ~BHR_OUT_U8;              // the u8 rows in memory belong to the other mode
    return BHR_OK;
}

int32_t bhr_read_final_u16(bhr_ctx *ctx, uint16_t *out) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_read_final_u16: bad argument");
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_U16));
    const size_t bytes = (size_t)ctx->rows * ctx->cfg.width * 3 * sizeof(uint16_t);
    BHR_TRY(bhr_ensure_pinned(ctx, bytes));
    BHR_HIP(hipMemcpyAsync(ctx->h_pinned, bhr_slot(ctx).d_final_u16, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(out, ctx->h_pinned, bytes);
    return BHR_OK;
}

}  // extern "C"
