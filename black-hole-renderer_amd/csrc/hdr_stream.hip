// hdr_stream.hip -- the HDR video stream's conversion (include/bhr_output.h: bhr_y4m_open_hdr): the frame slot's scene-linear
// HDR plane -> 10-bit BT.2020 Y'CbCr 4:2:0 under a PQ (ST 2084) or HLG (BT.2100) transfer, and the frame's light levels.
//
// Per pixel, all in f32, every operation rounded once (the object is compiled without contraction and without fast-math; exp2f,
// log2f, logf and sqrtf are the device library's):
//   v       = h * gain                                    gain = (float)exp2((double)exposure_stops), from the host
//   (R,G,B) = M . v, each row ((m0 r + m1 g) + m2 b)      BT.709 -> BT.2020 (BT.2087)
//   PQ      Y  = fminf(X * scale, 1)                      scale = white_nits / 10000, from the host
//           E' = ((c1 + c2 p) / (1 + c3 p))^m2            p = Y^m1; x^e is exp2f(e * log2f(x))
//   HLG     E  = fminf(X * 0.265f, 1)
//           E' = E <= 1/12 ? sqrtf(3 E) : a logf(12 E - b) + c
//   Y'  = (0.2627f R' + 0.6780f G') + 0.0593f B'          DY = clamp((int)floorf(876 Y' + 64.5f), 64, 940)
//   chroma of a 2x2 block from the mean R'G'B' ((a + b) + (c + d)) * 0.25f (a, b the upper row) and that mean's own Y':
//   Cb = (B' - Y') / 1.8814f, Cr = (R' - Y') / 1.4746f    DC = clamp((int)floorf(896 C + 512.5f), 64, 960)
// tests/hdr_ref.py restates all of it in NumPy.  Dither does not apply to this stream: it is quantised from these floats, never
// from the context's u8 rows, and a half-code offset is its only rounding.
//
// One thread per 2x2 block, 32 x 8 threads per workgroup, like the 8-bit stream's kernel.  The traffic is small: 12 bytes read
// and 3 written per pixel.  A thread's share of a row is two pixels = six floats = 24 bytes, 8-byte aligned for every even
// width, so it is read as three float2 loads (the compiler fuses them into a 16-byte and an 8-byte load): the lanes of a wave's
// row cover 32 x 24 contiguous bytes, every byte of every cache line they touch is used, and none is fetched twice.  The two
// luma samples of a row leave as one 4-byte store per lane (consecutive lanes, consecutive words), the chroma samples as 2-byte
// stores.  No LDS, no scratch.
//
// Light levels (PQ): per pixel nits = fminf(white_nits * max(R, G, B), 10000).  A lane sums its four pixels in binary64; a wave
// reduces the largest value and the sum with lane shuffles and issues one atomic for each: the maximum on the f32's bit pattern
// (the values are >= 0, so unsigned order is numeric order), the sum in binary64, whose result depends on the order of the waves
// far below 1e-9 relative.  Lanes outside the frame take part with zeros.  These atomics are what the PQ kernel costs: the 8160
// waves of an fhd frame meet on ONE pair of addresses and serialise in L2 -- 0.21 ms alone on the device against the HLG kernel's
// 0.016 ms, with powf or with exp2f / log2f alike.  Spreading them over many pairs of cells that the host folds, as the march's
// ray-step counters are spread (bhr_internal.h), is the known remedy and the next step; it has not run on the device yet.
#include "bhr_internal.h"
#include "../../include/bhr_output.h"

namespace {

struct Rgb { float r, g, b; };

// x^e for 0 <= x <= 1 and e > 0 as exp2f(e * log2f(x)): 0 -> exp2f(-inf) = 0.  The product's rounding is the error that counts:
// relative 2^-24 |e log2 x| on the power, which is at most 1.5e-6 on Y^m1 and, times E' itself, 2e-8 on E' -- far below the
// 1.1e-3 of a luma code.  The device library's powf carries the logarithm in extended precision to avoid just that, at about
// a thousand instructions per pixel; on the GPU tests both versions left the same share of samples one code off.
__device__ __forceinline__ float pow_unit(float x, float e) {
#pragma clang fp contract(off)
    return exp2f(e * log2f(x));
}

__device__ __forceinline__ float pq_oetf(float x, float scale) {
#pragma clang fp contract(off)
    const float y = fminf(x * scale, 1.0f);
    const float p = pow_unit(y, 2610.0f / 16384.0f);
    return pow_unit((3424.0f / 4096.0f + (2413.0f / 4096.0f * 32.0f) * p) / (1.0f + (2392.0f / 4096.0f * 32.0f) * p), 2523.0f / 4096.0f * 128.0f);
}

__device__ __forceinline__ float hlg_oetf(float x) {
#pragma clang fp contract(off)
    const float e = fminf(x * 0.265f, 1.0f);
    return e <= 1.0f / 12.0f ? sqrtf(3.0f * e) : 0.17883277f * logf(12.0f * e - 0.28466892f) + 0.55991073f;
}

__device__ __forceinline__ float luma2020(const Rgb &c) {
#pragma clang fp contract(off)
    return (0.2627f * c.r + 0.6780f * c.g) + 0.0593f * c.b;
}

__device__ __forceinline__ uint32_t code_y(float y) { return (uint32_t)min(max((int)floorf(876.0f * y + 64.5f), 64), 940); }
__device__ __forceinline__ uint16_t code_c(float c) { return (uint16_t)min(max((int)floorf(896.0f * c + 512.5f), 64), 960); }

// one pixel: scene-linear BT.709 h -> non-linear BT.2020 R'G'B'; *peak = max(R, G, B) of the linear BT.2020 value
template <int TRANSFER>
__device__ __forceinline__ Rgb encode_pixel(float hr, float hg, float hb, float gain, float scale, float *peak) {
#pragma clang fp contract(off)
    const float r = hr * gain, g = hg * gain, b = hb * gain;
    const float R = (0.6274f * r + 0.3293f * g) + 0.0433f * b;
    const float G = (0.0691f * r + 0.9195f * g) + 0.0114f * b;
    const float B = (0.0164f * r + 0.0880f * g) + 0.8956f * b;
    *peak = fmaxf(fmaxf(R, G), B);
    Rgb e;
    if (TRANSFER == BHR_HDR_PQ) { e.r = pq_oetf(R, scale); e.g = pq_oetf(G, scale); e.b = pq_oetf(B, scale); }
    else { e.r = hlg_oetf(R); e.g = hlg_oetf(G); e.b = hlg_oetf(B); }
    return e;
}

// hdr: (h, w, 3) f32; out: Y (h w) | Cb (h w / 4) | Cr, u16.  w and h even; both planes start on 8-byte boundaries.
template <int TRANSFER>
__global__ __launch_bounds__(256) void hdr_to_yuv420p10_kernel(const float *__restrict__ hdr, uint16_t *__restrict__ out, int w, int h, float gain,
                                                               float scale, float white_nits, unsigned int *__restrict__ lv_max,
                                                               double *__restrict__ lv_sum) {
#pragma clang fp contract(off)
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y * blockDim.y + threadIdx.y;
    const int cw = w >> 1, ch = h >> 1;
    float top = 0.0f;       // the lane's largest nits
    double sum = 0.0;       // and their sum
    if (bx < cw && by < ch) {
        uint16_t *Y = out, *U = out + (size_t)w * h, *V = U + (size_t)cw * ch;
        Rgb e[2][2];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const size_t at = (size_t)(2 * by + dy) * w + 2 * bx;                 // the row's first pixel of this block
            const float2 *p = reinterpret_cast<const float2 *>(hdr + at * 3);
            const float2 a = p[0], b = p[1], c = p[2];                            // r0 g0 | b0 r1 | g1 b1
            float peak0, peak1;
            e[dy][0] = encode_pixel<TRANSFER>(a.x, a.y, b.x, gain, scale, &peak0);
            e[dy][1] = encode_pixel<TRANSFER>(b.y, c.x, c.y, gain, scale, &peak1);
            *reinterpret_cast<uint32_t *>(Y + at) = code_y(luma2020(e[dy][0])) | (code_y(luma2020(e[dy][1])) << 16);   // little endian
            if (TRANSFER == BHR_HDR_PQ) {
                const float n0 = fminf(white_nits * peak0, 10000.0f), n1 = fminf(white_nits * peak1, 10000.0f);
                top = fmaxf(top, fmaxf(n0, n1));
                sum += (double)n0;
                sum += (double)n1;
            }
        }
        Rgb m;
        m.r = ((e[0][0].r + e[0][1].r) + (e[1][0].r + e[1][1].r)) * 0.25f;
        m.g = ((e[0][0].g + e[0][1].g) + (e[1][0].g + e[1][1].g)) * 0.25f;
        m.b = ((e[0][0].b + e[0][1].b) + (e[1][0].b + e[1][1].b)) * 0.25f;
        const float ym = luma2020(m);
        U[(size_t)by * cw + bx] = code_c((m.b - ym) / 1.8814f);
        V[(size_t)by * cw + bx] = code_c((m.r - ym) / 1.4746f);
    }
    if (TRANSFER == BHR_HDR_PQ) {
        // every lane of the workgroup is here (no early return): 256 threads are four whole waves
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            top = fmaxf(top, __shfl_xor(top, d, 64));
            sum += __shfl_xor(sum, d, 64);
        }
        if (((threadIdx.y * blockDim.x + threadIdx.x) & 63) == 0) {
            atomicMax(lv_max, __float_as_uint(top));
            atomicAdd(lv_sum, sum);
        }
    }
}

}  // namespace

int32_t bhr_launch_hdr_yuv420p10(bhr_ctx *ctx, int32_t transfer, float gain, float scale, float white_nits, uint16_t *d_out, void *d_levels) {
    const bhr_frame_slot &f = bhr_slot(ctx);
    if (!(f.have & BHR_OUT_HDR) || !f.d_hdr)
        return bhr_fail(BHR_ERR_STATE, "bhr_y4m_submit: the frame kept no HDR plane (bhr_set_grade with keep_hdr, then render or bhr_grade_frame)");
    const int w = ctx->cfg.width, h = ctx->rows;
    if ((w & 1) || (h & 1) || w < 2 || h < 2) return bhr_fail(BHR_ERR_INVALID, "bhr_y4m_submit: 4:2:0 needs even width and height, got %dx%d", w, h);
    BHR_HIP(hipMemsetAsync(d_levels, 0, 16, ctx->stream));
    unsigned int *lv_max = static_cast<unsigned int *>(d_levels);
    double *lv_sum = reinterpret_cast<double *>(static_cast<unsigned char *>(d_levels) + 8);
    const dim3 block(32, 8), grid(((w >> 1) + 31) / 32, ((h >> 1) + 7) / 8);
    if (transfer == BHR_HDR_PQ)
        hipLaunchKernelGGL(hdr_to_yuv420p10_kernel<BHR_HDR_PQ>, grid, block, 0, ctx->stream, f.d_hdr, d_out, w, h, gain, scale, white_nits, lv_max, lv_sum);
    else
        hipLaunchKernelGGL(hdr_to_yuv420p10_kernel<BHR_HDR_HLG>, grid, block, 0, ctx->stream, f.d_hdr, d_out, w, h, gain, scale, white_nits, lv_max, lv_sum);
    BHR_HIP(hipGetLastError());
    return BHR_OK;
}
