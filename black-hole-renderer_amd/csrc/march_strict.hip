// march_strict.hip -> march_strict.o: the strict march (ray_strict.h; -ffp-contract=off, no fast-math) in both schedules
// for every disk source, the detect kernel of adaptive supersampling and the self-test of the exact arithmetic.
#include "ray_strict.h"
#include "march_tile.h"
#include "march_persistent.h"

namespace {

// ---- adaptive supersampling (bhr_set_adaptive_supersample): which output pixels get k x k rays ---------------------------
// c(p) = the largest |L[p] - L[n]| over the edge neighbours n of p inside the frame, both layers L of the k = 1 frame and the
// three channels (each difference one f32 subtraction); p is refined iff c(p) > T.  One wave per 8 x 8 block of output pixels.
// It writes the mask (one byte per output pixel) and lists the 8 x 8 tiles of the FINE frame that hold a refined pixel -- k
// divides 8, so a block is (k x k) whole fine tiles of (8 / k) x (8 / k) output pixels each; the lane of a tile's first pixel
// lists it -- wave-aggregated: one atomicAdd per wave and list.  Under hybrid a tile goes to the strict list (list, counts[0])
// or the fast one (list + cap, counts[1]) by its flag; otherwise everything goes to the first.  counts[2], [3]: refined pixels
// in tiles of the first / second list.  Each list has room for every fine tile.  Built without fast-math: T may be +inf.
__global__ __launch_bounds__(256) void adaptive_detect_kernel(BhrDetectArgs d) {
    const int lane = threadIdx.x & 63;
    const int wave = wave_slot();
    const int bx_n = (d.width + 7) / 8;
    const int bx = wave % bx_n, by = wave / bx_n;
    const int i = bx * 8 + (lane & 7), j = by * 8 + (lane >> 3);
    const bool valid = i < d.width && j < d.height;
    float c = 0.0f;
    if (valid) {
        const size_t o = ((size_t)j * d.width + i) * 3;
        const int di[4] = {-1, 1, 0, 0}, dj[4] = {0, 0, -1, 1};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ni = i + di[q], nj = j + dj[q];
            if (ni < 0 || ni >= d.width || nj < 0 || nj >= d.height) continue;
            const size_t m = ((size_t)nj * d.width + ni) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                c = fmaxf(c, fabsf(__fsub_rn(d.bg[o + ch], d.bg[m + ch])));
                c = fmaxf(c, fabsf(__fsub_rn(d.disk[o + ch], d.disk[m + ch])));
            }
        }
    }
    const bool refine = valid && c > d.threshold;
    if (valid) d.mask[(size_t)j * d.width + i] = refine ? 1 : 0;
    // the lane's fine tile: s x s output pixels, s = 8 / k; its lanes inside the wave
    const int s_log2 = 3 - d.k_log2, s = 1 << s_log2;
    const int lx = (lane & 7) & ~(s - 1), ly = (lane >> 3) & ~(s - 1);
    const unsigned long long row = ((1ull << s) - 1ull) << lx;
    unsigned long long tile_lanes = 0;
    for (int r = 0; r < s; ++r) tile_lanes |= row << ((ly + r) * 8);
    const unsigned long long mr = __ballot(refine);
    const int n_ref = __popcll(mr & tile_lanes);                       // refined pixels of the lane's tile
    const bool lead = valid && (lane & 7) == lx && (lane >> 3) == ly && n_ref > 0;
    const int tile = ((j << d.k_log2) >> 3) * d.fine_tiles_x + ((i << d.k_log2) >> 3);
    bool second = false;
    if (d.flags && lead) second = d.flags[tile] == 0;
    const unsigned long long m0 = __ballot(lead && !second), m1 = __ballot(lead && second);
    const unsigned long long below = (1ull << lane) - 1ull;
    // refined pixels per list: the leaders' counts, summed over the wave
    int p0 = lead && !second ? n_ref : 0, p1 = lead && second ? n_ref : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { p0 += __shfl_xor(p0, off, BHR_WAVE); p1 += __shfl_xor(p1, off, BHR_WAVE); }
    unsigned int base0 = 0, base1 = 0;
    if (lane == 0 && m0) { base0 = atomicAdd(d.counts + 0, (unsigned int)__popcll(m0)); atomicAdd(d.counts + 2, (unsigned int)p0); }
    if (lane == 0 && m1) { base1 = atomicAdd(d.counts + 1, (unsigned int)__popcll(m1)); atomicAdd(d.counts + 3, (unsigned int)p1); }
    base0 = __shfl(base0, 0, BHR_WAVE);
    base1 = __shfl(base1, 0, BHR_WAVE);
    if (lead) {
        const unsigned int at = second ? base1 + (unsigned int)__popcll(m1 & below) : base0 + (unsigned int)__popcll(m0 & below);
        if (at < (unsigned int)d.cap) d.list[(second ? (size_t)d.cap : 0) + at] = tile;
    }
}

// ---- self-test of the hand-written exact arithmetic against hipcc's IEEE sequences ----------
__device__ __forceinline__ unsigned int lcg(unsigned int &s) { s = s * 1664525u + 1013904223u; return s; }
__global__ void selftest_kernel(unsigned long long *out, unsigned int div_rounds) {
    const unsigned int tid = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;
    unsigned long long bad_sqrt = 0, bad_div = 0, bad_div6 = 0, n = 0;
    // every f32 in [2^-80, 2^80): exponent field 47..206, all significands
    for (unsigned long long k = tid; k < 160ull << 23; k += nthreads) {
        float x = __uint_as_float((unsigned int)(k + (47ull << 23)));
        bad_sqrt += sqrt_rn(x) != sqrtf(x);
        bad_div += rcp_rn(x) != 1.0f / x;
        bad_div += rcp_rn(-x) != 1.0f / -x;
        bad_div6 += div6(x) != x / 6.0f;
        bad_div6 += div6(-x) != -x / 6.0f;
        n += 5;
    }
    // random pairs: a, b with exponents in [2^-24, 2^24), random significands and signs
    unsigned int st = tid * 2654435761u + 12345u;
    for (unsigned int k = 0; k < div_rounds; ++k) {
        unsigned int ra = lcg(st), rb = lcg(st), re = lcg(st);
        unsigned int ea = 103u + (re & 0xffffu) % 48u, eb = 103u + (re >> 16) % 48u;
        float a = __uint_as_float((ra & 0x807fffffu) | (ea << 23));
        float b = __uint_as_float((rb & 0x807fffffu) | (eb << 23));
        bad_div += div_rn(a, b) != a / b;
        bad_div += div_rn(1.0f, b) != 1.0f / b;
        n += 2;
    }
    atomicAdd(out + 0, bad_sqrt);
    atomicAdd(out + 1, bad_div);
    atomicAdd(out + 2, bad_div6);
    atomicAdd(out + 3, n);
}

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// ss: the supersampled twin (a.ss > 1; the schedules refused with supersampling have none)
const void *bhr_march_kernel_strict(bhr_march_kernel k, int32_t diff, int32_t ss) {
    switch (k) {   // adaptive supersampling: the detect kernel and the list kernels of the Disk V2 sources (a.ss > 1 always)
    case BHR_MK_DETECT: return (const void *)adaptive_detect_kernel;
    case BHR_MK_LIST_VOLUME: return (const void *)march_list_kernel<false, 2>;
    case BHR_MK_LIST_DV2: return diff ? (const void *)march_list_kernel<true, 1> : (const void *)march_list_kernel<false, 1>;
    default: break;
    }
    if (ss) {
        switch (k) {
        case BHR_MK_VOLUME: return (const void *)march_tile_ss_kernel<false, 2>;
        case BHR_MK_DV2: return diff ? (const void *)march_tile_ss_kernel<true, 1> : (const void *)march_tile_ss_kernel<false, 1>;
        default: return nullptr;
        }
    }
    switch (k) {
    case BHR_MK_VOLUME: return (const void *)march_tile_kernel<false, 2>;
    case BHR_MK_DV2: return diff ? (const void *)march_tile_kernel<true, 1> : (const void *)march_tile_kernel<false, 1>;
    case BHR_MK_PERSISTENT: return diff ? (const void *)march_persistent_kernel<true> : (const void *)march_persistent_kernel<false>;
    case BHR_MK_TILE: return diff ? (const void *)march_tile_kernel<true, 0> : (const void *)march_tile_kernel<false, 0>;
    default: return nullptr;
    }
}

int32_t bhr_selftest_strict(bhr_ctx *ctx, unsigned long long *d_out4) {
    BHR_HIP(hipMemsetAsync(d_out4, 0, 4 * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(selftest_kernel, dim3(2048), dim3(256), 0, ctx->stream, d_out4, 2048u);
    BHR_HIP(hipGetLastError());
    return BHR_OK;
}
