// march_kerr_line.hip -> march_kerr_line.o: the Kerr line profile's kernel (bhr_set_kerr_line; include/bhr.h states the model,
// DESIGN 4 "Kerr line profile" derives it), in an object of its own with exactly the flags of march_kerr_polar.o, for that
// object's reason: kerr_sample_disk and the g-factors are inlined here to the bits they have in the Kerr map's shade kernel, so the
// opacity and the transmittance this kernel weighs a record by are the frame's own.
//
// kerr_line_kernel<RS, TEX> runs behind the shade, overflow and Stokes launches of a frame from the k = 1 Kerr ray map with
// kerr_raymap_stokes_kernel's mapping -- a lane per pixel, an 8x8 tile per wave, tiles row-major -- and walks the lane's records
// front to back.  Per counted record it takes g (kerr_g_exact on words 2..4 of the record under the exact redshift, kerr_g_model
// under the model: no momentum build in either mode), the emissivity, the pixel's solid angle and the transmittance, and adds the
// integer Q = llrintf(w * unit) to the cell of g's bin.
//
// Template parameters and runtime branches.  RS (the redshift) picks the Kerr block and the g-factor; TEX (the emissivity) pulls in
// the disk sampler, its powf and the transmittance, ~40 registers the power law does not need: both are instantiations.  The orders
// (s.all) and the sample planes (s.g_out) are wave-uniform words of the argument block: scalar branches, nothing per lane.
//
// The histogram.  A workgroup keeps n_bins + 4 u64 cells in dynamic LDS, adds to them with LDS atomics and, at its end, adds every
// non-zero cell to the frame's device row with one global u64 atomic.  The grid is capped (march_launch.hip) and the workgroups
// stride over the tiles, so clearing and flushing the cells is paid once per workgroup and not once per four tiles.  All adds are
// integer adds, which commute: the row is a function of the samples alone, whatever the order of the atomics.  No float atomic.
// Q <= 2^32 (w <= 1.5^p, unit = 2^32 / 1.5^p), so 8 records of a 7680 x 4320 frame sum to less than 2^3 2^25 2^32 = 2^60.
//
// kerr_sample_disk, kerr_g_exact and pixel_ray are called, not edited: no other object's code moves.
#include <type_traits>

#include "ray_kerr.h"

namespace {

template <int RS>
using KerrBlock = std::conditional_t<RS == KERR_EXACT, BhrKerrExactMarchArgs, BhrKerrMarchArgs>;

template <int RS, bool TEX>
__global__ __launch_bounds__(256) void kerr_line_kernel(KerrBlock<RS> a, BhrRayMapArgs m, BhrKerrLineArgs s) {
    extern __shared__ unsigned long long cells[];    // n_bins, then under, over, samples, overflow pixels
    const int n_cells = s.n_bins + 4;
    for (int b = threadIdx.x; b < n_cells; b += 256) cells[b] = 0ull;
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t p = (size_t)m.plane;
    const float ka = kerr(a).kerr_a;
    const V3 fwd = ld3(a.cf);
    const bool keep = s.g_out != nullptr;
    for (int tile = blockIdx.x * 4 + wave; tile < a.n_tiles; tile += (int)gridDim.x * 4) {
        const int i = (tile % a.tiles_x) * 8 + (lane & 7);
        const int j = (tile / a.tiles_x) * 8 + (lane >> 3);
        if (!(i < a.width && j < a.rows)) continue;
        const size_t pix = (size_t)j * a.width + i;
        const int count = m.crossings[pix];
        const bool listed = count > m.slots;          // a pixel on the overflow list contributes nothing
        if (listed) atomicAdd(&cells[s.n_bins + 3], 1ull);
        // the pinhole pixel's solid angle relative to the central pixel's
        V3 unused_x, unused_y;
        const V3 D = pixel_ray<false>(a, i, j, unused_x, unused_y);
        const float ct = dot(D, fwd);
        const float domega = (ct * ct) * ct;
        float alpha_total = 0.0f;                     // as Ray::init leaves it
        bool first_done = false;
        // with the planes every slot is written; without, only the pixel's own records are walked
        const int n = keep ? m.slots : (listed ? 0 : count);
        for (int c = 0; c < n; ++c) {
            float g = 0.0f, w = 0.0f;
            if (c < count && !listed && !(first_done && !keep)) {
                const float *q = m.hits + (size_t)c * m.comps * p + pix;
                const float hx = q[0], hy = q[p];
                const float r = sqrtf(hx * hx + hy * hy - ka * ka);
                // kerr_shade_hit's own test: outside the disk's annulus the frame composites nothing
                if (a.r_outer >= r && r >= a.r_inner && !first_done) {
                    float disk_alpha = 1.0f;
                    if (TEX) {
                        const float4 rgba = kerr_sample_disk(a, hx, hy, r);
                        const float base_alpha = fminf(rgba.w, 0.999f);
                        disk_alpha = 1.0f - powf(1.0f - base_alpha, BHR_DISK_ALPHA_GAIN);
                    }
                    if (s.r_out >= r && r >= s.r_in) {
                        const V3 v = mk(q[2 * p], q[3 * p], q[4 * p]);
                        if (RS == KERR_EXACT) g = kerr_g_exact(a, hx, hy, r, v);
                        else g = kerr_g_model(a, a, hx, hy, r, v);
                        float eps = powf(r / s.r_in, -s.index);
                        if (TEX) eps = eps * disk_alpha;
                        w = (powf(g, s.power) * eps) * domega;
                        if (TEX && s.all) w = w * (1.0f - alpha_total);
                        const float t = (g - s.g_min) * s.scale;
                        int cell = s.n_bins;                       // under: below the range, or no number
                        if (t >= 0.0f) {
                            const float fl = floorf(t);
                            cell = fl < (float)s.n_bins ? (int)fl : s.n_bins + 1;
                        }
                        const unsigned long long Q = (unsigned long long)llrintf(w * s.unit);
                        atomicAdd(&cells[cell], Q);
                        atomicAdd(&cells[s.n_bins + 2], 1ull);
                        if (!s.all) first_done = true;
                    }
                    if (TEX) {
                        const float front = 1.0f - alpha_total;
                        alpha_total = 1.0f - front * (1.0f - disk_alpha);
                    }
                }
            }
            if (keep) {
                s.g_out[(size_t)c * p + pix] = g;
                s.w_out[(size_t)c * p + pix] = w;
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_cells; b += 256) {
        const unsigned long long v = cells[b];
        if (v) atomicAdd(&s.row[b], v);
    }
}

}  // namespace

const void *bhr_kerr_line_kernel(int32_t exact, int32_t texture) {
    if (exact) return texture ? (const void *)kerr_line_kernel<KERR_EXACT, true> : (const void *)kerr_line_kernel<KERR_EXACT, false>;
    return texture ? (const void *)kerr_line_kernel<0, true> : (const void *)kerr_line_kernel<0, false>;
}
