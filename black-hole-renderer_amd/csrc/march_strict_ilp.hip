// march_strict_ilp.hip -> march_strict_ilp.o: the strict march (ray_strict.h) under the ILP-first machine scheduler -- the
// strict texture kernels, the fix kernel of a hybrid march and the texture list kernel.
// Its two texture kernels (march_tile_plain_ilp, march_tile_aa_ilp, each with its own occupancy target):
// the plain one gains 4 % from the ILP-first schedule, the AA one 1-2 % once held to 4 waves per SIMD (unconstrained it took
// 134 VGPRs and lost 1.6 %); the fast build loses 3 % and keeps the default scheduler, as do the Disk V2 and persistent kernels.
#include "ray_strict.h"
#include "march_tile.h"

namespace {

// Second half of the hybrid march's fast list: the pixels march_tile_guard_kernel put on the fix list, 64 per wave whatever
// tile they came from, marched with the strict Ray -- bit-identical to math_mode 1.  Launched with a grid for the list's
// capacity; waves beyond the count the device holds exit at once.
// SS: the list holds whole k x k groups (march_tile_body), k^2 consecutive entries in sub-sample order, k^2-aligned; they are
// resolved like the tile's groups, with the sub-sample rows k lanes apart.
template <bool DIFF, bool SS>
__device__ __forceinline__ void march_fix_body(const BhrMarchArgs &a) {
    const int wave = wave_slot();
    unsigned int n = *a.fix_count;
    if (n > (unsigned int)a.fix_cap) n = (unsigned int)a.fix_cap;
    if ((unsigned int)wave * 64u >= n) return;
    const int lane = threadIdx.x & 63;
    const unsigned int k = (unsigned int)wave * 64u + (unsigned int)lane;
    const bool valid = k < n;
    const int pix = valid ? a.fix_list[k] : 0;
    Ray<DIFF, 0> ray;
    ray.init(a, pix % a.width, pix / a.width);
    if (!valid) ray.done = 4;
    while (ray.done == 0) {
        ray.step(a);
        if (ray.full) { ray.flush_one(a); ray.full = false; }
    }
    if (__ballot(ray.n_pend > 0)) ray.flush_one(a);
    if (__ballot(ray.n_pend > 0)) ray.flush_one(a);
    if (SS) resolve_store(a, ray, valid, valid, pix % a.width, pix / a.width, a.ss);
    else if (valid) ray.finish_at(a, pix % a.width, pix / a.width);
    // the row-cost profile (BHR_ROW_COSTS): the guard kernel left these pixels' steps out, they are strict steps of their row band
    if (a.row_steps && valid) atomicAdd(a.row_steps + (pix / a.width) / 8, (unsigned long long)ray.step_count);
    const unsigned long long tot = wave_sum_u32((unsigned int)ray.step_count);
    if (lane == 0) atomicAdd(a.ray_steps + (size_t)(blockIdx.x & (BHR_STEP_LANES - 1)) * BHR_STEP_STRIDE, tot);
}
template <bool DIFF>
__global__ __launch_bounds__(256) void march_fix_kernel(BhrMarchArgs a) { march_fix_body<DIFF, false>(a); }
template <bool DIFF>
__global__ __launch_bounds__(256) void march_fix_ss_kernel(BhrMarchArgs a) { march_fix_body<DIFF, true>(a); }

// The ILP-scheduled object launches two kernels, each with the occupancy its register allocation should aim for
// (A/B on fhd / 4k, isolated launches): plain texture march at 5 waves per SIMD (96 VGPRs, no spills; 0.697 -> 0.692 ms,
// 6 waves: 0.695), AA march at 4 (128 VGPRs; 6.50 -> 6.39 ms at 4k against the default scheduler).
// One tile per wave: the per-wave timeline (tools/wave_timeline.py) shows 88-92 % slot occupancy in the body of an fhd
// launch and a ~90 us ragged end; blocks of 64 threads (4x the workgroups) take 0.89 ms instead of 0.69, so the workgroup
// dispatcher matters -- but 2 / 3 / 4 tiles per wave do not buy it back (0.696 / 0.717 / 0.726 ms against 0.679 at one).
// A dynamic tile queue (resident waves popping tiles from a counter) was tried twice: with a data-dependent exit it compiled
// into a non-terminating loop, with a fixed trip count it ran correctly at 1.08-1.23 ms whatever the grid (each wave is
// latency-bound at ~15 cycles per instruction, so fewer, longer-lived waves only lengthen the critical path); both removed.
// (The single-trip loop is the form the two kernels were tuned in, a loop over tiles per wave: without it hipcc allocates
// their registers differently.)
template <bool DIFF, bool SS = false>
__device__ __forceinline__ void march_tile_of_wave(const BhrMarchArgs &a) {
    const int slot = wave_slot();
    for (int t = 0; t < 1; ++t)
        if (slot < a.n_list) march_tile_body<DIFF, 0, false, true, SS>(a, slot);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void march_tile_plain_ilp(BhrMarchArgs a) { march_tile_of_wave<false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void march_tile_aa_ilp(BhrMarchArgs a) { march_tile_of_wave<true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void march_tile_plain_ilp_ss(BhrMarchArgs a) { march_tile_of_wave<false, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void march_tile_aa_ilp_ss(BhrMarchArgs a) { march_tile_of_wave<true, true>(a); }

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// ss: the supersampled twin (a.ss > 1; the schedules refused with supersampling have none)
const void *bhr_march_kernel_strict_ilp(bhr_march_kernel k, int32_t diff, int32_t ss) {
    switch (k) {
    case BHR_MK_TILE_ILP:
        if (ss) return diff ? (const void *)march_tile_aa_ilp_ss : (const void *)march_tile_plain_ilp_ss;
        return diff ? (const void *)march_tile_aa_ilp : (const void *)march_tile_plain_ilp;
    case BHR_MK_FIX:
        if (ss) return diff ? (const void *)march_fix_ss_kernel<true> : (const void *)march_fix_ss_kernel<false>;
        return diff ? (const void *)march_fix_kernel<true> : (const void *)march_fix_kernel<false>;
    case BHR_MK_LIST: return diff ? (const void *)march_list_kernel<true, 0> : (const void *)march_list_kernel<false, 0>;
    default: return nullptr;
    }
}
