// march.hip -> march.o: the fast march (ray_fast.h; fast-math, see csrc/Makefile) in both schedules, and the kernels only
// the fast arithmetic has: the mip-staged march, the plain march at its own occupancy, the guard kernels of a hybrid march.
#include "ray_fast.h"
#include "march_tile.h"
#include "march_persistent.h"

namespace {

// BASELINE.json's north star asks for "mipmap levels staged through LDS".  Opt-in (BHR_MIP_LDS=1, fast arithmetic,
// anti-aliased views): every block copies the coarse levels of the packed mip stack -- as many of levels 3, 2, 1 as fit
// 44 KB -- into LDS before it marches, and _sample_disk_mip reads those levels from there.  Not the default, by
// measurement: the texture gathers are cache resident (FETCH_SIZE 0.36x the algorithmic bytes) and the kernel
// is issue bound, while 40 KB of LDS beside the parking slots leave two blocks per CU; and the BASELINE textures' level 3 (4.8 MB at 4k) does not
// fit any LDS -- the launcher falls back to the plain kernel when nothing fits.
__global__ __launch_bounds__(256) void march_tile_mipstaged_kernel(BhrMarchArgs a) {
    const int from = a.mip_lds_from;
    const int n = a.sc.mip_off[3] + a.sc.mip_h[3] * a.sc.mip_w[3] - a.sc.mip_off[from];     // levels from .. 3: the LOD is clamped to 3
    const float4 *src = a.sc.mips + a.sc.mip_off[from];
    for (int k = threadIdx.x; k < n; k += 256) g_mip_lds[k] = src[k];
    __syncthreads();
    march_tile_body<true, 3, false, false>(a, wave_slot());
}

// The plain fast march (no differentials, texture source) as an entry of its own, so that its occupancy target can be set
// without touching the other instantiations of the template: 6 waves per SIMD (80 registers per lane).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 6))) void march_tile_plain_fast(BhrMarchArgs a) {
    march_tile_body<false, 0, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6, 6))) void march_tile_plain_fast_ss(BhrMarchArgs a) {
    march_tile_body<false, 0, false, false, true>(a, wave_slot());
}

template <bool DIFF, bool COSTS = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DIFF ? 4 : 5, DIFF ? 4 : 5))) void march_tile_guard_kernel(BhrMarchArgs a) {
    march_tile_body<DIFF, 0, true, COSTS>(a, wave_slot());
}
template <bool DIFF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DIFF ? 4 : 5, DIFF ? 4 : 5))) void march_tile_guard_ss_kernel(BhrMarchArgs a) {
    march_tile_body<DIFF, 0, true, false, true>(a, wave_slot());
}

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// ss: the supersampled twin (a.ss > 1; the schedules refused with supersampling have none)
const void *bhr_march_kernel_fast(bhr_march_kernel k, int32_t diff, int32_t ss) {
    switch (k) {   // adaptive supersampling: the list kernels (a.ss > 1 always)
    case BHR_MK_LIST: return diff ? (const void *)march_list_kernel<true, 0> : (const void *)march_list_kernel<false, 0>;
    case BHR_MK_LIST_VOLUME: return (const void *)march_list_kernel<false, 2>;
    case BHR_MK_LIST_DV2: return diff ? (const void *)march_list_kernel<true, 1> : (const void *)march_list_kernel<false, 1>;
    default: break;
    }
    if (ss) {
        switch (k) {
        case BHR_MK_VOLUME: return (const void *)march_tile_ss_kernel<false, 2>;
        case BHR_MK_DV2: return diff ? (const void *)march_tile_ss_kernel<true, 1> : (const void *)march_tile_ss_kernel<false, 1>;
        case BHR_MK_TILE: return diff ? (const void *)march_tile_ss_kernel<true, 0> : (const void *)march_tile_plain_fast_ss;
        case BHR_MK_GUARD: return diff ? (const void *)march_tile_guard_ss_kernel<true> : (const void *)march_tile_guard_ss_kernel<false>;
        default: return nullptr;
        }
    }
    switch (k) {
    case BHR_MK_VOLUME: return (const void *)march_tile_kernel<false, 2>;
    case BHR_MK_DV2: return diff ? (const void *)march_tile_kernel<true, 1> : (const void *)march_tile_kernel<false, 1>;
    case BHR_MK_PERSISTENT: return diff ? (const void *)march_persistent_kernel<true> : (const void *)march_persistent_kernel<false>;
    case BHR_MK_TILE: return diff ? (const void *)march_tile_kernel<true, 0> : (const void *)march_tile_plain_fast;
    case BHR_MK_TILE_COSTS: return diff ? (const void *)march_tile_kernel<true, 0, true> : (const void *)march_tile_kernel<false, 0, true>;
    case BHR_MK_GUARD: return diff ? (const void *)march_tile_guard_kernel<true> : (const void *)march_tile_guard_kernel<false>;
    case BHR_MK_GUARD_COSTS: return diff ? (const void *)march_tile_guard_kernel<true, true> : (const void *)march_tile_guard_kernel<false, true>;
    case BHR_MK_MIPSTAGED: return diff ? (const void *)march_tile_mipstaged_kernel : nullptr;
    default: return nullptr;
    }
}
