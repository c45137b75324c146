// march_observer.hip -> march_observer.o: the strict march seen by a moving camera (ray_observer.h; bhr_render_observer) in the
// tile schedule, one ray per pixel and the supersampled twin.  Built with the strict objects' flags (csrc/Makefile).
#include "ray_observer.h"
#include "march_tile.h"

namespace {

// march_tile_kernel<false, 0> and march_tile_ss_kernel<false, 0> (march_tile.h) over the observer Ray, with the observer's block
// as their argument, at the occupancy target of the strict plain kernel (march_strict_ilp.hip: 5 waves per SIMD, 96 VGPRs, no
// spills -- the observer's D is one more value across the loop and still fits)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void march_observer_kernel(BhrObserverMarchArgs a) {
    march_tile_body<false, 0, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void march_observer_ss_kernel(BhrObserverMarchArgs a) {
    march_tile_body<false, 0, false, false, true>(a, wave_slot());
}

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// The observer march has the texture source and no differentials: BHR_MK_TILE with diff = 0 is all there is.
const void *bhr_march_kernel_observer(bhr_march_kernel k, int32_t diff, int32_t ss) {
    if (diff || k != BHR_MK_TILE) return nullptr;
    return ss ? (const void *)march_observer_ss_kernel : (const void *)march_observer_kernel;
}
