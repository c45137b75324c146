// march_projected.hip -> march_projected.o: the observer's march under an equirectangular or fisheye projection (ray_projected.h;
// bhr_render_projected) in the tile schedule, one ray per pixel and the supersampled twin.  Built with the strict objects' flags
// (csrc/Makefile).
#include "ray_projected.h"
#include "march_tile.h"

namespace {

// march_tile_kernel<false, 0> and march_tile_ss_kernel<false, 0> (march_tile.h) over the projected Ray, with the projection's block
// as their argument, at the occupancy target of the observer's kernels (march_observer.hip: 5 waves per SIMD) -- the projection
// is worked out ahead of the loop and leaves nothing alive across it
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void march_projected_kernel(BhrProjectedMarchArgs a) {
    march_tile_body<false, 0, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void march_projected_ss_kernel(BhrProjectedMarchArgs a) {
    march_tile_body<false, 0, false, false, true>(a, wave_slot());
}

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// The projected march has the texture source and no differentials: BHR_MK_TILE with diff = 0 is all there is.
const void *bhr_march_kernel_projected(bhr_march_kernel k, int32_t diff, int32_t ss) {
    if (diff || k != BHR_MK_TILE) return nullptr;
    return ss ? (const void *)march_projected_ss_kernel : (const void *)march_projected_kernel;
}
