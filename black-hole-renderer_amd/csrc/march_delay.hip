// march_delay.hip -> march_delay.o: the strict march with light delay (ray_delay.h; bhr_render_delayed) in the tile schedule, one
// ray per pixel and the supersampled twin.  Built with the strict objects' flags (csrc/Makefile).
#include "ray_delay.h"
#include "march_tile.h"

namespace {

// march_tile_kernel<false, 0> and march_tile_ss_kernel<false, 0> (march_tile.h) over the delayed Ray, with the delay's block as
// their argument.  The Ray keeps T, E and w across the loop and both ends of a step until its quadrature is done; the occupancy
// target is the one at which that fits without scratch (DESIGN.md "Light delay").
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void march_delay_kernel(BhrDelayMarchArgs a) {
    march_tile_body<false, 0, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void march_delay_ss_kernel(BhrDelayMarchArgs a) {
    march_tile_body<false, 0, false, false, true>(a, wave_slot());
}

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// The delayed march has the texture source and no differentials: BHR_MK_TILE with diff = 0 is all there is.
const void *bhr_march_kernel_delay(bhr_march_kernel k, int32_t diff, int32_t ss) {
    if (diff || k != BHR_MK_TILE) return nullptr;
    return ss ? (const void *)march_delay_ss_kernel : (const void *)march_delay_kernel;
}
