// march_kerr.hip -> march_kerr.o: the march around a spinning hole (ray_kerr.h) in the tile schedule, one ray per pixel and
// the supersampled twin.  Built with FMA contraction and without fast-math (csrc/Makefile says why).
#include "ray_kerr.h"
#include "march_tile.h"

namespace {

// march_tile_kernel<false, 0> and march_tile_ss_kernel<false, 0> (march_tile.h) over the Kerr Ray, with the Kerr block as their argument
__global__ __launch_bounds__(256) void march_kerr_kernel(BhrKerrMarchArgs a) {
    march_tile_body<false, 0, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256) void march_kerr_ss_kernel(BhrKerrMarchArgs a) {
    march_tile_body<false, 0, false, false, true>(a, wave_slot());
}

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// The Kerr march has the texture source and no differentials: BHR_MK_TILE with diff = 0 is all there is.
const void *bhr_march_kernel_kerr(bhr_march_kernel k, int32_t diff, int32_t ss) {
    if (k != BHR_MK_TILE || diff) return nullptr;
    return ss ? (const void *)march_kerr_ss_kernel : (const void *)march_kerr_kernel;
}
