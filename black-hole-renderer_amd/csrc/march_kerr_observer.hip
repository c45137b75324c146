// march_kerr_observer.hip -> march_kerr_observer.o: the Kerr march seen by a camera that may move and may be panoramic
// (ray_kerr_observer.h; bhr_render_kerr_view) in the tile schedule, one ray per pixel and the supersampled twin, each with the
// model redshift and with the exact one.  Built with exactly the Kerr object's flags (csrc/Makefile says why).
#include "ray_kerr_observer.h"
#include "march_tile.h"

namespace {

// march_kerr.hip's four kernels over the Kerr camera's Ray, with the camera's block as their argument
__global__ __launch_bounds__(256) void march_kerr_view_kernel(BhrKerrViewMarchArgs a) {
    march_tile_body<false, 0, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256) void march_kerr_view_ss_kernel(BhrKerrViewMarchArgs a) {
    march_tile_body<false, 0, false, false, true>(a, wave_slot());
}
__global__ __launch_bounds__(256) void march_kerr_view_exact_kernel(BhrKerrViewMarchArgs a) {
    march_tile_body<false, KERR_EXACT, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256) void march_kerr_view_exact_ss_kernel(BhrKerrViewMarchArgs a) {
    march_tile_body<false, KERR_EXACT, false, false, true>(a, wave_slot());
}

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// Like the Kerr march: BHR_MK_TILE (the model redshift) and BHR_MK_KERR_EXACT with diff = 0 are all there is.
const void *bhr_march_kernel_kerr_view(bhr_march_kernel k, int32_t diff, int32_t ss) {
    if (diff) return nullptr;
    if (k == BHR_MK_TILE) return ss ? (const void *)march_kerr_view_ss_kernel : (const void *)march_kerr_view_kernel;
    if (k == BHR_MK_KERR_EXACT) return ss ? (const void *)march_kerr_view_exact_ss_kernel : (const void *)march_kerr_view_exact_kernel;
    return nullptr;
}
