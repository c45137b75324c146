// march_kerr.hip -> march_kerr.o: the march around a spinning hole (ray_kerr.h) in the tile schedule, one ray per pixel and
// the supersampled twin, each with the model redshift and with the exact one (bhr_set_redshift), and each of the four once more
// over the Kerr Ray with differentials (bhr_set_kerr_anti_alias).  Built with FMA contraction and without fast-math (csrc/Makefile says why).
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
// the same two over the Kerr Ray of the exact redshift, with the ISCO's numbers behind the Kerr block
__global__ __launch_bounds__(256) void march_kerr_exact_kernel(BhrKerrExactMarchArgs a) {
    march_tile_body<false, KERR_EXACT, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256) void march_kerr_exact_ss_kernel(BhrKerrExactMarchArgs a) {
    march_tile_body<false, KERR_EXACT, false, false, true>(a, wave_slot());
}
// the four over the Kerr Ray with ray differentials: the disk texture at the mip level of each crossing's footprint
__global__ __launch_bounds__(256, 3) void march_kerr_aa_kernel(BhrKerrMarchArgs a) {
    march_tile_body<true, 0, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256, 3) void march_kerr_aa_ss_kernel(BhrKerrMarchArgs a) {
    march_tile_body<true, 0, false, false, true>(a, wave_slot());
}
__global__ __launch_bounds__(256) void march_kerr_exact_aa_kernel(BhrKerrExactMarchArgs a) {
    march_tile_body<true, KERR_EXACT, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256) void march_kerr_exact_aa_ss_kernel(BhrKerrExactMarchArgs a) {
    march_tile_body<true, KERR_EXACT, false, false, true>(a, wave_slot());
}

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// The Kerr march has the texture source: BHR_MK_TILE (the model redshift) and BHR_MK_KERR_EXACT, each without and with
// differentials, are all there is.
const void *bhr_march_kernel_kerr(bhr_march_kernel k, int32_t diff, int32_t ss) {
    if (k == BHR_MK_TILE) {
        if (diff) return ss ? (const void *)march_kerr_aa_ss_kernel : (const void *)march_kerr_aa_kernel;
        return ss ? (const void *)march_kerr_ss_kernel : (const void *)march_kerr_kernel;
    }
    if (k == BHR_MK_KERR_EXACT) {
        if (diff) return ss ? (const void *)march_kerr_exact_aa_ss_kernel : (const void *)march_kerr_exact_aa_kernel;
        return ss ? (const void *)march_kerr_exact_ss_kernel : (const void *)march_kerr_exact_kernel;
    }
    return nullptr;
}
