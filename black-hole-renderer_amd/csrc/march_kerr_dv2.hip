// march_kerr_dv2.hip -> march_kerr_dv2.o: the march around a spinning hole over the analytic Disk V2 sources (ray_kerr_dv2.h;
// bhr_set_kerr_disk_source) in the tile schedule: the surface with the model redshift and with the exact one, and the volume with
// the model redshift, each one ray per pixel and the supersampled twin.  Built with exactly the Kerr object's flags (csrc/Makefile).
#include "ray_kerr_dv2.h"
#include "march_tile.h"

namespace {

// march_kerr.hip's four kernels over the Kerr Disk V2 Ray's surface ...
__global__ __launch_bounds__(256) void march_kerr_dv2_kernel(BhrKerrMarchArgs a) {
    march_tile_body<false, 0, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256) void march_kerr_dv2_ss_kernel(BhrKerrMarchArgs a) {
    march_tile_body<false, 0, false, false, true>(a, wave_slot());
}
__global__ __launch_bounds__(256) void march_kerr_dv2_exact_kernel(BhrKerrExactMarchArgs a) {
    march_tile_body<false, KERR_EXACT, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256) void march_kerr_dv2_exact_ss_kernel(BhrKerrExactMarchArgs a) {
    march_tile_body<false, KERR_EXACT, false, false, true>(a, wave_slot());
}
// ... and the two over its volume.  The binary64 model inside the march loop needs 272 registers beside the ray's state, which is one
// wave per SIMD; held to 256 = two waves the kernel keeps 15 of them in 64 bytes of scratch per lane and is 1.7 times as fast
// (measured at fhd, A = 0.9: 13.2 ms against 23.1 ms; held to 168 it spills 344 bytes and takes 13.5 ms; DESIGN.md "Kerr Disk V2")
__global__ __launch_bounds__(256, 2) void march_kerr_dv2_volume_kernel(BhrKerrMarchArgs a) {
    march_tile_body<false, KERR_DV2_VOLUME, false, false>(a, wave_slot());
}
__global__ __launch_bounds__(256, 2) void march_kerr_dv2_volume_ss_kernel(BhrKerrMarchArgs a) {
    march_tile_body<false, KERR_DV2_VOLUME, false, false, true>(a, wave_slot());
}

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// BHR_MK_DV2 (the surface, model redshift), BHR_MK_KERR_EXACT (the surface, exact redshift) and BHR_MK_VOLUME (model redshift),
// without differentials, are all there is.
const void *bhr_march_kernel_kerr_dv2(bhr_march_kernel k, int32_t diff, int32_t ss) {
    if (diff) return nullptr;
    if (k == BHR_MK_DV2) return ss ? (const void *)march_kerr_dv2_ss_kernel : (const void *)march_kerr_dv2_kernel;
    if (k == BHR_MK_KERR_EXACT) return ss ? (const void *)march_kerr_dv2_exact_ss_kernel : (const void *)march_kerr_dv2_exact_kernel;
    if (k == BHR_MK_VOLUME) return ss ? (const void *)march_kerr_dv2_volume_ss_kernel : (const void *)march_kerr_dv2_volume_kernel;
    return nullptr;
}
