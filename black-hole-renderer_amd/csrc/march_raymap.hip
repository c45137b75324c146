// march_raymap.hip -> march_raymap.o: the ray map's kernels (build, shade, shade turned about z, shade all samples of a shutter
// frame, and the build and shade kernels of a supersampled map), and nothing else, in a strict object of their own
// (-ffp-contract=off, no fast-math, the ILP-first scheduler).  They are made of the strict march's device functions --
// Ray<DIFF, 0>, Pending, shade_hit, sample_skybox, store_pixel (ray_strict.h, march_device.h).
//
// The layout: three pieces of device code, each written once.
//   raymap_build_kernel<DIFF, SS>     the march that records; SS: the build of a supersampled map
//   raymap_shade_records<DIFF, ROT>   a lane's records -> its Shade       the three shade kernels
//   raymap_values<ROT>                Shade, fate, direction -> values    the three shade kernels
// A shade kernel is its pixel mapping, those two calls and its own way to store: store_pixel (raymap_shade_kernel), the mean
// over the samples (raymap_shade_shutter_kernel), resolve_store over the k x k groups (raymap_shade_ss_kernel).
//
// A ray's path depends on the camera and the geometry of bhr_config only, not on the skybox, the disk texture or t_offset.
// raymap_build_kernel marches a whole-frame view once with the strict Ray and, where the tile kernel shades a parked crossing
// (flush_one), records it instead (Ray::record_one): per pixel up to `slots` Pending records, front to back, and a header --
// executed steps, status, normalized escape direction, number of annulus crossings.  raymap_shade_kernel turns the records
// and the scene as it stands into the frame's BG and DISK values: shade_hit on every record in order from the Shade that
// Ray::init leaves, then the march's own pixel values and store.  These are the same device functions on the same values as
// the strict march runs, in an object without contraction or re-association, so the frame is the strict frame bit for bit.
// A pixel with more crossings than slots is on the overflow list; the shade kernel leaves it alone and march_fix_kernel
// (march_strict_ilp.o) re-marches it in the same frame.
//
// raymap_shade_kernel<DIFF, true> shades the map seen from the build camera turned rigidly about the z axis
// (bhr_raymap_render_view; an orbit frame).  With a disk that is not tilted that turn is a symmetry of everything a ray's path
// depends on -- the hole, the disk plane z = 0, its two radii, the escape sphere -- so the rays of the turned view are the
// stored rays turned: the kernel turns the xy parts of hit point, to_cam, the hit differentials and the escape direction by
// (c, s) = (m.rot_c, m.rot_s) and shades them with the same device functions.  Two products and a sum per component (no
// contraction in this object).  Such a frame is the strict march of the BUILD view's rays, not bit for bit the strict frame of
// the turned view; the launcher takes <DIFF, false> for c = 1, s = 0.
//
// raymap_shade_kernel<DIFF, ROT, true> (STARS) is the frame of a context with a star catalogue (bhr_set_stars; include/bhr.h "point
// stars"): the view's star plane, gathered by stars.hip's kernel ahead of this launch, joins the sky sample ahead of the march's
// own product.  The map's block then has the plane's pointer behind it (BhrRayMapStarArgs); the kernels without stars keep their
// block, their instructions and their registers (profiles/stars_code_objects.txt).
//
// raymap_shade_shutter_kernel<DIFF, ROT> is a shutter frame from the map in one launch (bhr_raymap_render_shutter): per pixel,
// the values raymap_shade_kernel<DIFF, ROT> would store under each sample's (t_offset, c, s), summed on the chip (in LDS, a word per lane and channel) in the order
// of bhr_render_shutter's mean and multiplied by 1 / n.  It is in this object because the object's flags are what make
// shade_hit, sample_skybox and turn_xy give the same bits wherever they are inlined.
#include <type_traits>

#include "ray_strict.h"
#include "raymap_device.h"

namespace {

// ---- the build ----------------------------------------------------------------------------------------------------------------
// One 8x8 tile per wave, tiles in the march's launch order (longest rays first).
// SS: the map of the fine frame of a supersampled map (option "raymap_supersample", a.ss = k > 1; k W x k rows, bhr_fine_camera)
// -- the fine argument block (a.width / rows / pw / ph fine, out_width / out_rows the frame's), fine planes, tiles in plain
// order.  The march, the records and the header are the same; what differs is what goes on the overflow list.
// One kernel template and not a shared body under two kernels: inlined from a function of its own, the body comes out with
// commuted operands in seven instructions of the two DIFF kernels; as a template parameter, SS leaves all four instantiations
// the instructions of the two kernels they were (tools/code_object_diff.py, profiles/raymap_refactor_code_objects.txt).
template <bool DIFF, bool SS>
__global__ __launch_bounds__(256) void raymap_build_kernel(BhrMarchArgs a, BhrRayMapArgs m) {
    const int slot = wave_slot();
    if (slot >= a.n_list) return;    // wave-uniform: the lanes of a wave stay together down to the butterfly
    const int lane = threadIdx.x & 63;
    const int tile = a.tile_order ? a.tile_order[slot] : slot;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int i = tx * 8 + (lane & 7);
    const int j = ty * 8 + (lane >> 3);
    const bool valid = tile < a.n_tiles && i < a.width && j < a.rows;

    Ray<DIFF, 0> ray;
    ray.init(a, valid ? i : 0, valid ? j : 0);
    if (!valid) ray.done = 4;
    const size_t pix = valid ? (size_t)j * a.width + i : 0;
    int cnt = 0, n_rec = 0;       // executed steps; crossings found so far (recorded while below m.slots)
    // the tile body's march loop: a lane leaves when its ray terminates; when some lane has filled both its parking slots
    // the wave records the older crossing of every lane that has one, and the second slot moves up
    while (ray.done == 0) {
        ray.step(a);
        cnt += 1;
        if (ray.full) {
            ray.record_one(m, pix, n_rec);
            ray.full = false;
        }
    }
    ray.step_count = cnt;
    if (cnt > 0) ray.settle(a);
    else ray.done = 3;               // no step taken (max_iter <= 0, or no ray)
    if (__ballot(ray.n_pend > 0)) ray.record_one(m, pix, n_rec);
    if (__ballot(ray.n_pend > 0)) ray.record_one(m, pix, n_rec);

    if (valid) {
        const bool esc = ray.escaped();
        m.steps[pix] = cnt;
        m.status[pix] = esc ? 1 : (ray.done == 2 ? 0 : 2);
        // the direction pixel_values hands sample_skybox
        const V3 dn = esc ? normalized(ray.d) : mk(0.0f, 0.0f, 0.0f);
        m.dir[pix] = dn.x;
        m.dir[(size_t)m.plane + pix] = dn.y;
        m.dir[2 * (size_t)m.plane + pix] = dn.z;
        m.crossings[pix] = n_rec;
    }
    if (SS) {
        raymap_append_overflow_groups(a, m, valid, n_rec > m.slots, lane, pix);   // whole k x k groups (raymap_device.h)
    } else {
        raymap_append_overflow(m, valid && n_rec > m.slots, lane, pix);
    }
    const unsigned long long stored = wave_sum_u32((unsigned int)(valid ? min(n_rec, m.slots) : 0));
    const unsigned long long tot = wave_sum_u32((unsigned int)cnt);
    if (lane == 0) {
        atomicAdd(m.stats, stored);
        atomicAdd(a.ray_steps + (size_t)(blockIdx.x & (BHR_STEP_LANES - 1)) * BHR_STEP_STRIDE, tot);
    }
}

// ---- the shade: the two steps every shade kernel is made of (turn_xy and raymap_pixel_values: raymap_device.h) ---------------------
// The lane's first `count` records of pixel `pix`, front to back, through shade_hit from the Shade that Ray::init leaves.
// ROT: each record is turned about z by (rc, rs) before it is shaded (the head of this file).
// f: the block shade_hit reads a frame's own two fields from -- `a` itself for a frame under one camera (what shade_hit's
// convenience overload passes), a sample's for the shutter kernel.  ONLY f.t_offset and f.cp may be read through f, here as in
// shade_hit and apply_g_factor (march_device.h says so at both): the shutter kernel sets nothing else in it.
// The map is taken by value on purpose: so the four raymap_shade_kernel instantiations compile to the instructions they had with
// the loop written out in them; with the map by reference two instructions of the DIFF ones move
// (tools/code_object_diff.py against the parent build; profiles/raymap_refactor_code_objects.txt is the last run).
template <bool DIFF, bool ROT>
__device__ __forceinline__ Shade raymap_shade_records(const BhrMarchArgs &a, const BhrMarchArgs &f, const BhrRayMapArgs m, size_t pix, int count,
                                                       float rc, float rs) {
    Shade sh;                        // as Ray::init leaves it
    sh.accum = mk(0, 0, 0);
    sh.alpha_total = 0.0f;
    sh.unsure = 0;
    for (int c = 0; c < count; ++c) {
        const float *q = m.hits + (size_t)c * m.comps * (size_t)m.plane + pix;
        const size_t p = (size_t)m.plane;
        float hx = q[0], hy = q[p];
        V3 to_cam = mk(q[2 * p], q[3 * p], q[4 * p]);
        float dxx = 0.0f, dxy = 0.0f, dyx = 0.0f, dyy = 0.0f;
        if (DIFF) { dxx = q[5 * p]; dxy = q[6 * p]; dyx = q[7 * p]; dyy = q[8 * p]; }
        if (ROT) {
            turn_xy(rc, rs, hx, hy);
            turn_xy(rc, rs, to_cam.x, to_cam.y);
            if (DIFF) {
                turn_xy(rc, rs, dxx, dxy);           // d(hit x, hit y) / d(pixel x)
                turn_xy(rc, rs, dyx, dyy);           // d(hit x, hit y) / d(pixel y)
            }
        }
        shade_hit<DIFF, 0>(a, f, sh, hx, hy, to_cam, dxx, dxy, dyx, dyy);
    }
    return sh;
}

// The pixel's BG and DISK values from its shaded records: the ray's fate and its stored escape direction (turned as the
// records were), then the march's own pixel values.
template <bool ROT>
__device__ __forceinline__ void raymap_values(const BhrMarchArgs &a, const BhrRayMapArgs &m, size_t pix, const Shade &sh, float rc, float rs,
                                              float bk[3], float dk[3], const float *star = nullptr) {
    const bool esc = m.status[pix] == 1;
    V3 dir = mk(m.dir[pix], m.dir[(size_t)m.plane + pix], m.dir[2 * (size_t)m.plane + pix]);
    if (ROT) turn_xy(rc, rs, dir.x, dir.y);
    raymap_pixel_values(a, esc, dir, sh, bk, dk, star);
}

// ---- the shade kernels --------------------------------------------------------------------------------------------------------
// One lane per pixel, an 8x8 tile per wave as in the march (texture locality, and store_pixel's packed layout is per tile);
// tiles in row-major order: every lane does about the same work.
// ROT: the records are turned about z by (m.rot_c, m.rot_s) before they are shaded (the head of this file).
// STARS: the frame of a context with a star catalogue (bhr_set_stars) -- the map's block has the view's star plane behind it
// (BhrRayMapStarArgs), whose value at the pixel joins the sky sample.  A pixel on the overflow list gets none: the fix kernel
// stores it.
template <bool DIFF, bool ROT, bool STARS = false>
__global__ __launch_bounds__(256) void raymap_shade_kernel(BhrMarchArgs a, std::conditional_t<STARS, BhrRayMapStarArgs, BhrRayMapArgs> m) {
    const int tile = wave_slot();
    if (tile >= a.n_tiles) return;
    const int lane = threadIdx.x & 63;
    const int i = (tile % a.tiles_x) * 8 + (lane & 7);
    const int j = (tile / a.tiles_x) * 8 + (lane >> 3);
    if (!(i < a.width && j < a.rows)) return;
    const size_t pix = (size_t)j * a.width + i;
    const int count = m.crossings[pix];
    if (count > m.slots) return;     // on the overflow list: the fix kernel marches and stores it
    // The turn's cosine and sine stay scalar operands.  A VALU instruction with an SGPR operand issues at half rate,
    // but there are 8 (16 with differentials) such products per crossing beside the ~700 instructions of shade_hit, and 4 for
    // the sky; copied into two vector registers once, the plain kernel goes from 79 to 81 VGPRs and loses a wave per SIMD
    // (6 -> 5), as scalars both instantiations keep the registers of the kernels without a turn (79 / 76 VGPRs, 6 waves).
    const float rc = ROT ? m.rot_c : 1.0f, rs = ROT ? m.rot_s : 0.0f;
    const Shade sh = raymap_shade_records<DIFF, ROT>(a, a, m, pix, count, rc, rs);
    float bk[3], dk[3];
    if constexpr (STARS) raymap_values<ROT>(a, m, pix, sh, rc, rs, bk, dk, m.stars + pix * 3);
    else raymap_values<ROT>(a, m, pix, sh, rc, rs, bk, dk);
    store_pixel(a, i, j, a.width, bk, dk);
}

// A shutter frame from the map: the mean of the n frames raymap_shade_kernel<DIFF, ROT> stores under the samples
// (t, c, s, cp) = sh.smp[j], j = 0 .. n - 1 (bhr_raymap_render_shutter; include/bhr.h states the mean).  Same mapping, same grid.
// The sample loop is the outer one and wave-uniform: sh.smp[j] is indexed by a scalar, so t, c, s and cp come out of scalar
// loads and stay scalar operands (what keeps the kernel above at its registers).
// Of the march's argument block the shade path reads two things that are a sample's own: t_offset, and the camera position
// (the g-factor's observer radius |cp|, which can differ in the last bit between the f32 positions of an orbit).  shade_hit
// reads both from a second block, which here holds nothing but the sample's two fields out of the table -- scalars; the rest of
// it is never read and never exists.  A whole private copy of the kernel's block with the fields replaced costs the
// anti-aliased kernel 472 bytes of scratch per lane, because the mip tables inside it are indexed by the lane's level.
// A pixel's records, its fate and its escape direction are read again for every sample -- 5 or 9 floats per crossing, the same
// 32-byte runs per tile row each time, so they come from the cache after the first sample -- instead of being held: up to
// 8 x 9 registers per lane would take the kernel from 6 waves per SIMD to 3, and the direction alone held across the samples
// spills two registers of the plain kernel at 6 waves.
// The six running sums are the only state that lives across samples.  They are kept in LDS, a word per lane and channel
// (conflict free, as the march's parking slots): touched once per sample beside the ~700 instructions of a shade_hit, and in
// registers they are what takes the kernel from 6 waves per SIMD to 5 (91 .. 96 VGPRs; 75 .. 80 with them in LDS, under the
// occupancy hint below, without scratch).  No layer goes through memory between the samples.
// ROT with c = 1, s = 0 (a sample at the build camera among turned ones) is an exact turn.
// A pixel on the overflow list is left alone, as above: the launcher takes this kernel for maps without one only.
__shared__ float g_shutter_acc[6][256];
template <bool DIFF, bool ROT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6))) void raymap_shade_shutter_kernel(BhrMarchArgs a, BhrRayMapArgs m, BhrShutterArgs sh) {
    const int tile = wave_slot();
    if (tile >= a.n_tiles) return;
    const int lane = threadIdx.x & 63;
    const int i = (tile % a.tiles_x) * 8 + (lane & 7);
    const int j = (tile / a.tiles_x) * 8 + (lane >> 3);
    if (!(i < a.width && j < a.rows)) return;
    const size_t pix = (size_t)j * a.width + i;
    const int count = m.crossings[pix];
    if (count > m.slots) return;
    const int t = threadIdx.x;
    for (int smp = 0; smp < sh.n; ++smp) {
        // the two fields of the argument block that are a frame's own; the rest of this block is never set
        BhrMarchArgs fs;
        fs.t_offset = sh.smp[smp].t;
        fs.cp[0] = sh.smp[smp].cp[0];
        fs.cp[1] = sh.smp[smp].cp[1];
        fs.cp[2] = sh.smp[smp].cp[2];
        const float rc = ROT ? sh.smp[smp].c : 1.0f, rs = ROT ? sh.smp[smp].s : 0.0f;
        const Shade shd = raymap_shade_records<DIFF, ROT>(a, fs, m, pix, count, rc, rs);
        float bk[3], dk[3];
        raymap_values<ROT>(a, m, pix, shd, rc, rs, bk, dk);
        {
#pragma clang fp contract(off)
            // acc = L_0, then acc = acc + L_j: one f32 addition per channel (smp is wave-uniform)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                g_shutter_acc[k][t] = smp == 0 ? bk[k] : g_shutter_acc[k][t] + bk[k];
                g_shutter_acc[3 + k][t] = smp == 0 ? dk[k] : g_shutter_acc[3 + k][t] + dk[k];
            }
        }
    }
    float acc_b[3], acc_d[3];
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc_b[k] = g_shutter_acc[k][t];
            acc_d[k] = g_shutter_acc[3 + k][t];
            if (sh.n > 1) {
                acc_b[k] = acc_b[k] * sh.inv;
                acc_d[k] = acc_d[k] * sh.inv;
            }
        }
    }
    // six plain stores: the pack kernel makes the split post-pass's operands from the resolved layer, as behind every shutter frame
    const size_t o = ((size_t)j * a.width + i) * 3;
    a.bg[o + 0] = acc_b[0];
    a.bg[o + 1] = acc_b[1];
    a.bg[o + 2] = acc_b[2];
    a.disk[o + 0] = acc_d[0];
    a.disk[o + 1] = acc_d[1];
    a.disk[o + 2] = acc_d[2];
}

// A frame from a supersampled map: one 8x8 tile of the FINE frame per wave, every lane shades its own fine record list exactly
// as raymap_shade_kernel does (same device functions, same order, same turn), and the k x k groups are resolved in the wave by
// resolve_store -- the marched supersampled kernels' butterfly and product, so the output pixel is theirs bit for bit; the lane
// at sub-sample (0, 0) stores it at (i >> log2 k, j >> log2 k) of the output frame.
// Two things the k = 1 kernel does are NOT done here:
//  * no lane returns early (beyond the frame, or on the overflow list): __shfl_xor reads whatever a lane that has left last held
//    in the register.  A lane without a ray shades no record and contributes zeros; its whole group is beyond the frame and is
//    not stored.
//  * overflow is a group's property: a group with any ray over the slots is on the overflow list whole (the build above) and is
//    not stored here at all -- march_fix_ss_kernel marches and resolves it, so that pixel is the strict supersampled march itself.
//    Its lanes shade nothing.
template <bool DIFF, bool ROT>
__global__ __launch_bounds__(256) void raymap_shade_ss_kernel(BhrMarchArgs a, BhrRayMapArgs m) {
    const int tile = wave_slot();
    if (tile >= a.n_tiles) return;   // wave-uniform
    const int lane = threadIdx.x & 63;
    const int i = (tile % a.tiles_x) * 8 + (lane & 7);
    const int j = (tile / a.tiles_x) * 8 + (lane >> 3);
    const bool valid = i < a.width && j < a.rows;
    const size_t pix = valid ? (size_t)j * a.width + i : 0;
    const int crossings = valid ? m.crossings[pix] : 0;
    int u = crossings > m.slots ? 1 : 0;
    for (int x = 1; x < a.ss; x <<= 1) u |= __shfl_xor(u, x, BHR_WAVE);
    for (int x = 8; x < 8 * a.ss; x <<= 1) u |= __shfl_xor(u, x, BHR_WAVE);
    const bool have = valid && u == 0;
    const float rc = ROT ? m.rot_c : 1.0f, rs = ROT ? m.rot_s : 0.0f;   // scalar operands, as in raymap_shade_kernel
    const Shade sh = raymap_shade_records<DIFF, ROT>(a, a, m, pix, have ? crossings : 0, rc, rs);
    RayMapValues val = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}};
    if (have) raymap_values<ROT>(a, m, pix, sh, rc, rs, val.v, val.v + 3);
    // every lane of the wave, whatever it holds
    resolve_store(a, val, have, have, i, j, 8);
}

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// ss: the kernels of a supersampled map (a.ss > 1); its shutter frames go sample by sample through the shade kernels, there is
// no fused supersampled shutter kernel
const void *bhr_march_kernel_raymap(bhr_march_kernel k, int32_t diff, int32_t ss) {
    if (ss) {
        switch (k) {
        case BHR_MK_RAYMAP_BUILD: return diff ? (const void *)raymap_build_kernel<true, true> : (const void *)raymap_build_kernel<false, true>;
        case BHR_MK_RAYMAP_SHADE: return diff ? (const void *)raymap_shade_ss_kernel<true, false> : (const void *)raymap_shade_ss_kernel<false, false>;
        case BHR_MK_RAYMAP_SHADE_ROT: return diff ? (const void *)raymap_shade_ss_kernel<true, true> : (const void *)raymap_shade_ss_kernel<false, true>;
        default: return nullptr;
        }
    }
    switch (k) {
    case BHR_MK_RAYMAP_BUILD: return diff ? (const void *)raymap_build_kernel<true, false> : (const void *)raymap_build_kernel<false, false>;
    case BHR_MK_RAYMAP_SHADE: return diff ? (const void *)raymap_shade_kernel<true, false> : (const void *)raymap_shade_kernel<false, false>;
    case BHR_MK_RAYMAP_SHADE_ROT: return diff ? (const void *)raymap_shade_kernel<true, true> : (const void *)raymap_shade_kernel<false, true>;
    case BHR_MK_RAYMAP_SHADE_STARS:
        return diff ? (const void *)raymap_shade_kernel<true, false, true> : (const void *)raymap_shade_kernel<false, false, true>;
    case BHR_MK_RAYMAP_SHADE_STARS_ROT:
        return diff ? (const void *)raymap_shade_kernel<true, true, true> : (const void *)raymap_shade_kernel<false, true, true>;
    case BHR_MK_RAYMAP_SHUTTER:
        return diff ? (const void *)raymap_shade_shutter_kernel<true, false> : (const void *)raymap_shade_shutter_kernel<false, false>;
    case BHR_MK_RAYMAP_SHUTTER_ROT:
        return diff ? (const void *)raymap_shade_shutter_kernel<true, true> : (const void *)raymap_shade_shutter_kernel<false, true>;
    default: return nullptr;
    }
}
