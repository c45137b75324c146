// march_kerr_raymap.hip -> march_kerr_raymap.o: the Kerr ray map's kernels (build, shade, shade turned about z, the shade of a
// whole shutter exposure, the build and shade kernels of a supersampled map, and the march of the overflow list), each with the
// model redshift and with the exact one, and nothing else.  Built with exactly the flags of march_kerr.o (csrc/Makefile says
// why): the kernels are made of the Kerr march's device functions -- Ray<false, RS>, Pending, kerr_shade_hit, sample_skybox,
// store_pixel (ray_kerr.h, march_device.h) -- and under those flags a function gives the same bits wherever it is inlined.
//
// The layout: four pieces of device code, each written once.
//   kerr_raymap_build_kernel<RS, KIND>     the march that records; KIND: plain, the build of a supersampled map, the build that
//                                          keeps the photon's momentum
//   kerr_raymap_shade_records<RS, ROT>     a lane's records -> its Shade       the three shade kernels
//   kerr_raymap_values<ROT>                Shade, fate, direction -> values    the three shade kernels
//   kerr_raymap_fix_kernel<RS, SS>         the march of the overflow list; SS: whole k x k groups, resolved in the wave
// A shade kernel is its pixel mapping, the two calls and its own way to store: store_pixel (kerr_raymap_shade_kernel), the mean
// over the samples (kerr_raymap_shade_shutter_kernel), resolve_store over the k x k groups (kerr_raymap_shade_ss_kernel).
// What the two maps' kernels spell alike -- both overflow appends, the turn, the pixel's values, the six values handed to
// resolve_store -- is raymap_device.h's.  A shutter frame's sums, mean and stores are not: called through a function they move
// instructions of march_raymap.hip's shutter kernels and take 8 or 9 out of this object's.
// Which spelling each piece has was decided by the compiler's output (tools/code_object_diff.py against the build with the
// pieces written out three, three, three and two times; profiles/kerr_raymap_refactor_code_objects.txt is the last run): the
// build, fix and k = 1 shade kernels are the instructions they were, the supersampled and shutter shade kernels keep their
// registers.  The comment at each piece names the spellings that lost that.
//
// A Kerr ray's path depends on the camera, the geometry of bhr_config and the spin, not on the skybox, the disk texture or
// t_offset.  kerr_raymap_build_kernel marches a whole-frame view once with the Kerr Ray and, where the tile kernel shades a
// parked crossing (flush_one), records it instead (Ray::record_one): per pixel up to `slots` Pending<false> records, front to
// back, and a header -- executed steps, status, normalized escape direction, number of annulus crossings.  For the exact
// redshift the three to_cam floats of a record are the photon's momentum (p_x, p_y, 0) at the hit, which is what its step
// parks.  kerr_raymap_shade_kernel turns the records and the scene as it stands into the frame's BG and DISK values:
// kerr_shade_hit on every record in order from the Shade that Ray::init leaves, then the march's own pixel values and store --
// the frame march_kerr_kernel / march_kerr_exact_kernel leaves, bit for bit.  A pixel with more crossings than slots is on the
// overflow list; the shade kernel leaves it alone and kerr_raymap_fix_kernel marches it in the same frame.
//
// kerr_raymap_shade_kernel<RS, true> shades the map seen from the build camera turned rigidly about the z axis
// (bhr_kerr_raymap_render_view; an orbit frame).  The spin axis is z and the disk of a spinning hole is not tilted, so that turn
// is a symmetry of everything a Kerr ray's path depends on: the rays of the turned view are the stored rays turned.  The kernel
// turns the xy parts of hit point, to_cam (a direction or a momentum: a vector either way) and escape direction by
// (c, s) = (m.rot_c, m.rot_s).  Such a frame is the Kerr march of the BUILD view's rays, not bit for bit the marched frame of
// the turned view; the launcher takes <RS, false> for c = 1, s = 0.
//
// The supersampled map (option "kerr_raymap_supersample", a.ss = k > 1) is the map of the fine frame, k W x k rows seen through
// bhr_fine_camera: kerr_raymap_build_kernel<RS, KERR_BUILD_SS>, kerr_raymap_shade_ss_kernel and kerr_raymap_fix_kernel<RS, true>
// take the fine argument block (a.width / rows / pw / ph fine, out_width / out_rows the frame's) and handle the k x k groups in
// the wave: a group with any ray over the slots goes on the overflow list whole, every other group is resolved by resolve_store
// (march_device.h) from its lanes' shaded records, and the listed groups are marched and resolved by the fix kernel -- the frame
// march_kerr_ss_kernel / march_kerr_exact_ss_kernel leaves, bit for bit.
//
// kerr_raymap_shade_shutter_kernel<RS, ROT> is a shutter frame from the k = 1 map in one launch (bhr_kerr_raymap_render_shutter's
// fused route): the mean of the n frames kerr_raymap_shade_kernel<RS, ROT> stores under n (t_offset, turn, camera position), the
// running sums kept on the chip.
//
// No differentials (the Kerr Ray has none); the momentum build and the shutter kernel have no supersampled form.
#include <type_traits>

#include "ray_kerr.h"
#include "raymap_device.h"

namespace {

// the block of a redshift's kernels: the Kerr block, with the ISCO's numbers behind it for the exact one
template <int RS>
using KerrBlock = std::conditional_t<RS == KERR_EXACT, BhrKerrExactMarchArgs, BhrKerrMarchArgs>;

// ---- the build ----------------------------------------------------------------------------------------------------------------
// raymap_build_kernel's march (march_raymap.hip) over the Kerr Ray: one 8x8 tile per wave, tiles in the march's launch order
// (longest rays first).  The march, the records, the header and the counters are the same for every KIND; what differs:
//   KERR_BUILD_SS   the build of a supersampled map: the fine block, the fine tiles in plain order (a.tile_order null), and a
//                   k x k group with ANY ray over the slots appended to the overflow list whole (raymap_device.h)
//   KERR_BUILD_MOM  the build under a Kerr polarisation (bhr_set_kerr_polarization; march_kerr_polar.hip has the pass that
//                   reads what it keeps): Ray<false, RS, true> parks the photon's whole momentum (p_x, p_y, p_z) with each
//                   crossing and record_mom stores it in the map's momentum planes m.mom beside the record.  Records, header,
//                   overflow list and counters are the plain build's bit for bit -- the march is the same and the momentum
//                   rides in words the plain ray leaves alone.
// Plain integers and not an enum: an unnamed enum's `$` in the mangled names keeps tools/code_object_diff.py from pairing the kernels.
// One kernel template with the recording call chosen by `if constexpr` at each of its three sites: all six instantiations are
// the instructions of the six kernels they were.  Ruled out: a body of its own that the kernels call (it moved ~180
// instructions of the plain build), and the recording call behind a local lambda (same registers and instruction counts in all
// six, the text of none).
constexpr int KERR_BUILD_PLAIN = 0, KERR_BUILD_SS = 1, KERR_BUILD_MOM = 2;
template <int RS, int KIND>
__global__ __launch_bounds__(256) void kerr_raymap_build_kernel(KerrBlock<RS> a, std::conditional_t<KIND == KERR_BUILD_MOM, BhrRayMapMomArgs, BhrRayMapArgs> m) {
    const int slot = wave_slot();
    if (slot >= a.n_list) return;    // wave-uniform: the lanes of a wave stay together down to the ballots and the butterfly
    const int lane = threadIdx.x & 63;
    const int tile = a.tile_order ? a.tile_order[slot] : slot;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int i = tx * 8 + (lane & 7);
    const int j = ty * 8 + (lane >> 3);
    const bool valid = tile < a.n_tiles && i < a.width && j < a.rows;

    Ray<false, RS, KIND == KERR_BUILD_MOM> ray;
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
            if constexpr (KIND == KERR_BUILD_MOM) ray.record_mom(m, m.mom, pix, n_rec);
            else ray.record_one(m, pix, n_rec);
            ray.full = false;
        }
    }
    ray.step_count = cnt;
    if (cnt > 0) ray.settle(a);
    else ray.done = 3;               // no step taken (max_iter <= 0, or no ray)
    if (__ballot(ray.n_pend > 0)) {
        if constexpr (KIND == KERR_BUILD_MOM) ray.record_mom(m, m.mom, pix, n_rec);
        else ray.record_one(m, pix, n_rec);
    }
    if (__ballot(ray.n_pend > 0)) {
        if constexpr (KIND == KERR_BUILD_MOM) ray.record_mom(m, m.mom, pix, n_rec);
        else ray.record_one(m, pix, n_rec);
    }

    if (valid) {
        const bool esc = ray.escaped(a);
        m.steps[pix] = cnt;
        m.status[pix] = esc ? 1 : (ray.done == 2 ? 0 : 2);
        // the direction pixel_values hands sample_skybox
        V3 dn = mk(0.0f, 0.0f, 0.0f);
        if (esc) dn = normalized(ray.velocity(a));
        m.dir[pix] = dn.x;
        m.dir[(size_t)m.plane + pix] = dn.y;
        m.dir[2 * (size_t)m.plane + pix] = dn.z;
        m.crossings[pix] = n_rec;
    }
    if constexpr (KIND == KERR_BUILD_SS) raymap_append_overflow_groups(a, m, valid, n_rec > m.slots, lane, pix);
    else raymap_append_overflow(m, valid && n_rec > m.slots, lane, pix);
    const unsigned long long stored = wave_sum_u32((unsigned int)(valid ? min(n_rec, m.slots) : 0));
    const unsigned long long tot = wave_sum_u32((unsigned int)cnt);
    if (lane == 0) {
        atomicAdd(m.stats, stored);
        atomicAdd(a.ray_steps + (size_t)(blockIdx.x & (BHR_STEP_LANES - 1)) * BHR_STEP_STRIDE, tot);
    }
}

// ---- the shade: the two steps every shade kernel is made of (turn_xy and raymap_pixel_values: raymap_device.h) ---------------------
// The lane's first `count` records of pixel `pix`, front to back, through kerr_shade_hit from the Shade that Ray::init leaves.
// ROT: each record is turned about z by (rc, rs) before it is shaded (the head of this file).
// f: the block kerr_shade_hit reads a frame's own fields from (t_offset in kerr_sample_disk, cp in both g-factors) -- `a` itself
// for a frame under one camera, a sample's for the shutter kernel, which sets nothing else in it (ray_kerr.h: kerr_sample_disk
// says why it is a bare BhrMarchArgs); the spin and the ISCO stay on `a`, the kernel's own block.
// The map is taken by value, as march_raymap.hip's raymap_shade_records takes it: so the four kerr_raymap_shade_kernel
// instantiations compile to the instructions they had with the loop written out in them; with the map by reference 7 or 8
// instructions of each come out otherwise.
// Pix: the pixel index in the caller's own type -- size_t, and the shutter kernel's int, which it makes opaque once per sample
// and widens at each use.  Taken as size_t from that kernel too, the index is widened once ahead of the loop: the four shutter
// kernels then lose 3 or 4 instructions with about 100 of 1800 elsewhere (at the same speed: DESIGN 4 "Kerr ray map: one build
// kernel ..."); in its own type they keep their instruction counts, and all that differs from the loop written out is commuted
// operands, two swapped scalar pairs and one scalar branch (22 or 23 instructions).
template <int RS, bool ROT, class Pix>
__device__ __forceinline__ Shade kerr_raymap_shade_records(const BhrMarchArgs &a, const BhrMarchArgs &f, const BhrRayMapArgs m, Pix pix, int count,
                                                            float rc, float rs) {
    Shade sh;                        // as Ray::init leaves it
    sh.accum = mk(0, 0, 0);
    sh.alpha_total = 0.0f;
    sh.unsure = 0;
    const size_t p = (size_t)m.plane;
    for (int c = 0; c < count; ++c) {
        const float *q = m.hits + (size_t)c * m.comps * p + pix;
        float hx = q[0], hy = q[p];
        V3 to_cam = mk(q[2 * p], q[3 * p], q[4 * p]);
        if (ROT) {
            turn_xy(rc, rs, hx, hy);
            turn_xy(rc, rs, to_cam.x, to_cam.y);
        }
        kerr_shade_hit<RS>(a, f, sh, hx, hy, to_cam);
    }
    return sh;
}

// The pixel's BG and DISK values from its shaded records: the ray's fate and its stored escape direction (turned as the
// records were), then the march's own pixel values.
// star: the pixel's value of the view's star plane (the STARS kernel), which joins the sky sample; null: none.
template <bool ROT>
__device__ __forceinline__ void kerr_raymap_values(const BhrMarchArgs &a, const BhrRayMapArgs &m, size_t pix, const Shade &sh, float rc, float rs,
                                                   float bk[3], float dk[3], const float *star = nullptr) {
    const size_t p = (size_t)m.plane;
    const bool esc = m.status[pix] == 1;
    V3 dir = mk(m.dir[pix], m.dir[p + pix], m.dir[2 * p + pix]);
    if (ROT) turn_xy(rc, rs, dir.x, dir.y);
    raymap_pixel_values(a, esc, dir, sh, bk, dk, star);
}

// ---- the shade kernels --------------------------------------------------------------------------------------------------------
// One lane per pixel, an 8x8 tile per wave as in the march (texture locality, and store_pixel's packed layout is per tile);
// tiles in row-major order: every lane does about the same work.
// ROT: the records are turned about z by (m.rot_c, m.rot_s) before they are shaded (the head of this file).
// STARS: the frame of a context with a Kerr star catalogue (bhr_set_kerr_stars) -- march_raymap.hip's raymap_shade_kernel<.., true>
// over the Kerr records: the map's block has the view's star plane behind it (BhrRayMapStarArgs), gathered by stars.hip's kernel
// over this map's status and direction planes ahead of the launch, and the plane's value at the pixel joins the sky sample in one
// f32 addition ahead of the march's own product (raymap_device.h: raymap_pixel_values).  A pixel on the overflow list gets none:
// the fix kernel stores it.  The kernels without stars keep their block, their instructions and their registers
// (profiles/kerr_stars_code_objects.txt).  No supersampled, shutter or fix twin.
template <int RS, bool ROT, bool STARS = false>
__global__ __launch_bounds__(256) void kerr_raymap_shade_kernel(KerrBlock<RS> a, std::conditional_t<STARS, BhrRayMapStarArgs, BhrRayMapArgs> m) {
    const int tile = wave_slot();
    if (tile >= a.n_tiles) return;
    const int lane = threadIdx.x & 63;
    const int i = (tile % a.tiles_x) * 8 + (lane & 7);
    const int j = (tile / a.tiles_x) * 8 + (lane >> 3);
    if (!(i < a.width && j < a.rows)) return;
    const size_t pix = (size_t)j * a.width + i;
    const int count = m.crossings[pix];
    if (count > m.slots) return;     // on the overflow list: the fix kernel marches and stores it
    // the turn's cosine and sine stay scalar operands (march_raymap.hip: raymap_shade_kernel says why)
    const float rc = ROT ? m.rot_c : 1.0f, rs = ROT ? m.rot_s : 0.0f;
    const Shade sh = kerr_raymap_shade_records<RS, ROT>(a, a, m, pix, count, rc, rs);
    float bk[3], dk[3];
    if constexpr (STARS) kerr_raymap_values<ROT>(a, m, pix, sh, rc, rs, bk, dk, m.stars + pix * 3);
    else kerr_raymap_values<ROT>(a, m, pix, sh, rc, rs, bk, dk);
    store_pixel(a, i, j, a.width, bk, dk);
}

// A shutter frame from the Kerr map: the mean of the n frames kerr_raymap_shade_kernel<RS, ROT> stores under the samples
// (t, c, s, cp) = sh.smp[j], j = 0 .. n - 1 (bhr_kerr_raymap_render_shutter; include/bhr.h states the mean) -- march_raymap.hip's
// raymap_shade_shutter_kernel over the Kerr records.  Same mapping, same grid, same early exits as the k = 1 shade above.
// The sample loop is the outer one and wave-uniform: sh.smp[j] is indexed by a scalar, so t, c, s and cp come out of scalar
// loads and stay scalar operands.  The fields of the argument block that are a sample's own go to kerr_shade_hit in a second
// block that holds the sample's four floats out of the table and nothing else (kerr_raymap_shade_records: f).
// A pixel's records, fate and escape direction are read again for every sample (the same 32-byte runs per tile row each time)
// instead of being held across them.  The six running sums are the only state that lives across samples; they are kept in LDS, a
// word per lane and channel, conflict free: in registers they are live across the whole of
// kerr_shade_hit and cost the kernel a wave per SIMD against its k = 1 twin (DESIGN 4 "Kerr shutter frames from the map" has
// both forms' registers).  No layer goes through memory between the samples.
// This object is compiled with -ffp-contract=on: the accumulation and the final product sit under `fp contract(off)`, or the last
// product of a sample's value would be fused into the sum and the mean would no longer be the sum of the frames' stored values.
// ROT with c = 1, s = 0 (a sample at the build camera among turned ones) is an exact turn.
// A pixel on the overflow list is left alone, as above: the launcher takes this kernel for maps without one only.
__shared__ float g_kerr_shutter_acc[6][256];
template <int RS, bool ROT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RS == KERR_EXACT ? 7 : 8))) void kerr_raymap_shade_shutter_kernel(KerrBlock<RS> a, BhrRayMapArgs m,
                                                                                                                                      BhrShutterArgs sh) {
    const int tile = wave_slot();
    if (tile >= a.n_tiles) return;
    const int lane = threadIdx.x & 63;
    const int i = (tile % a.tiles_x) * 8 + (lane & 7);
    const int j = (tile / a.tiles_x) * 8 + (lane >> 3);
    if (!(i < a.width && j < a.rows)) return;
    int pix = j * a.width + i;           // below 2^31: the build refuses a plane that is not
    const int count = m.crossings[pix];
    if (count > m.slots) return;
    // the lane's word of the sums: the wave's number in the block is a scalar and the lane is the low bits of (i, j), so no
    // register is spent on threadIdx.x across kerr_shade_hit
    const int t = __builtin_amdgcn_readfirstlane(threadIdx.x & 192) + (i & 7) + ((j & 7) << 3);
    for (int smp = 0; smp < sh.n; ++smp) {
        // The pixel index is made opaque once per sample: the loads below are then not loop-invariant and stay inside the
        // sample.  Left alone, the compiler hoists the pixel's fate and escape direction out of the sample loop and holds them
        // across kerr_shade_hit -- 5 or 6 spilled registers (24 / 28 bytes of scratch) at the k = 1 twin's occupancy.
        asm volatile("" : "+v"(pix));
        // the fields of the argument block that are a frame's own; the rest of this block is never set
        BhrMarchArgs fs;
        fs.t_offset = sh.smp[smp].t;
        fs.cp[0] = sh.smp[smp].cp[0];
        fs.cp[1] = sh.smp[smp].cp[1];
        fs.cp[2] = sh.smp[smp].cp[2];
        const float rc = ROT ? sh.smp[smp].c : 1.0f, rs = ROT ? sh.smp[smp].s : 0.0f;
        const Shade shd = kerr_raymap_shade_records<RS, ROT>(a, fs, m, pix, count, rc, rs);
        float bk[3], dk[3];
        kerr_raymap_values<ROT>(a, m, pix, shd, rc, rs, bk, dk);
        {
#pragma clang fp contract(off)
            // acc = L_0, then acc = acc + L_j: one f32 addition per channel (smp is wave-uniform)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                g_kerr_shutter_acc[k][t] = smp == 0 ? bk[k] : g_kerr_shutter_acc[k][t] + bk[k];
                g_kerr_shutter_acc[3 + k][t] = smp == 0 ? dk[k] : g_kerr_shutter_acc[3 + k][t] + dk[k];
            }
        }
    }
    float acc_b[3], acc_d[3];
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc_b[k] = g_kerr_shutter_acc[k][t];
            acc_d[k] = g_kerr_shutter_acc[3 + k][t];
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
// as kerr_raymap_shade_kernel does (same device functions, same order, same turn), and the k x k groups are resolved in the wave
// by resolve_store -- the marched Kerr supersampled kernels' butterfly and product, so the output pixel is theirs bit for bit;
// the lane at sub-sample (0, 0) stores it at (i >> log2 k, j >> log2 k) of the output frame.
// Two things the k = 1 kernel does are NOT done here:
//  * no lane returns early (beyond the frame, or on the overflow list): __shfl_xor reads whatever a lane that has left last held
//    in the register.  A lane without a ray shades no record and contributes zeros; its whole group is beyond the frame and is
//    not stored.
//  * overflow is a group's property: a group with any ray over the slots is on the overflow list whole (the build above) and is
//    not stored here at all -- kerr_raymap_fix_kernel<RS, true> marches and resolves it.  Its lanes shade nothing.
// The occupancy hint is the k = 1 twin's waves per SIMD (63 / 71 VGPRs: 8 with the model redshift, 7 with the exact one).  The
// six values across the butterfly are the only new live state; without the hint the model kernels take 66 VGPRs and lose a
// wave, with it 64, and the exact ones 72 for 71 -- no scratch either way (tools/kernel_resources.sh kerr_raymap).
template <int RS, bool ROT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RS == KERR_EXACT ? 7 : 8))) void kerr_raymap_shade_ss_kernel(KerrBlock<RS> a, BhrRayMapArgs m) {
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
    const float rc = ROT ? m.rot_c : 1.0f, rs = ROT ? m.rot_s : 0.0f;   // scalar operands, as in kerr_raymap_shade_kernel
    const Shade sh = kerr_raymap_shade_records<RS, ROT>(a, a, m, pix, have ? crossings : 0, rc, rs);
    RayMapValues val = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}};
    if (have) kerr_raymap_values<ROT>(a, m, pix, sh, rc, rs, val.v, val.v + 3);
    // every lane of the wave, whatever it holds
    resolve_store(a, val, have, have, i, j, 8);
}

// ---- the overflow list --------------------------------------------------------------------------------------------------------
// march_fix_kernel's body (march_strict_ilp.hip) over the Kerr Ray: the pixels of the map's overflow list, 64 per wave whatever
// tile they came from, marched from the frame's own camera and stored through the march's own values and store -- the marched
// Kerr frame's pixels.  Launched with a grid for the list's capacity; waves beyond the count the device holds exit at once.
// SS: the overflow list of a supersampled map -- whole k x k groups, k^2 consecutive entries in sub-sample order, k^2-aligned
// (the build above), 64 / k^2 groups per wave -- and the groups resolved like a tile's, with the sub-sample rows k lanes apart:
// the supersampled Kerr march of those pixels.  Only the last store differs; under `if constexpr` all four instantiations are
// the instructions of the four kernels they were.
template <int RS, bool SS>
__global__ __launch_bounds__(256) void kerr_raymap_fix_kernel(KerrBlock<RS> a) {
    const int wave = wave_slot();
    unsigned int n = *a.fix_count;
    if (n > (unsigned int)a.fix_cap) n = (unsigned int)a.fix_cap;
    if ((unsigned int)wave * 64u >= n) return;    // wave-uniform
    const int lane = threadIdx.x & 63;
    const unsigned int k = (unsigned int)wave * 64u + (unsigned int)lane;
    const bool valid = k < n;
    const int pix = valid ? a.fix_list[k] : 0;
    Ray<false, RS> ray;
    ray.init(a, pix % a.width, pix / a.width);
    if (!valid) ray.done = 4;
    int cnt = 0;
    while (ray.done == 0) {
        ray.step(a);
        cnt += 1;
        if (ray.full) { ray.flush_one(a); ray.full = false; }
    }
    ray.step_count = cnt;
    if (cnt > 0) ray.settle(a);
    else ray.done = 3;
    if (__ballot(ray.n_pend > 0)) ray.flush_one(a);
    if (__ballot(ray.n_pend > 0)) ray.flush_one(a);
    if constexpr (SS) {
        resolve_store(a, ray, valid, valid, pix % a.width, pix / a.width, a.ss);
    } else if (valid) {
        float bk[3], dk[3];
        ray.values(a, bk, dk);
        store_pixel(a, pix % a.width, pix / a.width, a.width, bk, dk);
    }
    const unsigned long long tot = wave_sum_u32((unsigned int)ray.step_count);
    if (lane == 0) atomicAdd(a.ray_steps + (size_t)(blockIdx.x & (BHR_STEP_LANES - 1)) * BHR_STEP_STRIDE, tot);
}

}  // namespace

// ---- the kernels of this object, by the launcher's names (march_launch.hip); null: not in this object ----------
// exact: the kernels of the exact redshift (they take BhrKerrExactMarchArgs); ss: the kernels of a supersampled map (a.ss > 1;
// the momentum build has none, neither have the STARS shade kernels, and neither have the shutter kernels: a supersampled map's
// shutter frames go sample by sample)
const void *bhr_march_kernel_kerr_raymap(bhr_march_kernel k, int32_t exact, int32_t ss) {
    if (ss) {
        switch (k) {
        case BHR_MK_KERR_RAYMAP_BUILD: return exact ? (const void *)kerr_raymap_build_kernel<KERR_EXACT, KERR_BUILD_SS> : (const void *)kerr_raymap_build_kernel<0, KERR_BUILD_SS>;
        case BHR_MK_KERR_RAYMAP_SHADE: return exact ? (const void *)kerr_raymap_shade_ss_kernel<KERR_EXACT, false> : (const void *)kerr_raymap_shade_ss_kernel<0, false>;
        case BHR_MK_KERR_RAYMAP_SHADE_ROT: return exact ? (const void *)kerr_raymap_shade_ss_kernel<KERR_EXACT, true> : (const void *)kerr_raymap_shade_ss_kernel<0, true>;
        case BHR_MK_KERR_RAYMAP_FIX: return exact ? (const void *)kerr_raymap_fix_kernel<KERR_EXACT, true> : (const void *)kerr_raymap_fix_kernel<0, true>;
        default: return nullptr;
        }
    }
    switch (k) {
    case BHR_MK_KERR_RAYMAP_BUILD: return exact ? (const void *)kerr_raymap_build_kernel<KERR_EXACT, KERR_BUILD_PLAIN> : (const void *)kerr_raymap_build_kernel<0, KERR_BUILD_PLAIN>;
    case BHR_MK_KERR_RAYMAP_SHADE: return exact ? (const void *)kerr_raymap_shade_kernel<KERR_EXACT, false> : (const void *)kerr_raymap_shade_kernel<0, false>;
    case BHR_MK_KERR_RAYMAP_SHADE_ROT: return exact ? (const void *)kerr_raymap_shade_kernel<KERR_EXACT, true> : (const void *)kerr_raymap_shade_kernel<0, true>;
    case BHR_MK_KERR_RAYMAP_SHADE_STARS:
        return exact ? (const void *)kerr_raymap_shade_kernel<KERR_EXACT, false, true> : (const void *)kerr_raymap_shade_kernel<0, false, true>;
    case BHR_MK_KERR_RAYMAP_SHADE_STARS_ROT:
        return exact ? (const void *)kerr_raymap_shade_kernel<KERR_EXACT, true, true> : (const void *)kerr_raymap_shade_kernel<0, true, true>;
    case BHR_MK_KERR_RAYMAP_BUILD_MOM: return exact ? (const void *)kerr_raymap_build_kernel<KERR_EXACT, KERR_BUILD_MOM> : (const void *)kerr_raymap_build_kernel<0, KERR_BUILD_MOM>;
    case BHR_MK_KERR_RAYMAP_FIX: return exact ? (const void *)kerr_raymap_fix_kernel<KERR_EXACT, false> : (const void *)kerr_raymap_fix_kernel<0, false>;
    case BHR_MK_KERR_RAYMAP_SHUTTER:
        return exact ? (const void *)kerr_raymap_shade_shutter_kernel<KERR_EXACT, false> : (const void *)kerr_raymap_shade_shutter_kernel<0, false>;
    case BHR_MK_KERR_RAYMAP_SHUTTER_ROT:
        return exact ? (const void *)kerr_raymap_shade_shutter_kernel<KERR_EXACT, true> : (const void *)kerr_raymap_shade_shutter_kernel<0, true>;
    default: return nullptr;
    }
}
