// raymap_device.h -- the device code the two ray maps' kernels state once (march_raymap.hip, march_kerr_raymap.hip): what a
// build kernel appends to the overflow list (one ray per pixel, or whole k x k groups), and what a shade kernel does besides
// shading the records -- the turn about z, the pixel's values, the six values a supersampled shade hands resolve_store.
// Included behind the object's one ray_*.h (V3, Shade, sample_skybox and the argument blocks are march_device.h's); every
// function is inlined, under the including object's own flags.
// The march that records and the loops over the records stay with each object: they are made of its Ray and its shade_hit.
#pragma once

// x' = c x - s y, y' = s x + c y: two products and a sum per component.  Kept out of contraction by the pragma -- the Kerr
// object contracts within an expression, the strict object not at all, where the pragma does nothing -- so both maps turn a
// record to the same bits.
__device__ __forceinline__ void turn_xy(float c, float s, float &x, float &y) {
#pragma clang fp contract(off)
    const float xr = c * x - s * y, yr = s * x + c * y;
    x = xr;
    y = yr;
}

// render.py:3008-3018 as pixel_values has it, from the direction the build kernel stored already normalized
// star: the pixel's value of the star plane (stars.hip; include/bhr.h "point stars"), added to the sky sample ahead of the product --
// of a captured ray's pixel too, which has images from the triangles of its neighbours; null: no catalogue, no addition
__device__ __forceinline__ void raymap_pixel_values(const BhrMarchArgs &a, bool escaped, V3 dir, const Shade &sh, float bk[3], float dk[3],
                                                    const float *star = nullptr) {
    V3 bg = mk(0, 0, 0);
    if (escaped) bg = sample_skybox(a.sc, dir);
    if (star) {
        // a statement of its own, kept out of contraction (the Kerr object contracts within an expression; the strict object not
        // at all, where the pragma does nothing): the sky sample keeps the bits it has without a catalogue, the sum is one f32 addition
#pragma clang fp contract(off)
        bg = bg + mk(star[0], star[1], star[2]);
    }
    float k = 1.0f - sh.alpha_total;
    bk[0] = __fmul_rn(bg.x, k);
    bk[1] = __fmul_rn(bg.y, k);
    bk[2] = __fmul_rn(bg.z, k);
    dk[0] = fminf(fmaxf(sh.accum.x, 0.0f), 1.0f);
    dk[1] = fminf(fmaxf(sh.accum.y, 0.0f), 1.0f);
    dk[2] = fminf(fmaxf(sh.accum.z, 0.0f), 1.0f);
}

// The header store is NOT here: each build kernel keeps its six stores.  Called through a function -- with the direction as a
// value, or evaluated between the stores as the kernels have it -- they come out in another order in raymap_build_kernel<true, *>
// (20 instructions of each; with the direction as a value, in all six build kernels): tools/code_object_diff.py.
// Neither are a shutter kernel's running sums in LDS, its mean and its six stores (the LDS array handed in by reference): called
// through functions they take 5 instructions out of each raymap_shade_shutter_kernel and 8 or 9 out of each
// kerr_raymap_shade_shutter_kernel (registers and LDS kept).  The two kernels keep them written out.

// One ray per pixel, more crossings than slots: the pixel keeps its first m.slots records and goes on the overflow list
// (wave-aggregated append, as the guard kernel's; every pixel is appended at most once and the list has room for all of them).
// Every lane of the wave calls it.
__device__ __forceinline__ void raymap_append_overflow(const BhrRayMapArgs &m, bool over, int lane, size_t pix) {
    const unsigned long long om = __ballot(over);
    if (om) {
        const int first = __ffsll((long long)om) - 1;
        unsigned int base = 0;
        if (lane == first) base = atomicAdd(m.over_count, (unsigned int)__popcll(om));
        base = __shfl(base, first, BHR_WAVE);
        if (over) m.over_list[base + (unsigned int)__popcll(om & ((1ull << lane) - 1ull))] = (int32_t)pix;
    }
}

// A supersampled build (a.ss = k > 1): a k x k group with ANY ray over the slots goes on the overflow list whole, in the format
// march_tile_body writes for the supersampled fix kernels (march_tile.h): k^2 consecutive entries in sub-sample order
// (sy k + sx), k^2-aligned, groups in the order of their (0, 0) lanes -- a fix kernel resolves a group from 64 / k^2 of them per
// wave.  k W and k rows are multiples of k (and 8 is one of k), so a group lies in one tile, inside the frame or outside it, whole.
// mine: this lane's ray is over the slots.  Every lane of the wave calls it: no lane may have returned ahead of the butterfly.
__device__ __forceinline__ void raymap_append_overflow_groups(const BhrMarchArgs &a, const BhrRayMapArgs &m, bool valid, bool mine, int lane, size_t pix) {
    // the group's flag: the guard kernel's butterfly
    int u = valid && mine ? 1 : 0;
    for (int x = 1; x < a.ss; x <<= 1) u |= __shfl_xor(u, x, BHR_WAVE);
    for (int x = 8; x < 8 * a.ss; x <<= 1) u |= __shfl_xor(u, x, BHR_WAVE);
    const bool over = valid && u != 0;
    const unsigned long long om = __ballot(over);
    if (om) {
        const int first = __ffsll((long long)om) - 1;
        const int km = a.ss - 1, sx = lane & km, sy = (lane >> 3) & km;
        const unsigned long long lead = __ballot(over && sx == 0 && sy == 0);
        unsigned int base = 0;
        if (lane == first) base = atomicAdd(m.over_count, (unsigned int)__popcll(lead) << (2 * a.ss_log2));
        base = __shfl(base, first, BHR_WAVE);
        const int l0 = lane - sx - 8 * sy;
        const unsigned int at = base + ((unsigned int)__popcll(lead & ((1ull << l0) - 1ull)) << (2 * a.ss_log2)) + (unsigned int)((sy << a.ss_log2) + sx);
        // (every group is appended at most once and the list has room for the whole fine plane)
        if (over) m.over_list[at] = (int32_t)pix;
    }
}

// What resolve_store (march_device.h) asks of a ray: the six values it leaves.  In a supersampled shade kernel they come out of
// the lane's records.
struct RayMapValues {
    float v[6];
    __device__ __forceinline__ void values(const BhrMarchArgs &, float bk[3], float dk[3]) const {
        bk[0] = v[0]; bk[1] = v[1]; bk[2] = v[2];
        dk[0] = v[3]; dk[1] = v[4]; dk[2] = v[5];
    }
};
