// march_tile.h -- the march's tile schedule, over the Ray of the header included before it (ray_strict.h or ray_fast.h).
#pragma once

namespace {

// ---------------------------------------------------------------------------
// tile schedule: block = 4 waves = 4 horizontally adjacent 8x8 tiles (32x8 px).
// blockIdx maps to tiles in plain row-major order: the dispatcher deals consecutive blocks
// round-robin over the 8 XCDs, which spreads the expensive rows (those through the photon
// ring) evenly.  An XCD-banded remap was measured and rejected (-13 %: the kernel is VALU
// bound, texture traffic is negligible, and bands of rows differ in cost).
// ---------------------------------------------------------------------------
// The texture kernels are held to 128 VGPRs (4 waves per SIMD): the strict arithmetic is a chain of dependent
// exact-rounding sequences and needs the waves to cover its latency (measured at 4k with AA: 141 VGPRs / 3 waves
// 7.6 ms, 128 / 4 waves 6.7 ms).  The binary64 Disk V2 instantiations take what they need.
// GUARD (the fast list of a hybrid march, fast object only): a lane that came within a guard band of one of the
// algorithm's switches (Shade.unsure) does not write its pixel; it appends it to the context's fix list, which
// march_fix_kernel (strict objects) marches again with the strict Ray.
// SS (supersampled instantiations, a.ss > 1): the tile is one of the fine frame, its k x k groups are resolved in the wave
// (resolve_store); the guard appends whole groups.
// LIST (march_list_kernel, the refinement of an adaptively supersampled frame): the launch's tiles are the fine tiles the detect
// kernel listed (a.tile_order, list_n of them: a count the device holds), and only the k x k groups of refined output pixels
// are marched and stored -- a.fix_list is then the detect kernel's mask, one byte per OUTPUT pixel; the other lanes sit the
// march out like the lanes beyond the frame's edge.  The wave is a tile of the fine frame exactly as in the frame's own
// supersampled kernel, and everything between the two places that name the lane's pixel is that kernel's code: under
// fast-math the form of the code around the march decides how it is contracted and re-associated, and a refined pixel has to
// be the supersampled frame's bit for bit.
__device__ __forceinline__ bool list_refined(const BhrMarchArgs &a, int i, int j) {
    return ((const unsigned char *)a.fix_list)[(size_t)(j >> a.ss_log2) * a.out_width + (i >> a.ss_log2)] != 0;
}

template <bool DIFF, int SRC = 0, bool GUARD = false, bool COSTS = true, bool SS = false, bool LIST = false>
__device__ __forceinline__ void march_tile_body(const BhrMarchArgs &a, const int slot, const int list_n = 0) {
    const int lane = threadIdx.x & 63;
    // one 8x8 tile per wave; `slot` is its position in the launch order
    // tiles are handed out longest first (tile_order: by distance from the image of the hole, where rays take the
    // most steps), so that the launch does not end on a few late, long waves
    // n_list = launch slots of THIS launch: all tiles of the row block, or the sub-list a hybrid launch hands this kernel
    const int tile = slot < (LIST ? list_n : a.n_list) ? (a.tile_order ? a.tile_order[slot] : slot) : a.n_tiles;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int i = tx * 8 + (lane & 7);
    const int j = ty * 8 + (lane >> 3);
    bool valid = tile < a.n_tiles && i < a.width && j < a.rows;
    if (LIST) valid = valid && list_refined(a, i, j);
    // (slot, tile, tx, ty are wave-uniform: march_tile_kernel / march_tile_of_wave hand over wave_slot())

#if BHR_WAVE_STAMPS_BUILD
    const unsigned long long t_start = a.wave_stamps ? __builtin_amdgcn_s_memrealtime() : 0ull;
#endif
    Ray<DIFF, SRC> ray;
    ray.init(a, valid ? i : 0, valid ? j : 0);
    if (!valid) ray.done = 4;
    // Divergent loop: a lane leaves when its ray terminates, the wave leaves when its EXEC mask is
    // empty (the hardware form of "loop while __ballot(alive)").  Written without an inner `if` because
    // hipcc otherwise shuttles the whole ray state through v_mov at every iteration (24 moves/step).
    unsigned int flushes = 0;     // wave-uniform
    // Values that are uniform over the live lanes but read behind the divergent loop (the step count, the
    // number of shading passes) are kept in scalar registers by hipcc and copied into a vector register in EVERY
    // iteration for the lanes that leave (v_mov from an SGPR: 4 issue cycles each).  The lane's own count in a vector
    // register costs one plain v_add.  The shading passes inside the loop are counted only by the instantiations that
    // fill the row-cost profile (COSTS: BHR_ROW_COSTS launches): the plain kernel sits exactly at 80 registers = 6 waves
    // per SIMD, and one more value alive across the loop costs it a wave of occupancy.
    int cnt = 0, passes = 0;
    asm volatile("" : "+v"(cnt));
    if (COSTS) asm volatile("" : "+v"(passes));
    // The loop body twice per trip: the state a step leaves in fresh registers (new position, new plane function) is the
    // next step's input where it stands -- rolled once, hipcc closed every iteration with three v_mov to bring it back to
    // the registers the loop head expects.
#define BHR_FAST_STEP()                                                                                                     \
    ray.step(a);                                                                                                            \
    cnt += 1;                                                                                                               \
    if (ray.full) { /* wave-uniform, a scalar register (Ray::step): some live lane has filled both its parking slots */     \
        asm volatile("" : "+v"(ray.n_pend)); /* the lanes' own n_pend > 0 test stays inside this branch */                  \
        ray.flush_one(a);                                                                                                   \
        ray.full = false;                                                                                                   \
        if (COSTS) passes += 1;                                                                                             \
    }
    while (ray.done == 0) {
        BHR_FAST_STEP()
        if (ray.done != 0) break;
        BHR_FAST_STEP()
    }
#undef BHR_FAST_STEP
    ray.step_count = cnt;
    if (cnt > 0) ray.settle(a);
    else ray.done = 3;               // no step taken (max_iter <= 0, or no ray: those lanes store nothing)
    if (COSTS) {   // the lanes that were alive at the wave's last pass have seen them all
        int m = passes;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, BHR_WAVE));
        flushes = (unsigned int)m;
    }
    if (__ballot(ray.n_pend > 0)) { ray.flush_one(a); flushes += 1u; }
    if (__ballot(ray.n_pend > 0)) { ray.flush_one(a); flushes += 1u; }
    {
        // The lane's pixel, worked out AGAIN from the thread index behind an optimisation barrier: nothing that is
        // only needed here (pixel index, validity, store addresses) stays in a register across the march loop -- the
        // strict AA kernel spilled five such values at 128 VGPRs (round 2: 6 spills, 28 B of scratch).
        int t2 = threadIdx.x;
        asm volatile("" : "+v"(t2));
        const int i2 = tx * 8 + (t2 & 7), j2 = ty * 8 + ((t2 & 63) >> 3);
        bool valid2 = tile < a.n_tiles && i2 < a.width && j2 < a.rows;
        if (LIST) valid2 = valid2 && list_refined(a, i2, j2);
        bool again = false;
        if (GUARD) {
            again = valid2 && ray.sh.unsure != 0;
            if (SS) {                                  // a group is re-marched whole when any of its rays is flagged
                int u = again ? 1 : 0;
                for (int m = 1; m < a.ss; m <<= 1) u |= __shfl_xor(u, m, BHR_WAVE);
                for (int m = 8; m < 8 * a.ss; m <<= 1) u |= __shfl_xor(u, m, BHR_WAVE);
                again = valid2 && u != 0;
            }
            const unsigned long long m = __ballot(again);
            if (m) {                                   // wave-aggregated append
                const int lane2 = t2 & 63, first = __ffsll((long long)m) - 1;
                unsigned int base = 0, at;
                if (SS) {
                    // k^2 consecutive entries per group, in sub-sample order (sy k + sx), groups in the order of their (0, 0) lanes
                    const int km = a.ss - 1, sx = lane2 & km, sy = (lane2 >> 3) & km;
                    const unsigned long long lead = __ballot(again && sx == 0 && sy == 0);
                    if (lane2 == first) base = atomicAdd(a.fix_count, (unsigned int)__popcll(lead) << (2 * a.ss_log2));
                    base = __shfl(base, first, BHR_WAVE);
                    const int l0 = lane2 - sx - 8 * sy;
                    at = base + ((unsigned int)__popcll(lead & ((1ull << l0) - 1ull)) << (2 * a.ss_log2)) + (unsigned int)((sy << a.ss_log2) + sx);
                } else {
                    if (lane2 == first) base = atomicAdd(a.fix_count, (unsigned int)__popcll(m));
                    base = __shfl(base, first, BHR_WAVE);
                    at = base + (unsigned int)__popcll(m & ((1ull << lane2) - 1ull));
                }
                // (with SS the count and the capacity are multiples of k^2: a group is listed whole or not at all)
                if (again && at < (unsigned int)a.fix_cap) a.fix_list[at] = j2 * a.width + i2;
                else again = false;                    // list full: the fast pixel stands
            }
            if (again) ray.step_count = 0;             // its steps are counted by the strict re-march
        }
        if (SS) resolve_store(a, ray, valid2, valid2 && !again, i2, j2, 8);
        else if (valid2 && !again) ray.finish_at(a, i2, j2);
    }
    // a lane executes one step per loop iteration: its step count is the number of steps it executed (0: no ray)
    unsigned long long tot = wave_sum_u32((unsigned int)ray.step_count);
    if (lane == 0) {
        atomicAdd(a.ray_steps + (size_t)(blockIdx.x & (BHR_STEP_LANES - 1)) * BHR_STEP_STRIDE, tot);
        // BHR_ROW_COSTS: cost profile over tile rows = ray-steps + the wave's shading passes, each priced as
        // BHR_FLUSH_COST wave-steps (a pass is ~1000 instructions, a strict step ~220)
        if (a.row_steps && tile < a.n_tiles) atomicAdd(a.row_steps + ty, tot + (unsigned long long)flushes * (64u * BHR_FLUSH_COST));
#if BHR_WAVE_STAMPS_BUILD
        if (a.wave_stamps && slot < a.n_tiles) {          // diagnostic: when this wave lived (100 MHz ticks) and what it did
            unsigned long long *w = a.wave_stamps + (size_t)slot * 4;
            w[0] = t_start;
            w[1] = __builtin_amdgcn_s_memrealtime();
            w[2] = tot | ((unsigned long long)flushes << 40);
            w[3] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // HW_ID
        }
#endif
    }
}

template <bool DIFF, int SRC = 0, bool COSTS = false>
__global__ __launch_bounds__(256) void march_tile_kernel(BhrMarchArgs a) {
    march_tile_body<DIFF, SRC, false, COSTS>(a, wave_slot());
}

// The supersampled twins of the tile kernels (a.ss > 1) are instantiations of their own: the k = 1 kernels stay as they were.
template <bool DIFF, int SRC = 0>
__global__ __launch_bounds__(256) void march_tile_ss_kernel(BhrMarchArgs a) {
    march_tile_body<DIFF, SRC, false, false, true>(a, wave_slot());
}

// The refinement of an adaptively supersampled frame: the fine tiles the detect kernel listed, marched by the tile body in its
// LIST form (march.o, march_strict.o, march_strict_ilp.o).  The host does not know the list's length (frames stay in flight):
// like the fix kernel it is launched with a grid for the list's capacity -- every tile of the fine frame -- and the waves beyond
// the count the detect kernel left exit at once.  No loop over the list around the body: in the fast object a trip loop changed how the march's
// arithmetic was contracted (the loop-invariant parts of the ray set-up were hoisted and re-associated).
template <bool DIFF, int SRC>
__global__ __launch_bounds__(256) void march_list_kernel(BhrMarchArgs a) {
    const int wave = wave_slot();
    int n = (int)__builtin_amdgcn_readfirstlane(*a.fix_count);
    if (n > a.n_list) n = a.n_list;
    if (wave >= n) return;
    march_tile_body<DIFF, SRC, false, false, true, true>(a, wave, n);
}

}  // namespace
