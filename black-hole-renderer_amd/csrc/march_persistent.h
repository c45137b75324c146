// march_persistent.h -- the march's persistent schedule, over the Ray of the header included before it.
#pragma once

namespace {

// ---------------------------------------------------------------------------
// persistent schedule: waves pull pixels from a queue (8x8-tile-major order, so refilled lanes
// stay spatially coherent) and refill dead lanes when fewer than `refill_below` are alive:
// __ballot gives the live mask, popcount of the lower lanes the slot of each lane that wants work.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool tile_pixel(const BhrMarchArgs &a, unsigned int w, int &i, int &j) {
    unsigned int tile = w >> 6, in = w & 63u;
    if ((int)tile >= a.n_tiles) return false;
    int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    i = tx * 8 + (in & 7);
    j = ty * 8 + (in >> 3);
    return i < a.width && j < a.rows;
}

template <bool DIFF>
__global__ __launch_bounds__(256) void march_persistent_kernel(BhrMarchArgs a, int refill_below) {
    const int lane = threadIdx.x & 63;
    const unsigned int total = (unsigned int)a.n_tiles * 64u;
    Ray<DIFF> ray;
    ray.done = 4;  // empty lane: no pixel, nothing parked, nothing accumulated
    ray.pix = -1;
    ray.n_pend = 0;
    ray.sh.accum = mk(0, 0, 0);
    ray.sh.alpha_total = 0.0f;
    unsigned int executed = 0;
    bool queue_empty = false;

    for (;;) {
        unsigned long long live = __ballot(ray.done == 0);
        int n_live = __popcll(live);
        if (!queue_empty && n_live < refill_below) {
            // retire finished lanes, then hand every non-running lane a new pixel
            for (int k = 0; k < 2; ++k)
                if (__ballot(ray.n_pend > 0 && ray.done != 0)) {
                    if (ray.done != 0) ray.flush_one(a);
                }
            if (ray.done >= 1 && ray.done <= 3) ray.finish(a);
            unsigned long long want = ~live;
            int n_want = 64 - n_live;
            unsigned int base = 0;
            if (lane == 0) base = atomicAdd(a.queue, (unsigned int)n_want);
            base = __shfl(base, 0, BHR_WAVE);
            unsigned long long below = want & ((1ull << lane) - 1ull);
            unsigned int w = base + (unsigned int)__popcll(below);
            if ((want >> lane) & 1ull) {   // running lanes keep their ray
                ray.done = 4;
                ray.pix = -1;
                ray.n_pend = 0;       // a lane that gets no pixel (queue exhausted) must not look as if it had a hit parked
                int i, j;
                if (w < total && tile_pixel(a, w, i, j)) ray.init(a, i, j);
            }
            if (base + (unsigned int)n_want >= total) queue_empty = true;
            live = __ballot(ray.done == 0);
            if (!live && queue_empty) break;
            continue;
        }
        if (!live) {
            for (int k = 0; k < 2; ++k)
                if (__ballot(ray.n_pend > 0)) ray.flush_one(a);
            if (ray.done >= 1 && ray.done <= 3) ray.finish(a);
            break;
        }
        bool blocked = false;
        if (ray.done == 0) {
            blocked = !ray.step(a);
            executed += blocked ? 0u : 1u;
        }
        if (__ballot(blocked || ray.n_pend == 2)) ray.flush_one(a);
    }
    unsigned long long tot = wave_sum_u32(executed);
    if (lane == 0) atomicAdd(a.ray_steps + (size_t)(blockIdx.x & (BHR_STEP_LANES - 1)) * BHR_STEP_STRIDE, tot);
}

}  // namespace
