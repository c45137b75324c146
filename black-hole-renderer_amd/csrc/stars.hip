// stars.hip -> stars.o: the point stars' gather kernel (bhr_set_stars; include/bhr.h states the model, DESIGN 4 "Point stars"),
// in a strict object of its own (-ffp-contract=off, no fast-math): what is written here is what is rounded.
//
// stars_gather_kernel<ROT> turns the map's STATUS and direction planes, the view's camera block and the binned catalogue into the
// star plane S.  A gather, no floating-point atomics:
//   * a block of 256 lanes owns 16 x 16 CELLS, one lane per cell, and stores the 15 x 15 PIXELS that have all four of their cells
//     among them (the issue's 16 x 16 pixels over 17 x 17 cells needs 289 cells per 256 lanes: a second pass with 33 lanes live,
//     twice the time for 14 % more pixels; 16 x 16 cells keep every lane busy once, and a cell column and row are formed twice);
//   * the 17 x 17 pixel centres those cells have as corners -- the tile plus its halo -- are staged through LDS once: status,
//     escape direction (turned about z by (rot_c, rot_s) for ROT, the shade kernel's two products and a sum) and the camera-side
//     direction pixel_ray gives.  Planar, 289 words per plane; a lane reads its four corners at words 17 ly + lx (+ 1, + 17, + 18):
//     a 32-lane half covers two rows, words 0 .. 15 and 17 .. 32, one two-way conflict (word 32 on word 0's bank), else none;
//   * a lane forms its cell's twelve corner sums (4 corners x RGB) in registers -- T0's stars, then T1's, each in the catalogue's
//     binned order -- and leaves them in LDS, a word per lane and sum (conflict free);
//   * a pixel then adds its four cells in the fixed order (j-1, i-1), (j-1, i), (j, i-1), (j, i).
// A triangle visits the bins under its bounding cap: centred on normalize(e_a + e_b + e_c), radius the largest vertex angle, padded
// by 1 % and 2e-3 rad against the f32 acos (error ~3e-4 near 1).  A spherical triangle with sides under 60 degrees lies inside that cap
// (a cap below a hemisphere is convex).  The cap takes all longitudes where it touches a pole, and wraps in longitude.  Of the stars
// in those bins -- a bin is degrees wide, a triangle a pixel -- all but a few lie outside the cap itself: they are dropped on their
// angle to the cap's centre (the padding, 2e-6 in the cosine at the least, is far above that product's rounding) before the inside test.
#include "ray_strict.h"       // march_device.h under the strict key: V3, pixel_ray, pymod

namespace {

#define ST_CELLS 16                  // cells per block side
#define ST_PIX (ST_CELLS - 1)        // pixels per block side
#define ST_STAGE (ST_CELLS + 1)      // staged pixel centres per block side
#define ST_NSTAGE (ST_STAGE * ST_STAGE)

__device__ __forceinline__ void star_turn_xy(float c, float s, float &x, float &y) {
    const float xr = c * x - s * y, yr = s * x + c * y;
    x = xr;
    y = yr;
}

// Van Oosterom and Strackee, the triple product on differences
__device__ __forceinline__ float solid_angle(V3 a, V3 b, V3 c) {
    const float num = fabsf(dot(a, cross(b - a, c - a)));
    const float den = 1.0f + dot(a, b) + dot(b, c) + dot(c, a);
    return 2.0f * atan2f(num, den);
}

// The deposits of every catalogue star inside the triangle (ea, eb, ec) onto the cell's four corner sums acc[corner][channel],
// corners P00, P10, P01, P11.  second: the triangle is T1 = (P11, P01, P10), else T0 = (P00, P10, P01).
__device__ __forceinline__ void triangle_deposits(const BhrStarsArgs &s, bool second, V3 ea, V3 eb, V3 ec, V3 na, V3 nb, V3 nc, float acc[4][3],
                                                  unsigned int &images, unsigned int &capped, unsigned int &skipped) {
    const float span = fminf(fminf(dot(ea, eb), dot(eb, ec)), dot(ec, ea));
    if (!(span >= s.cos_span)) {
        skipped += 1;
        return;
    }
    const float o_sky = solid_angle(ea, eb, ec), o_cam = solid_angle(na, nb, nc);
    const float mag = o_cam / o_sky;
    if (mag > s.max_mag) capped += 1;
    const float q = fminf(mag, s.max_mag) / (2.0f * o_cam);     // a deposit is Phi q
    // the bounding cap
    const V3 sum = (ea + eb) + ec;
    const V3 m = normalized(sum);
    const float cr = fminf(fminf(fminf(dot(m, ea), dot(m, eb)), dot(m, ec)), 1.0f);
    const float rho = acosf(cr) * 1.01f + 2e-3f;
    const float cos_cap = cosf(rho);         // a star outside the padded cap is outside the triangle: three products instead of three determinants
    const float theta = acosf(fminf(fmaxf(m.z, -1.0f), 1.0f));
    const float t_lo = theta - rho, t_hi = theta + rho;
    const int nt = s.bins_theta, np = s.bins_phi;
    const int t0 = min(max((int)floorf(t_lo / BHR_PI_F * (float)nt), 0), nt - 1);
    const int t1 = min(max((int)floorf(t_hi / BHR_PI_F * (float)nt), 0), nt - 1);
    int p0 = 0, p1 = np - 1;
    const float s_theta = sqrtf(fmaxf(1.0f - m.z * m.z, 0.0f)), s_rho = sinf(rho);
    if (t_lo > 0.0f && t_hi < BHR_PI_F && s_rho < s_theta) {
        const float dphi = asinf(s_rho / s_theta) + 2e-3f;
        float phi = atan2f(m.y, m.x);
        if (phi < 0) phi += BHR_TWO_PI_F;
        const int q0 = (int)floorf((phi - dphi) / BHR_TWO_PI_F * (float)np);
        const int q1 = (int)floorf((phi + dphi) / BHR_TWO_PI_F * (float)np);
        if (q1 - q0 + 1 < np) {          // else: every longitude, each bin once
            p0 = q0;
            p1 = q1;
        }
    }
    for (int t = t0; t <= t1; ++t) {
        for (int p = p0; p <= p1; ++p) {
            const int bin = t * np + pymod(p, np);
            const int k1 = s.off[bin + 1];
            for (int k = s.off[bin]; k < k1; ++k) {
                const float *r = s.rec + (size_t)k * 6;
                const V3 u = mk(r[0], r[1], r[2]);
                if (dot(u, m) < cos_cap) continue;
                const V3 da = ea - u, db = eb - u, dc = ec - u;
                const float sc = dot(u, cross(da, db)), sa = dot(u, cross(db, dc)), sb = dot(u, cross(dc, da));
                const bool in = ((sa >= 0.0f && sb >= 0.0f && sc >= 0.0f) || (sa <= 0.0f && sb <= 0.0f && sc <= 0.0f)) && dot(u, sum) > 0.0f;
                const float tot = (sa + sb) + sc;
                if (!in || tot == 0.0f) continue;
                const float wa = sa / tot, wb = sb / tot, wc = sc / tot;
                // the image in the cell: T0 = P00 + wb (1, 0) + wc (0, 1); T1: P11 (1, 1), P01 (0, 1), P10 (1, 0)
                const float fx = second ? wa + wc : wb, fy = second ? wa + wb : wc;
                const float w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
                images += 1;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float d = r[3 + c] * q;
                    acc[0][c] = acc[0][c] + d * w00;
                    acc[1][c] = acc[1][c] + d * w10;
                    acc[2][c] = acc[2][c] + d * w01;
                    acc[3][c] = acc[3][c] + d * w11;
                }
            }
        }
    }
}

__shared__ float g_st_e[3][ST_NSTAGE];      // staged escape directions ...
__shared__ float g_st_n[3][ST_NSTAGE];      // ... camera-side directions ...
__shared__ int g_st_status[ST_NSTAGE];      // ... and fates (0 beyond the frame)
__shared__ float g_st_cell[12][256];        // the cells' corner sums: [corner * 3 + channel][lane]
__shared__ unsigned int g_st_counts[3];

template <bool ROT>
__global__ __launch_bounds__(256) void stars_gather_kernel(BhrMarchArgs a, BhrStarsArgs s) {
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ST_PIX, y0 = blockIdx.y * ST_PIX;     // the block's first pixel
    if (tid < 3) g_st_counts[tid] = 0u;
    // stage pixel centres (x0 - 1 .. x0 + 15) x (y0 - 1 .. y0 + 15)
    for (int q = tid; q < ST_NSTAGE; q += 256) {
        const int i = x0 - 1 + q % ST_STAGE, j = y0 - 1 + q / ST_STAGE;
        int st = 0;
        V3 e = mk(0.0f, 0.0f, 0.0f), n = mk(0.0f, 0.0f, 0.0f);
        if (i >= 0 && i < a.width && j >= 0 && j < a.rows) {
            const size_t pix = (size_t)j * a.width + i;
            st = s.status[pix];
            e = mk(s.dir[pix], s.dir[(size_t)s.plane + pix], s.dir[2 * (size_t)s.plane + pix]);
            if (ROT) star_turn_xy(s.rot_c, s.rot_s, e.x, e.y);
            V3 unused_x, unused_y;
            n = pixel_ray<false>(a, i, j, unused_x, unused_y);
        }
        g_st_status[q] = st;
        g_st_e[0][q] = e.x; g_st_e[1][q] = e.y; g_st_e[2][q] = e.z;
        g_st_n[0][q] = n.x; g_st_n[1][q] = n.y; g_st_n[2][q] = n.z;
    }
    __syncthreads();

    // the lane's cell: corners at staged (lx, ly), (lx + 1, ly), (lx, ly + 1), (lx + 1, ly + 1)
    const int lx = tid & (ST_CELLS - 1), ly = tid >> 4;
    float acc[4][3] = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    unsigned int images = 0, capped = 0, skipped = 0;
    {
        const int q00 = ly * ST_STAGE + lx, q10 = q00 + 1, q01 = q00 + ST_STAGE, q11 = q01 + 1;
        const bool s00 = g_st_status[q00] == 1, s10 = g_st_status[q10] == 1, s01 = g_st_status[q01] == 1, s11 = g_st_status[q11] == 1;
        if (s10 && s01 && (s00 || s11)) {
            const V3 e10 = mk(g_st_e[0][q10], g_st_e[1][q10], g_st_e[2][q10]), e01 = mk(g_st_e[0][q01], g_st_e[1][q01], g_st_e[2][q01]);
            const V3 n10 = mk(g_st_n[0][q10], g_st_n[1][q10], g_st_n[2][q10]), n01 = mk(g_st_n[0][q01], g_st_n[1][q01], g_st_n[2][q01]);
            if (s00) {
                const V3 e00 = mk(g_st_e[0][q00], g_st_e[1][q00], g_st_e[2][q00]), n00 = mk(g_st_n[0][q00], g_st_n[1][q00], g_st_n[2][q00]);
                triangle_deposits(s, false, e00, e10, e01, n00, n10, n01, acc, images, capped, skipped);
            }
            if (s11) {
                const V3 e11 = mk(g_st_e[0][q11], g_st_e[1][q11], g_st_e[2][q11]), n11 = mk(g_st_n[0][q11], g_st_n[1][q11], g_st_n[2][q11]);
                triangle_deposits(s, true, e11, e01, e10, n11, n01, n10, acc, images, capped, skipped);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) g_st_cell[k * 3 + c][tid] = acc[k][c];
    // the counts: a cell in the block's first column or row is the last one of the block before it, and counted there
    if (lx > 0 && ly > 0) {
        if (images) atomicAdd(&g_st_counts[0], images);
        if (capped) atomicAdd(&g_st_counts[1], capped);
        if (skipped) atomicAdd(&g_st_counts[2], skipped);
    }
    __syncthreads();
    if (tid < 3 && g_st_counts[tid]) atomicAdd(s.counts + tid, g_st_counts[tid]);

    // pixel (x0 + lx, y0 + ly): P11 of cell (lx, ly), P01 of (lx + 1, ly), P10 of (lx, ly + 1), P00 of (lx + 1, ly + 1)
    const int i = x0 + lx, j = y0 + ly;
    if (lx < ST_PIX && ly < ST_PIX && i < a.width && j < a.rows) {
        const int c0 = tid, c1 = tid + 1, c2 = tid + ST_CELLS, c3 = tid + ST_CELLS + 1;
        float *o = s.out + ((size_t)j * a.width + i) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = g_st_cell[3 * 3 + c][c0];
            v = v + g_st_cell[2 * 3 + c][c1];
            v = v + g_st_cell[1 * 3 + c][c2];
            v = v + g_st_cell[0 * 3 + c][c3];
            o[c] = v;
        }
    }
}

}  // namespace

const void *bhr_stars_kernel(int32_t rot) { return rot ? (const void *)stars_gather_kernel<true> : (const void *)stars_gather_kernel<false>; }
