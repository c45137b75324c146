// march_polar.hip -> march_polar.o: the polarisation's two kernels (bhr_set_polarization; include/bhr.h states the model, DESIGN 4
// "Polarisation"), in a strict object of their own with the flags of march_raymap.o (-ffp-contract=off, no fast-math, the ILP-first
// scheduler): shade_hit is inlined here as it is there, so the accumulator differences this kernel takes are differences of the
// values the shade kernel accumulated, bit for bit.
//
// raymap_stokes_kernel<DIFF> runs behind the shade launch of a map frame with raymap_shade_kernel's mapping -- one lane per pixel,
// an 8x8 tile per wave, tiles row-major -- and walks the lane's records as raymap_shade_records does.  Around each shade_hit it takes
// what the crossing added to the accumulator (its Rec. 709 luma is the crossing's weight c_k) and evaluates the closed-form transport of
// the polarisation vector: in Schwarzschild the unit normal N of the ray's plane is parallel-transported along the ray, so the angle
// between the polarisation vector and N is the same at the gas and at the camera.  No integration, no trigonometric call: a few hundred
// flops per record beside shade_hit's ~700 instructions.  The frame's camera, field and fraction are kernel arguments (scalars); what a
// lane keeps across its records on top of the Shade is I, Q, U, N and the four products that carry (cos psi, sin psi) to the image axes.
// It stores three planes, pixel index j W + i as the map's own: a wave's tile writes 32-byte runs of each.
// shade_hit, apply_g_factor and Ray are called, not edited: no other object's code moves.
//
// stokes_cells_kernel: the means of the three planes over cell x cell pixels, one block of min(256, cell^2) threads per cell.  A lane adds
// its pixels of the cell in row-major order (lane t takes pixels t, t + 256, ...), the lanes of a wave are added by a fixed butterfly, the
// block's waves (one for the 8 x 8 cell, four for the larger ones) through LDS in order: no floating-point atomics, so the grid is the same bits from run to run.
#include "ray_strict.h"

namespace {

template <bool DIFF>
__global__ __launch_bounds__(256) void raymap_stokes_kernel(BhrMarchArgs a, BhrRayMapArgs m, BhrStokesArgs s) {
    const int tile = wave_slot();
    if (tile >= a.n_tiles) return;
    const int lane = threadIdx.x & 63;
    const int i = (tile % a.tiles_x) * 8 + (lane & 7);
    const int j = (tile / a.tiles_x) * 8 + (lane >> 3);
    if (!(i < a.width && j < a.rows)) return;
    const size_t pix = (size_t)j * a.width + i;
    const size_t p = (size_t)m.plane;
    const int count = m.crossings[pix];
    float sI = 0.0f, sQ = 0.0f, sU = 0.0f;
    if (count <= m.slots) {          // a pixel on the overflow list keeps the zeros
        // the camera side: the ray's plane and the image axes
        const V3 C = ld3(a.cp);
        V3 unused_x, unused_y;
        const V3 D = pixel_ray<false>(a, i, j, unused_x, unused_y);
        const V3 CxD = cross(C, D);
        const float cxd = sqrtf(dot(CxD, CxD));
        const bool radial = cxd < 1e-6f * sqrtf(dot(C, C));
        const V3 N = radial ? mk(0.0f, 0.0f, 0.0f) : (1.0f / cxd) * CxD;
        const V3 R = ld3(a.cr);
        const V3 ex = normalized(R - dot(R, D) * D);
        V3 ey = cross(D, ex);
        if (dot(ey, ld3(a.cu)) < 0.0f) ey = mk(-ey.x, -ey.y, -ey.z);
        const V3 M = cross(N, mk(-D.x, -D.y, -D.z));        // N x K_c: f_c = cos psi N + sin psi M
        const float nx = dot(N, ex), ny = dot(N, ey), mx = dot(M, ex), my = dot(M, ey);
        const V3 dn = mk(0.0f, -a.sin_t, a.cos_t);           // the disk normal

        Shade sh;                    // as Ray::init leaves it
        sh.accum = mk(0, 0, 0);
        sh.alpha_total = 0.0f;
        sh.unsure = 0;
        for (int c = 0; c < count; ++c) {
            const float *q = m.hits + (size_t)c * m.comps * p + pix;
            const float hx = q[0], hy = q[p];
            const V3 w = mk(q[2 * p], q[3 * p], q[4 * p]);
            float dxx = 0.0f, dxy = 0.0f, dyx = 0.0f, dyy = 0.0f;
            if (DIFF) { dxx = q[5 * p]; dxy = q[6 * p]; dyx = q[7 * p]; dyy = q[8 * p]; }
            const V3 before = sh.accum;
            shade_hit<DIFF, 0>(a, a, sh, hx, hy, w, dxx, dxy, dyx, dyy);
            const V3 add = sh.accum - before;
            const float ck = 0.2126f * add.x + 0.7152f * add.y + 0.0722f * add.z;
            sI = sI + ck;
            // shade_hit's own test: outside the annulus it returned early and the crossing adds nothing
            const float hit_r = sqrtf(hx * hx + hy * hy);
            if (radial || !(a.r_outer >= hit_r && hit_r >= a.r_inner)) continue;

            // the photon's direction at the gas, in the static observer's frame and in the ray's plane
            const V3 P = mk(hx, hy, hy * a.tan_t);
            const float r_em = sqrtf(dot(P, P));
            const V3 rh = (1.0f / r_em) * P;
            const float r = fmaxf(r_em, BHR_RS + 1e-3f);
            const float sF = sqrtf(1.0f - BHR_RS / r);
            const float wr = dot(w, rh);
            V3 K = (wr / sF) * rh + (w - wr * rh);
            K = normalized(K - dot(K, N) * N);
            // the gas
            V3 vh = cross(rh, dn);
            const float vn = sqrtf(dot(vh, vh));
            if (vn > 1e-6f) vh = mk(vh.x / vn, vh.y / vn, vh.z / vn);
            else vh = mk(0.0f, 1.0f, 0.0f);
            const float omega = sqrtf(0.5f / (r * r * r));
            const float beta = fminf(r * omega / sF, 0.99f);
            const float gamma = 1.0f / sqrtf(1.0f - beta * beta);
            // the photon's direction in the gas frame
            const float kv = dot(K, vh);
            const float inv = 1.0f / (gamma * (1.0f - beta * kv));
            const V3 np = inv * (K + ((gamma - 1.0f) * kv - gamma * beta) * vh);
            // the field and the electric vector
            const V3 B = normalized((s.b[0] * rh + s.b[1] * vh) + s.b[2] * dn);
            const V3 e = cross(np, B);
            const float s2 = dot(e, e);
            if (!(s2 > 0.0f)) continue;
            const V3 eh = (1.0f / sqrtf(s2)) * e;
            // back to the static frame; the conserved angle; the image axes
            const float ev = dot(eh, vh);
            const V3 f = (eh + ((gamma - 1.0f) * ev) * vh) - (gamma * beta * ev) * K;
            const float cpsi = dot(f, N), spsi = dot(f, cross(N, K));
            const float x = cpsi * nx + spsi * mx, y = cpsi * ny + spsi * my;
            const float den = x * x + y * y;
            if (!(den > 0.0f)) continue;
            const float wgt = s.frac * s2 * ck;
            sQ = sQ + wgt * ((x * x - y * y) / den);
            sU = sU + wgt * ((2.0f * x * y) / den);
        }
    }
    s.out[pix] = sI;
    s.out[p + pix] = sQ;
    s.out[2 * p + pix] = sU;
}

__shared__ float g_cell_acc[3][4];

__global__ __launch_bounds__(256) void stokes_cells_kernel(BhrStokesArgs s) {
    const int cell = blockIdx.x;     // gy gw + gx
    if (cell >= s.gw * s.gh) return;
    const int gx = cell % s.gw, gy = cell / s.gw;
    const int x0 = gx * s.cell, y0 = gy * s.cell;
    const int cw = min(s.cell, s.width - x0), ch = min(s.cell, s.rows - y0);      // an edge cell: the pixels it has
    const size_t plane = (size_t)s.width * s.rows;
    const int t = threadIdx.x;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    // the block is min(256, cell^2) threads (bhr_launch_stokes): one wave for the 8 x 8 cell, four for the larger ones
    const int nt = blockDim.x, nw = nt >> 6;
    for (int k = t; k < s.cell * s.cell; k += nt) {
        const int lx = k % s.cell, ly = k / s.cell;
        if (lx < cw && ly < ch) {
            const size_t pix = (size_t)(y0 + ly) * s.width + (x0 + lx);
#pragma unroll
            for (int v = 0; v < 3; ++v) acc[v] = acc[v] + s.out[(size_t)v * plane + pix];
        }
    }
    // the lanes of a wave, then the waves: a fixed order
#pragma unroll
    for (int v = 0; v < 3; ++v) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[v] = acc[v] + __shfl_down(acc[v], off, BHR_WAVE);
    }
    if ((t & 63) == 0) {
#pragma unroll
        for (int v = 0; v < 3; ++v) g_cell_acc[v][t >> 6] = acc[v];
    }
    __syncthreads();
    if (t < 3) {
        float sum = g_cell_acc[t][0];
        for (int w = 1; w < nw; ++w) sum = sum + g_cell_acc[t][w];
        s.cells[(size_t)cell * 3 + t] = sum / (float)(cw * ch);
    }
}

}  // namespace

const void *bhr_stokes_kernel(int32_t diff) { return diff ? (const void *)raymap_stokes_kernel<true> : (const void *)raymap_stokes_kernel<false>; }
const void *bhr_stokes_cells_kernel(void) { return (const void *)stokes_cells_kernel; }
