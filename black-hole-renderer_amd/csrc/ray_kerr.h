// ray_kerr.h -- the Kerr Ray of the march (march_kerr.o; see march_device.h): a spinning hole in Kerr-Schild coordinates.
//
// Units r_s = 1, M = 1/2; a = A M is the spin parameter (kerr(a).kerr_a), the spin axis is z = the normal of the untilted disk.
// With rho2 = x.x, w = rho2 - a^2 and S = sqrt(w^2 + 4 a^2 z^2):
//   r^2 = (w + S) / 2               (the Kerr-Schild radius; S = 2 r^2 - w = r^2 + a^2 cos^2 theta, so r^4 + a^2 z^2 = r^2 S)
//   f   = r_s r^3 / (r^4 + a^2 z^2) = r / S
//   l   = ((r x + a y) / Q, (r y - a x) / Q, z / r),   Q = r^2 + a^2
//   H   = (p.p - 1) / 2 - f (1 + l.p)^2 / 2            (p_t = -1)
//   dx/dl = p - f u l,   u = 1 + l.p
//   dp/dl = -grad_x H = (u^2 / 2) grad f + f u grad (l.p)
//   grad r = (r^2 x + a^2 z e_z) / (r S),   grad S = (2 w x + 4 a^2 z e_z) / S,   grad f = (grad r - f grad S) / S
//   grad (l.p) = ((r p_x - a p_y) / Q, (a p_x + r p_y) / Q, p_z / r) + (d(l.p)/dr) grad r
//   d(l.p)/dr  = (x p_x + y p_y) / Q - 2 r N / Q^2 - z p_z / r^2,   N = r (x p_x + y p_y) + a (y p_x - x p_y)
// tests/kerr_ref.py states the same model in NumPy (rhs()) and checks the gradients against central differences of H.
//
// The state is (x, p), six components, RK4 with the reference's adaptive step on the Kerr-Schild radius.  What is conserved
// along a ray (E = 1, L_z) is not carried.  The traced ray is the future-directed photon that leaves the camera with its
// coordinate velocity along the pixel direction; by time reversal and a -> -a that is the image of a hole that turns with
// this project's disk (v_hat = r_hat x n, clockwise seen from +z) for A > 0.  DESIGN.md "Kerr" has the conventions.
//
// One disk source, the texture.  The Ray's second parameter, the disk source everywhere else, selects the disk's redshift
// here: Ray<DIFF, 0> has the reference's g-factor model with Kerr's orbital frequency, Ray<DIFF, KERR_EXACT> the g-factor of
// the Kerr metric (kerr_g_exact below; bhr_set_redshift).  The march is one and the same; the two differ in what a crossing
// parks and in how its shade makes g.
//
// Ray differentials (DIFF, bhr_set_kerr_anti_alias): beside (x, p) the ray carries two tangents (xi, pi), one per pixel axis,
// d(x, p) / d(pixel).  They obey the variational equations of the system above, which are kerr_rhs differentiated line by
// line in forward mode (kerr_rhs_tangent: every reciprocal and root it needs is one the primal stage has already made), and
// are integrated by the same RK4 step with the same h, h being a constant of the step as in the strict Ray's variational pair.
// Seeds: xi = 0, and pi the differential of the camera's momentum p = s d + f Lam l under d -> d + delta d, with delta d
// pixel_ray<true>'s and f, l constants of the camera.  A crossing parks the x and y components of the two new xi (the
// reference's convention: the end of the crossing step, not projected onto the plane) and its shade picks the mip level
// from them (kerr_lod).  The primal march is not touched: Ray<true, RS> marches the bits Ray<false, RS> marches.
// tests/kerr_aa_ref.py states the same in NumPy.
#pragma once
#define BHR_RAY_STRICT 1   // the shared samplers in the reference's evaluation order (march_device.h: BHR_BILERP)
#include "march_device.h"

namespace {

// The kernels of this object take the march's block with the hole's numbers behind it (bhr_internal.h: BhrKerrMarchArgs) and hand
// it to the shared schedule as the BhrMarchArgs it is; the Kerr code reads the tail through this.
__device__ __forceinline__ const BhrKerrMarchArgs &kerr(const BhrMarchArgs &a) { return static_cast<const BhrKerrMarchArgs &>(a); }
// ... and the exact-redshift kernels' block with the ISCO's numbers behind that (BhrKerrExactMarchArgs); theirs alone
__device__ __forceinline__ const BhrKerrExactMarchArgs &kerr_exact(const BhrMarchArgs &a) { return static_cast<const BhrKerrExactMarchArgs &>(a); }
constexpr int KERR_EXACT = 1;   // Ray<DIFF, KERR_EXACT>: the exact redshift

// v_rsq of x and v_rcp of y back to back (march_device.h: rsq2 / rcp2 say why)
__device__ __forceinline__ void rsq_rcp(float x, float y, float &rs, float &rc) {
    asm("v_rsq_f32 %0, %2\n\tv_rcp_f32 %1, %3\n\ts_nop 0" : "=&v"(rs), "=&v"(rc) : "v"(x), "v"(y));
}
// sqrt(x) and 1 / sqrt(x) from the seed y = v_rsq(x): one Newton step each from the one residual e = 1 - x y^2
__device__ __forceinline__ void sqrt_both(float x, float y, float &s, float &inv) {
    const float s0 = x * y;
    const float e = fmaf(-s0, y, 1.0f);
    s = fmaf(0.5f * s0, e, s0);
    inv = fmaf(0.5f * y, e, y);
}

// The Kerr-Schild geometry at a point: what the right-hand side and the termination test share.
struct KerrGeom {
    float w, S, iS, r2;
};
__device__ __forceinline__ KerrGeom kerr_geom(float a2, V3 x) {
    KerrGeom g;
    g.w = dot(x, x) - a2;
    const float S2 = fmaf(g.w, g.w, 4.0f * a2 * (x.z * x.z));
    sqrt_both(S2, q_rsq(S2), g.S, g.iS);
    g.r2 = 0.5f * (g.w + g.S);
    return g;
}
// What a right-hand side evaluation leaves behind for the tangents of the same stage (kerr_rhs_tangent)
struct KerrStage {
    float w, S, iS, r2, Q, r, ir, iQ, f, u, fu, gg, sxy, N, dr, c1;
    V3 l, gr, gS, gf, gl;
};
// dx/dl and dp/dl at (x, p), with the stage's record: kerr_rhs below, value for value
__device__ __forceinline__ void kerr_rhs_stage(float a, float a2, V3 x, V3 p, V3 &v, V3 &dp, KerrStage &s) {
    const KerrGeom g = kerr_geom(a2, x);
    const float Q = g.r2 + a2;
    float y_r, y_q;
    rsq_rcp(g.r2, Q, y_r, y_q);
    float r, ir;
    sqrt_both(g.r2, y_r, r, ir);
    const float iQ = rcp_rn_s(Q, y_q);
    const float f = r * g.iS;
    const V3 l = mk((r * x.x + a * x.y) * iQ, (r * x.y - a * x.x) * iQ, x.z * ir);
    const float u = 1.0f + dot(l, p);
    const float fu = f * u;
    v = mk(p.x - fu * l.x, p.y - fu * l.y, p.z - fu * l.z);
    const float gg = ir * g.iS;
    const V3 gr = mk(g.r2 * x.x * gg, g.r2 * x.y * gg, Q * x.z * gg);
    const float w2 = 2.0f * g.w;
    const V3 gS = mk(w2 * x.x * g.iS, w2 * x.y * g.iS, (w2 + 4.0f * a2) * x.z * g.iS);
    const V3 gf = mk((gr.x - f * gS.x) * g.iS, (gr.y - f * gS.y) * g.iS, (gr.z - f * gS.z) * g.iS);
    const float sxy = x.x * p.x + x.y * p.y;
    const float N = r * sxy + a * (x.y * p.x - x.x * p.y);
    const float dr = sxy * iQ - 2.0f * r * N * iQ * iQ - x.z * p.z * ir * ir;
    const V3 gl = mk((r * p.x - a * p.y) * iQ + dr * gr.x, (a * p.x + r * p.y) * iQ + dr * gr.y, p.z * ir + dr * gr.z);
    const float c1 = 0.5f * u * u;
    dp = mk(c1 * gf.x + fu * gl.x, c1 * gf.y + fu * gl.y, c1 * gf.z + fu * gl.z);
    s.w = g.w; s.S = g.S; s.iS = g.iS; s.r2 = g.r2; s.Q = Q; s.r = r; s.ir = ir; s.iQ = iQ; s.f = f; s.u = u; s.fu = fu;
    s.gg = gg; s.sxy = sxy; s.N = N; s.dr = dr; s.c1 = c1; s.l = l; s.gr = gr; s.gS = gS; s.gf = gf; s.gl = gl;
}
// ... for a ray without differentials: the same lines without the stage's record (kept as they were written: the objects that
// inline it stay the bytes they are)
__device__ __forceinline__ void kerr_rhs(float a, float a2, V3 x, V3 p, V3 &v, V3 &dp, float &r_out) {
    const KerrGeom g = kerr_geom(a2, x);
    const float Q = g.r2 + a2;
    float y_r, y_q;
    rsq_rcp(g.r2, Q, y_r, y_q);
    float r, ir;
    sqrt_both(g.r2, y_r, r, ir);
    const float iQ = rcp_rn_s(Q, y_q);
    r_out = r;
    const float f = r * g.iS;
    const V3 l = mk((r * x.x + a * x.y) * iQ, (r * x.y - a * x.x) * iQ, x.z * ir);
    const float u = 1.0f + dot(l, p);
    const float fu = f * u;
    v = mk(p.x - fu * l.x, p.y - fu * l.y, p.z - fu * l.z);
    const float gg = ir * g.iS;
    const V3 gr = mk(g.r2 * x.x * gg, g.r2 * x.y * gg, Q * x.z * gg);
    const float w2 = 2.0f * g.w;
    const V3 gf = mk((gr.x - f * (w2 * x.x * g.iS)) * g.iS, (gr.y - f * (w2 * x.y * g.iS)) * g.iS,
                     (gr.z - f * ((w2 + 4.0f * a2) * x.z * g.iS)) * g.iS);
    const float sxy = x.x * p.x + x.y * p.y;
    const float N = r * sxy + a * (x.y * p.x - x.x * p.y);
    const float dr = sxy * iQ - 2.0f * r * N * iQ * iQ - x.z * p.z * ir * ir;
    const V3 gl = mk((r * p.x - a * p.y) * iQ + dr * gr.x, (a * p.x + r * p.y) * iQ + dr * gr.y, p.z * ir + dr * gr.z);
    const float c1 = 0.5f * u * u;
    dp = mk(c1 * gf.x + fu * gl.x, c1 * gf.y + fu * gl.y, c1 * gf.z + fu * gl.z);
}
// The tangent of kerr_rhs_stage at (x, p) along (xi, pi): d(dx/dl) and d(dp/dl), every line of the primal differentiated in
// forward mode with the stage's own values (s) -- no reciprocal, no root:
//   d(1/S) = -dS / S^2, d(1/Q) = -dQ / Q^2, d(1/r) = -dr / r^2, and for a quotient n / D kept as n iD: d(n iD) = (dn - (n iD) dD) iD
__device__ __forceinline__ void kerr_rhs_tangent(float a, float a2, V3 x, V3 p, const KerrStage &s, V3 xi, V3 pi, V3 &tv, V3 &tdp) {
    const float dw = 2.0f * dot(x, xi);
    const float dS = (s.w * dw + 4.0f * a2 * x.z * xi.z) * s.iS;
    const float dr2 = 0.5f * (dw + dS);                   // = dQ
    const float dr = 0.5f * dr2 * s.ir;
    const float diS = -dS * s.iS * s.iS;
    const float diQ = -dr2 * s.iQ * s.iQ;
    const float dir = -dr * s.ir * s.ir;
    const float df = dr * s.iS + s.r * diS;
    const V3 dl = mk((dr * x.x + s.r * xi.x + a * xi.y - s.l.x * dr2) * s.iQ, (dr * x.y + s.r * xi.y - a * xi.x - s.l.y * dr2) * s.iQ,
                     (xi.z - s.l.z * dr) * s.ir);
    const float du = dot(dl, p) + dot(s.l, pi);
    const float dfu = df * s.u + s.f * du;
    tv = mk(pi.x - dfu * s.l.x - s.fu * dl.x, pi.y - dfu * s.l.y - s.fu * dl.y, pi.z - dfu * s.l.z - s.fu * dl.z);
    const float dgg = dir * s.iS + s.ir * diS;
    const V3 dgr = mk((dr2 * x.x + s.r2 * xi.x) * s.gg + s.r2 * x.x * dgg, (dr2 * x.y + s.r2 * xi.y) * s.gg + s.r2 * x.y * dgg,
                      (dr2 * x.z + s.Q * xi.z) * s.gg + s.Q * x.z * dgg);
    const float w2 = 2.0f * s.w, dw2 = 2.0f * dw, w4 = w2 + 4.0f * a2;
    const V3 dgS = mk((dw2 * x.x + w2 * xi.x) * s.iS + w2 * x.x * diS, (dw2 * x.y + w2 * xi.y) * s.iS + w2 * x.y * diS,
                      (dw2 * x.z + w4 * xi.z) * s.iS + w4 * x.z * diS);
    const V3 dgf = mk((dgr.x - df * s.gS.x - s.f * dgS.x - s.gf.x * dS) * s.iS, (dgr.y - df * s.gS.y - s.f * dgS.y - s.gf.y * dS) * s.iS,
                      (dgr.z - df * s.gS.z - s.f * dgS.z - s.gf.z * dS) * s.iS);
    const float dsxy = xi.x * p.x + x.x * pi.x + xi.y * p.y + x.y * pi.y;
    const float dN = dr * s.sxy + s.r * dsxy + a * (xi.y * p.x + x.y * pi.x - xi.x * p.y - x.x * pi.y);
    const float ddr = dsxy * s.iQ + s.sxy * diQ - 2.0f * (dr * s.N + s.r * dN) * s.iQ * s.iQ - 4.0f * s.r * s.N * s.iQ * diQ
                      - (xi.z * p.z + x.z * pi.z) * s.ir * s.ir - 2.0f * x.z * p.z * s.ir * dir;
    const V3 dgl = mk((dr * p.x + s.r * pi.x - a * pi.y) * s.iQ + (s.r * p.x - a * p.y) * diQ + ddr * s.gr.x + s.dr * dgr.x,
                      (a * pi.x + dr * p.y + s.r * pi.y) * s.iQ + (a * p.x + s.r * p.y) * diQ + ddr * s.gr.y + s.dr * dgr.y,
                      pi.z * s.ir + p.z * dir + ddr * s.gr.z + s.dr * dgr.z);
    const float dc1 = s.u * du;
    tdp = mk(dc1 * s.gf.x + s.c1 * dgf.x + dfu * s.gl.x + s.fu * dgl.x, dc1 * s.gf.y + s.c1 * dgf.y + dfu * s.gl.y + s.fu * dgl.y,
             dc1 * s.gf.z + s.c1 * dgf.z + dfu * s.gl.z + s.fu * dgl.z);
}
__device__ __forceinline__ float kerr_radius(float a2, V3 x) {
    const KerrGeom g = kerr_geom(a2, x);
    return sqrt_rn(g.r2);
}

// Kerr's orbital frequency sqrt(M) / (r^1.5 + a sqrt(M)) with the reference's guard: sqrt(0.5 / (r^3 + 1e-6)) at a = 0
__device__ __forceinline__ float kerr_omega(float r_safe, float a) {
    const float sm = 0.70710678118654752f;   // sqrt(M)
    return sm / (sqrtf(r_safe * r_safe * r_safe + 1e-6f) + a * sm);
}

// _sample_disk (render.py:2568-2600) at level 0 with the Boyer-Lindquist hit radius and Kerr's Omega in the roll
// (march_device.h: sample_disk_level is the Schwarzschild sampler and stays as it is)
// f: the block the fields that are a FRAME's own are read from -- t_offset here, cp in the g-factors below -- `a` itself in every
// march and every map frame (the overloads without it).  A shutter frame from the Kerr map shades one set of records as several
// frames and hands over a bare BhrMarchArgs that holds each sample's four floats and nothing else (march_kerr_raymap.hip):
// ONLY f.t_offset and f.cp may be read through f, and kerr(a) / kerr_exact(a) stay on `a` -- f is not inside a Kerr block.
// A BhrMarchArgs and not a type of its own for march_device.h's reason (shade_hit): read through the same struct type the
// fields keep their access metadata and every existing Kerr kernel compiles to the bytes it had (tools/code_object_diff.py;
// profiles/kerr_map_shutter_code_objects.txt is the last run).
__device__ __forceinline__ float4 kerr_sample_disk(const BhrMarchArgs &a, const BhrMarchArgs &f, float hit_x, float hit_y, float hit_r) {
    const BhrScene &sc = a.sc;
    float phi = atan2f(hit_y, hit_x);
    const float r_safe = fmaxf(hit_r, 1e-3f);
    phi = phi + f.t_offset * kerr_omega(r_safe, kerr(a).kerr_a);
    while (phi < 0) phi += BHR_TWO_PI_F;
    while (phi >= BHR_TWO_PI_F) phi -= BHR_TWO_PI_F;
    const float u = phi / BHR_TWO_PI_F * (float)sc.n_phi;
    const float v = (hit_r - a.r_inner) / (a.r_outer - a.r_inner) * (float)sc.n_r;
    const int u0 = (int)floorf(u), v0 = (int)floorf(v);
    const float fu = u - (float)u0, fv = v - (float)v0;
    const int u0_w = pymod(u0, sc.n_phi), u1_w = pymod(u0 + 1, sc.n_phi);
    const int v0_h = min(max(v0, 0), sc.n_r - 1), v1_h = min(max(v0 + 1, 0), sc.n_r - 1);
    const float4 *t = sc.mips + sc.mip_off[0];
    const int stride = sc.mip_w[0];
    const float4 c00 = t[(size_t)v0_h * stride + u0_w], c10 = t[(size_t)v0_h * stride + u1_w];
    const float4 c01 = t[(size_t)v1_h * stride + u0_w], c11 = t[(size_t)v1_h * stride + u1_w];
    return make_float4(BHR_BILERP(c00.x, c10.x, c01.x, c11.x), BHR_BILERP(c00.y, c10.y, c01.y, c11.y),
                       BHR_BILERP(c00.z, c10.z, c01.z, c11.z), BHR_BILERP(c00.w, c10.w, c01.w, c11.w));
}
__device__ __forceinline__ float4 kerr_sample_disk(const BhrMarchArgs &a, float hit_x, float hit_y, float hit_r) {
    return kerr_sample_disk(a, a, hit_x, hit_y, hit_r);
}
// ... at mip level lod_i (Ray<true, RS>): kerr_sample_disk with sample_disk_level's level arithmetic -- u, v, the wrap and the
// clamp on the level's size.  At level 0 the same values as kerr_sample_disk (n / 2^0 = n).
__device__ __forceinline__ float4 kerr_sample_disk_level(const BhrMarchArgs &a, float hit_x, float hit_y, float hit_r, int lod_i) {
    const BhrScene &sc = a.sc;
    float phi = atan2f(hit_y, hit_x);
    const float r_safe = fmaxf(hit_r, 1e-3f);
    phi = phi + a.t_offset * kerr_omega(r_safe, kerr(a).kerr_a);
    while (phi < 0) phi += BHR_TWO_PI_F;
    while (phi >= BHR_TWO_PI_F) phi -= BHR_TWO_PI_F;
    const float scale = (float)(1 << lod_i);
    const float tex_w_lod = (float)sc.n_phi / scale, tex_h_lod = (float)sc.n_r / scale;
    const float u = phi / BHR_TWO_PI_F * tex_w_lod;
    const float v = (hit_r - a.r_inner) / (a.r_outer - a.r_inner) * tex_h_lod;
    const int u0 = (int)floorf(u), v0 = (int)floorf(v);
    const float fu = u - (float)u0, fv = v - (float)v0;
    const int wl = (int)tex_w_lod, vmax = (int)(tex_h_lod - 1.0f);
    const int u0_w = pymod(u0, wl), u1_w = pymod(u0 + 1, wl);
    const int v0_h = min(max(v0, 0), vmax), v1_h = min(max(v0 + 1, 0), vmax);
    const float4 *t = sc.mips + sc.mip_off[lod_i];
    const int stride = sc.mip_w[lod_i];
    const float4 c00 = t[(size_t)v0_h * stride + u0_w], c10 = t[(size_t)v0_h * stride + u1_w];
    const float4 c01 = t[(size_t)v1_h * stride + u0_w], c11 = t[(size_t)v1_h * stride + u1_w];
    return make_float4(BHR_BILERP(c00.x, c10.x, c01.x, c11.x), BHR_BILERP(c00.y, c10.y, c01.y, c11.y),
                       BHR_BILERP(c00.z, c10.z, c01.z, c11.z), BHR_BILERP(c00.w, c10.w, c01.w, c11.w));
}
// The mip level of a crossing from its hit differentials (hdx, hdy: the x and y components of d hit / d pixel along the two
// pixel axes): shade_hit's lines (render.py:2964-2988) in the Kerr texture coordinates phi = atan2(hy, hx) and the
// Boyer-Lindquist r = sqrt(hx^2 + hy^2 - a^2), so dr = (hx xi_x + hy xi_y) / r; the reference's 1e-6 guards; the roll's own
// derivative ignored, as the reference ignores it.  At a = 0 the reference's expressions.
__device__ __forceinline__ int kerr_lod(const BhrMarchArgs &a, float hit_x, float hit_y, float hdx_x, float hdx_y, float hdy_x, float hdy_y) {
    const float ka = kerr(a).kerr_a;
    const float rho2 = hit_x * hit_x + hit_y * hit_y;
    const float hit_r_g = sqrtf(rho2 - ka * ka + 1e-6f);
    const float hit_r_cyl = sqrtf(rho2 + 1e-6f);
    const float den = hit_r_cyl * hit_r_cyl + 1e-6f;
    const float w_f = (float)a.sc.n_phi, h_f = (float)a.sc.n_r, span = a.r_outer - a.r_inner;
    const float dr_dx = (hit_x * hdx_x + hit_y * hdx_y) / hit_r_g;
    const float dphi_dx = (-hit_y * hdx_x + hit_x * hdx_y) / den;
    const float dudx = dphi_dx * w_f / (2.0f * BHR_PI_F), dvdx = dr_dx * h_f / span;
    const float dr_dy = (hit_x * hdy_x + hit_y * hdy_y) / hit_r_g;
    const float dphi_dy = (-hit_y * hdy_x + hit_x * hdy_y) / den;
    const float dudy = dphi_dy * w_f / (2.0f * BHR_PI_F), dvdy = dr_dy * h_f / span;
    const float grad_sq = fmaxf(dudx * dudx + dvdx * dvdx, dudy * dudy + dvdy * dvdy);
    const float lod = logf(fmaxf(grad_sq, 1.0f)) / logf(2.0f) * a.aa_strength;
    return min((int)fminf(fmaxf(lod, 0.0f), 3.0f), a.sc.mip_last);
}

// The g-factor of the Kerr metric for a crossing at Boyer-Lindquist radius r of the plane, g = nu_obs / nu_em with both
// frequencies -p.u on the traced photon (p_t = -1), capped like the model's.  ph: the photon's momentum at the hit (hx, hy, 0)
// (Ray<false, KERR_EXACT>::step parks its x and y), of which three numbers enter: L_z = hx p_y - hy p_x, P = p.e_rho =
// (hx p_x + hy p_y) / rho and U = 1 + l.p = 1 + (r P - a L_z / rho) / rho, with rho^2 = hx^2 + hy^2 = r^2 + a^2.
//   observer  static at the camera: nu_obs = 1 / sqrt(1 - f), f = r / S there
//   emitter   r >= r_isco (of the disk's sense): the circular geodesic of Kerr's Omega,
//               nu_em = (1 - Omega L_z) / sqrt(1 - Omega^2 (r^2 + a^2) - (1 - a Omega)^2 / r)
//             the radicand clamped at 1e-6 like the reference's other guards (inside the photon orbit of the disk's sense there
//             is no circular orbit and the clamp would leave the gas dark; r_isco lies outside it at every spin)
//             r < r_isco: the gas keeps the ISCO orbit's E = -u_t and L = u_phi (from the host, binary64) and falls: its
//             covariant velocity is (-E, (L / rho) e_phi + w e_rho), rho^2 = r^2 + a^2, with w the inward root of
//             g^{mu nu} u_mu u_nu = -1,  qa w^2 + qb w + qc = 0:
//               c0 = E - a L / rho^2,  qa = 1 - r / rho^2,  qb = -2 c0 / rho,  qc = 1 - E^2 + L^2 / rho^2 - c0^2 / r
//               w = (-qb - sqrt(qb^2 - 4 qa qc)) / (2 qa),  S = l^mu u_mu = c0 + r w / rho
//               nu_em = E - L L_z / rho^2 - w P + U S / r
//             The discriminant is 4 (u^rho)^2 and, with the ISCO's E and L, the radial potential has its triple root at
//             r_isco: qb^2 - 4 qa qc = 4 (1 - E^2) (r_isco - r)^3 / (r rho^2), which is what is evaluated -- the literal
//             difference vanishes at r_isco and its square root there is the square root of the rounding (3e-4 in f32).
// tests/kerr_redshift_ref.py states the same in NumPy; tests/test_kerr_redshift_ref.py checks it against the 4 x 4 metric.
// obs_d: nu_moving / nu_static of the ray at a camera that moves (ray_kerr_observer.h), a factor of nu_obs; 1 at rest.
// f: the block the camera position is read from (kerr_sample_disk says what it is).
__device__ __forceinline__ float kerr_g_exact(const BhrMarchArgs &a, const BhrMarchArgs &f, float hx, float hy, float r, V3 ph, float obs_d = 1.0f) {
    const BhrKerrExactMarchArgs &k = kerr_exact(a);
    const float ka = k.kerr_a, a2 = ka * ka;
    V3 c = ld3(f.cp);
    asm volatile("" : "+v"(c.x));                // recomputed per hit, as the model's camera radius is
    const float cw = dot(c, c) - a2;
    const float cS = sqrtf(cw * cw + 4.0f * a2 * (c.z * c.z));
    const float nu_obs = 1.0f / sqrtf(1.0f - sqrtf(0.5f * (cw + cS)) / cS);
    const float rho2 = r * r + a2;
    const float irho = 1.0f / sqrtf(hx * hx + hy * hy);
    const float lz = hx * ph.y - hy * ph.x;
    const float P = (hx * ph.x + hy * ph.y) * irho;
    const float U = 1.0f + (r * P - ka * lz * irho) * irho;
    float nu_em;
    if (r >= k.isco_r) {
        const float om = kerr_omega(r, ka);
        const float q = 1.0f - ka * om;
        nu_em = (1.0f - om * lz) / sqrtf(fmaxf(1.0f - om * om * rho2 - q * q / r, 1e-6f));
    } else {
        const float E = k.isco_e, L = k.isco_l;
        const float rho = sqrtf(rho2);
        const float c0 = E - ka * L / rho2;
        const float qa = 1.0f - r / rho2;
        const float qb = -2.0f * c0 / rho;
        const float dr = fmaxf(k.isco_r - r, 0.0f);
        const float disc = 4.0f * ((1.0f - E) * (1.0f + E)) * (dr * dr * dr) / (r * rho2);
        const float w = (-qb - sqrtf(disc)) / (2.0f * qa);
        const float S = c0 + r * w / rho;
        nu_em = E - L * lz / rho2 - w * P + U * S / r;
    }
    return fminf(nu_obs * obs_d / fmaxf(nu_em, 1e-3f), BHR_G_FACTOR_CAP);
}
__device__ __forceinline__ float kerr_g_exact(const BhrMarchArgs &a, float hx, float hy, float r, V3 ph, float obs_d = 1.0f) {
    return kerr_g_exact(a, a, hx, hy, r, ph, obs_d);
}

// _apply_g_factor (render.py:2439-2516) for the untilted disk, unchanged but for the orbital frequency (Kerr's) and the
// emitter's radius, which is the Boyer-Lindquist hit radius the frequency is a function of.  The exact Kerr g-factor
// u^t (1 - Omega L_z) with frame dragging is kerr_g_exact above.  RS = KERR_EXACT: to_cam is the photon's momentum at the hit instead and
// g is kerr_g_exact's; everything downstream of g is the same code.
// f: the block the camera position is read from (kerr_sample_disk says what it is).
template <int RS>
__device__ __forceinline__ V3 kerr_g_factor(const BhrMarchArgs &a, const BhrMarchArgs &f, V3 base_color, float hit_x, float hit_y, float hit_r, V3 to_cam, float obs_d = 1.0f) {
    const float rs_f = BHR_RS;
    float g;
    if (RS == KERR_EXACT) {
        g = kerr_g_exact(a, f, hit_x, hit_y, hit_r, to_cam, obs_d);
    } else {
        V3 cam_pos = ld3(f.cp);
        asm volatile("" : "+v"(cam_pos.x));          // recomputed per hit, not kept across the march loop (march_device.h: apply_g_factor)
        const float r_obs = sqrtf(dot(cam_pos, cam_pos));
        const float r_em = hit_r;
        const float r_safe = fmaxf(r_em, rs_f + 1e-3f);
        const float omega = kerr_omega(r_safe, kerr(a).kerr_a);
        const float lorentz = sqrtf(fmaxf(1.0f - rs_f / r_safe, 1e-6f));
        const float beta = fminf(r_safe * omega / fmaxf(lorentz, 1e-6f), 0.99f);
        const float gamma = 1.0f / sqrtf(fmaxf(1.0f - beta * beta, 1e-6f));
        const float inv = 1.0f / sqrtf(hit_x * hit_x + hit_y * hit_y);
        const float rx = inv * hit_x, ry = inv * hit_y;
        float vx = ry, vy = -rx;                     // v_hat = r_hat x n, n = (0, 0, 1)
        const float v_norm = sqrtf(vx * vx + vy * vy);
        if (v_norm > 1e-6f) { vx = vx / v_norm; vy = vy / v_norm; } else { vx = 0.0f; vy = 1.0f; }
        const float ti = 1.0f / sqrtf(dot(to_cam, to_cam));
        const float cos_theta = vx * (ti * to_cam.x) + vy * (ti * to_cam.y);
        const float denom = fmaxf(1.0f - beta * cos_theta, 1e-3f);
        const float g_doppler = 1.0f / (gamma * denom);
        const float grav_num = sqrtf(fmaxf(1.0f - rs_f / fmaxf(r_obs, rs_f + 1e-3f), 1e-6f));
        const float grav_den = sqrtf(fmaxf(1.0f - rs_f / fmaxf(r_em, rs_f + 1e-3f), 1e-6f));
        g = fminf(g_doppler * (grav_num / grav_den) * obs_d, BHR_G_FACTOR_CAP);
    }
    const float intensity = fmaxf(powf(g, BHR_G_LUMINOSITY_POWER), 0.0f);
    float brightness = BHR_G_BRIGHTNESS_GAIN * intensity / (1.0f + intensity / BHR_G_FACTOR_CAP);
    const float radial_span = fmaxf(a.r_outer - a.r_inner, 1e-3f);
    const float radial_t = fminf(fmaxf((fmaxf(hit_r, a.r_inner) - a.r_inner) / radial_span, 0.0f), 1.0f);
    const float radial_profile = powf(1.0f - radial_t, BHR_DISK_RADIAL_BRIGHTNESS_POWER);
    brightness *= BHR_DISK_RADIAL_BRIGHTNESS_MIN + (BHR_DISK_RADIAL_BRIGHTNESS_MAX - BHR_DISK_RADIAL_BRIGHTNESS_MIN) * radial_profile;
    const float wien_arg = 1.0f - 1.0f / fmaxf(g, 0.1f);
    float r_scale = expf(2.21f * wien_arg);
    const float g_scale = expf(2.72f * wien_arg);
    float b_scale = expf(3.13f * wien_arg);
    r_scale = fminf(r_scale / g_scale, 3.0f);
    b_scale = fminf(b_scale / g_scale, 3.0f);
    const V3 tint = disk_tint();
    V3 out = mk(base_color.x * r_scale * tint.x * brightness, base_color.y * tint.y * brightness, base_color.z * b_scale * tint.z * brightness);
    out.x = fminf(fmaxf(out.x, 0.0f), 10.0f);
    out.y = fminf(fmaxf(out.y, 0.0f), 10.0f);
    out.z = fminf(fmaxf(out.z, 0.0f), 10.0f);
    return out;
}
template <int RS>
__device__ __forceinline__ V3 kerr_g_factor(const BhrMarchArgs &a, V3 base_color, float hit_x, float hit_y, float hit_r, V3 to_cam, float obs_d = 1.0f) {
    return kerr_g_factor<RS>(a, a, base_color, hit_x, hit_y, hit_r, to_cam, obs_d);
}
// The model's g alone, cap included: kerr_g_factor<0>'s own lines up to its g, for the Kerr line pass (march_kerr_line.hip), which
// bins g itself.  A function of its own beside it: kerr_g_factor stays the code it is in every object that inlines it.
__device__ __forceinline__ float kerr_g_model(const BhrMarchArgs &a, const BhrMarchArgs &f, float hit_x, float hit_y, float hit_r, V3 to_cam, float obs_d = 1.0f) {
    const float rs_f = BHR_RS;
    V3 cam_pos = ld3(f.cp);
    asm volatile("" : "+v"(cam_pos.x));          // recomputed per hit, as kerr_g_factor does
    const float r_obs = sqrtf(dot(cam_pos, cam_pos));
    const float r_em = hit_r;
    const float r_safe = fmaxf(r_em, rs_f + 1e-3f);
    const float omega = kerr_omega(r_safe, kerr(a).kerr_a);
    const float lorentz = sqrtf(fmaxf(1.0f - rs_f / r_safe, 1e-6f));
    const float beta = fminf(r_safe * omega / fmaxf(lorentz, 1e-6f), 0.99f);
    const float gamma = 1.0f / sqrtf(fmaxf(1.0f - beta * beta, 1e-6f));
    const float inv = 1.0f / sqrtf(hit_x * hit_x + hit_y * hit_y);
    const float rx = inv * hit_x, ry = inv * hit_y;
    float vx = ry, vy = -rx;                     // v_hat = r_hat x n, n = (0, 0, 1)
    const float v_norm = sqrtf(vx * vx + vy * vy);
    if (v_norm > 1e-6f) { vx = vx / v_norm; vy = vy / v_norm; } else { vx = 0.0f; vy = 1.0f; }
    const float ti = 1.0f / sqrtf(dot(to_cam, to_cam));
    const float cos_theta = vx * (ti * to_cam.x) + vy * (ti * to_cam.y);
    const float denom = fmaxf(1.0f - beta * cos_theta, 1e-3f);
    const float g_doppler = 1.0f / (gamma * denom);
    const float grav_num = sqrtf(fmaxf(1.0f - rs_f / fmaxf(r_obs, rs_f + 1e-3f), 1e-6f));
    const float grav_den = sqrtf(fmaxf(1.0f - rs_f / fmaxf(r_em, rs_f + 1e-3f), 1e-6f));
    return fminf(g_doppler * (grav_num / grav_den) * obs_d, BHR_G_FACTOR_CAP);
}

// one disk crossing, shaded and composited front to back (render.py:2951-3002 without the mip levels); obs_d: the moving
// camera's factor of g ahead of its cap in both redshift modes (1: the camera at rest); f: the block the frame's own fields
// (t_offset, cp) are read from (kerr_sample_disk says what it is)
template <int RS>
__device__ __forceinline__ void kerr_shade_hit(const BhrMarchArgs &a, const BhrMarchArgs &f, Shade &sh, float hit_x, float hit_y, V3 to_cam, float obs_d = 1.0f) {
    const float hit_r = sqrtf(hit_x * hit_x + hit_y * hit_y - kerr(a).kerr_a * kerr(a).kerr_a);
    if (!(a.r_outer >= hit_r && hit_r >= a.r_inner)) return;
    const float4 rgba = kerr_sample_disk(a, f, hit_x, hit_y, hit_r);
    const float base_alpha = fminf(rgba.w, 0.999f);
    const float disk_alpha = 1.0f - powf(1.0f - base_alpha, BHR_DISK_ALPHA_GAIN);
    const V3 col = kerr_g_factor<RS>(a, f, mk(rgba.x, rgba.y, rgba.z), hit_x, hit_y, hit_r, to_cam, obs_d);
    const float front = 1.0f - sh.alpha_total;
    const float wgt = disk_alpha * front;
    sh.accum = mk(sh.accum.x + col.x * wgt, sh.accum.y + col.y * wgt, sh.accum.z + col.z * wgt);
    sh.alpha_total = 1.0f - front * (1.0f - disk_alpha);
}
template <int RS>
__device__ __forceinline__ void kerr_shade_hit(const BhrMarchArgs &a, Shade &sh, float hit_x, float hit_y, V3 to_cam, float obs_d = 1.0f) {
    kerr_shade_hit<RS>(a, a, sh, hit_x, hit_y, to_cam, obs_d);
}
// ... of a ray with differentials: the texture at the crossing's mip level (kerr_lod); the g-factor and the compositing are
// kerr_shade_hit's.  A function of its own: the level-0 shade above stays the code it is in every object that inlines it.
template <int RS>
__device__ __forceinline__ void kerr_shade_hit_lod(const BhrMarchArgs &a, Shade &sh, float hit_x, float hit_y, V3 to_cam,
                                                   float hdx_x, float hdx_y, float hdy_x, float hdy_y) {
    const float hit_r = sqrtf(hit_x * hit_x + hit_y * hit_y - kerr(a).kerr_a * kerr(a).kerr_a);
    if (!(a.r_outer >= hit_r && hit_r >= a.r_inner)) return;
    const int lod_i = kerr_lod(a, hit_x, hit_y, hdx_x, hdx_y, hdy_x, hdy_y);
    const float4 rgba = kerr_sample_disk_level(a, hit_x, hit_y, hit_r, lod_i);
    const float base_alpha = fminf(rgba.w, 0.999f);
    const float disk_alpha = 1.0f - powf(1.0f - base_alpha, BHR_DISK_ALPHA_GAIN);
    const V3 col = kerr_g_factor<RS>(a, a, mk(rgba.x, rgba.y, rgba.z), hit_x, hit_y, hit_r, to_cam);
    const float front = 1.0f - sh.alpha_total;
    const float wgt = disk_alpha * front;
    sh.accum = mk(sh.accum.x + col.x * wgt, sh.accum.y + col.y * wgt, sh.accum.z + col.z * wgt);
    sh.alpha_total = 1.0f - front * (1.0f - disk_alpha);
}

// MOM (the Kerr ray map's build under a Kerr polarisation, march_kerr_raymap.hip): a crossing also parks the photon's whole
// momentum (p_x, p_y, p_z) at the hit, interpolated like the hit point, in words 5..7 of the lane's parking slot -- the words a
// ray with differentials would use, which the Kerr ray has none of -- and record_mom stores it beside the record.
template <bool DIFF, int SRC = 0, bool MOM = false>
struct KerrRay {
    static_assert(SRC == 0 || SRC == KERR_EXACT, "the Kerr Ray's second parameter is the redshift, model or exact");
    static_assert(!(DIFF && MOM), "the hit differentials and the parked momentum both use parking words 5..7");
    V3 x, p;
    V3 xi[2], pi[2];   // DIFF: the tangents d(x, p) / d(pixel) along the two pixel axes
    float r;       // Kerr-Schild radius of x
    float affine;
    Shade sh;
    int n_pend;    // parked disk crossings (0..2), in the lane's LDS slots, oldest first
    int step_count;
    int done;      // 0 running, 2 captured or escaped (escaped() tells), 3 ran out of iterations, 4 empty lane
    bool full;     // wave-uniform: some live lane has both its parking slots occupied

    // The camera: the momentum of the future-directed photon whose coordinate velocity is parallel to the pixel direction d,
    //   s = 1 / sqrt(1 - f (1 - (l.d)^2)),   Lam = (1 + s l.d) / (1 - f),   p = s d + f Lam l
    // (then 1 + l.p = Lam and dx/dl = s d; H = 0).  Outside the loop: IEEE operations.
    __device__ __forceinline__ void init(const BhrMarchArgs &a, int i, int j_local) {
        V3 ddx, ddy;
        const V3 d = pixel_ray<DIFF>(a, i, j_local, ddx, ddy);
        init_along(a, d);
        if (DIFF) {
            seed(a, d, ddx, 0);
            seed(a, d, ddy, 1);
        }
    }
    // DIFF: the tangent k of the camera's photon under d -> d + dd, with f and l constants of the camera:
    //   dc = l.dd,  ds = -s^3 f c dc,  dLam = (c ds + s dc) / (1 - f),  pi = ds d + s dd + f dLam l,  xi = 0
    __device__ __forceinline__ void seed(const BhrMarchArgs &a, const V3 d, const V3 dd, int k) {
        const float ka = kerr(a).kerr_a, a2 = ka * ka;
        const float w = dot(x, x) - a2;
        const float S = sqrtf(w * w + 4.0f * a2 * (x.z * x.z));
        const float r2 = 0.5f * (w + S), rc = sqrtf(r2);
        const float f = rc / S, Q = r2 + a2;
        const V3 l = mk((rc * x.x + ka * x.y) / Q, (rc * x.y - ka * x.x) / Q, x.z / rc);
        const float c = dot(l, d);
        const float s = 1.0f / sqrtf(1.0f - f * (1.0f - c * c));
        const float dc = dot(l, dd);
        const float ds = -(s * s * s) * f * c * dc;
        const float fdl = f * ((c * ds + s * dc) / (1.0f - f));
        xi[k] = mk(0, 0, 0);
        pi[k] = mk(ds * d.x + s * dd.x + fdl * l.x, ds * d.y + s * dd.y + fdl * l.y, ds * d.z + s * dd.z + fdl * l.z);
    }
    // the photon leaves the camera along d (ray_kerr_observer.h: a moving or panoramic camera's is not the pinhole pixel's own)
    __device__ __forceinline__ void init_along(const BhrMarchArgs &a, const V3 d) {
        x = ld3(a.cp);
        const float ka = kerr(a).kerr_a, a2 = ka * ka;
        const float w = dot(x, x) - a2;
        const float S = sqrtf(w * w + 4.0f * a2 * (x.z * x.z));
        const float r2 = 0.5f * (w + S);
        r = sqrtf(r2);
        const float f = r / S, Q = r2 + a2;
        const V3 l = mk((r * x.x + ka * x.y) / Q, (r * x.y - ka * x.x) / Q, x.z / r);
        const float c = dot(l, d);
        const float s = 1.0f / sqrtf(1.0f - f * (1.0f - c * c));
        const float fl = f * ((1.0f + s * c) / (1.0f - f));
        p = mk(s * d.x + fl * l.x, s * d.y + fl * l.y, s * d.z + fl * l.z);
        affine = 0.0f;
        sh.accum = mk(0, 0, 0);
        sh.alpha_total = 0.0f;
        sh.unsure = 0;
        n_pend = 0;
        full = false;
        step_count = 0;
        done = a.max_iter <= 0 ? 3 : 0;
    }

    // One RK4 step on (x, p).  The state is committed unconditionally, as in the strict Ray: a lane whose ray has ended
    // leaves the loop and reads only what settle() and values() need.
    __device__ __forceinline__ bool step(const BhrMarchArgs &a) {
        const float ka = kerr(a).kerr_a, a2 = ka * ka;
        // h = h_base dt_fac, the reference's step rule (render.py:2865-2868) on the Kerr-Schild radius; r_cap = r_s = 1
        float r_safe;
        asm("v_max_f32 %0, %1, %2" : "=v"(r_safe) : "v"(r), "v"(BHR_RS + 1e-3f));
        float y_s, y_q;
        rsq_rcp(r_safe, r_safe, y_s, y_q);
        const float far_scale = __builtin_fminf(sqrt_rn_s(r_safe, y_s), 10.0f);
        const float q = rcp_rn_s(r_safe, y_q);
        const float near_damp = rcp_rn(fmaf(2.0f, q * q * q, 1.0f));
        const float h = a.h_base * __builtin_amdgcn_fmed3f(far_scale * near_damp, 0.2f, 10.0f);
        const float hh = 0.5f * h;

        V3 v1, nx, np;
        V3 nxi[2], npi[2];
        if constexpr (!DIFF) {
            V3 d1, v, d, sv, sd;
            float rr;
            kerr_rhs(ka, a2, x, p, v1, d1, rr);
            kerr_rhs(ka, a2, fma3(hh, v1, x), fma3(hh, d1, p), v, d, rr);
            sv = fma3(2.0f, v, v1);
            sd = fma3(2.0f, d, d1);
            kerr_rhs(ka, a2, fma3(hh, v, x), fma3(hh, d, p), v, d, rr);
            sv = fma3(2.0f, v, sv);
            sd = fma3(2.0f, d, sd);
            kerr_rhs(ka, a2, fma3(h, v, x), fma3(h, d, p), v, d, rr);
            const float h6 = h * (1.0f / 6.0f);
            nx = fma3(h6, sv + v, x);
            np = fma3(h6, sd + d, p);
        } else {
            // the same primal lines, and the two tangents evaluated stage by stage next to them from the stage's own geometry
            // (tv, td: the tangent of the stage's (v, d); stv, std: their running RK4 sums)
            V3 d1, v, d, sv, sd;
            KerrStage st;
            V3 tv[2], td[2], stv[2], std[2];
            kerr_rhs_stage(ka, a2, x, p, v1, d1, st);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                kerr_rhs_tangent(ka, a2, x, p, st, xi[k], pi[k], tv[k], td[k]);
                stv[k] = tv[k];
                std[k] = td[k];
            }
            V3 xs = fma3(hh, v1, x), ps = fma3(hh, d1, p);
            kerr_rhs_stage(ka, a2, xs, ps, v, d, st);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                kerr_rhs_tangent(ka, a2, xs, ps, st, fma3(hh, tv[k], xi[k]), fma3(hh, td[k], pi[k]), tv[k], td[k]);
                stv[k] = fma3(2.0f, tv[k], stv[k]);
                std[k] = fma3(2.0f, td[k], std[k]);
            }
            sv = fma3(2.0f, v, v1);
            sd = fma3(2.0f, d, d1);
            xs = fma3(hh, v, x);
            ps = fma3(hh, d, p);
            kerr_rhs_stage(ka, a2, xs, ps, v, d, st);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                kerr_rhs_tangent(ka, a2, xs, ps, st, fma3(hh, tv[k], xi[k]), fma3(hh, td[k], pi[k]), tv[k], td[k]);
                stv[k] = fma3(2.0f, tv[k], stv[k]);
                std[k] = fma3(2.0f, td[k], std[k]);
            }
            sv = fma3(2.0f, v, sv);
            sd = fma3(2.0f, d, sd);
            xs = fma3(h, v, x);
            ps = fma3(h, d, p);
            kerr_rhs_stage(ka, a2, xs, ps, v, d, st);
            const float h6 = h * (1.0f / 6.0f);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                kerr_rhs_tangent(ka, a2, xs, ps, st, fma3(h, tv[k], xi[k]), fma3(h, td[k], pi[k]), tv[k], td[k]);
                nxi[k] = fma3(h6, stv[k] + tv[k], xi[k]);
                npi[k] = fma3(h6, std[k] + td[k], pi[k]);
            }
            nx = fma3(h6, sv + v, x);
            np = fma3(h6, sd + d, p);
        }
        const float rn = kerr_radius(a2, nx);

        const float aff = affine + h;
        // the ray goes on iff r_plus <= r <= r_escape and the affine parameter is within its limit
        const bool ended = __builtin_amdgcn_fmed3f(rn, kerr(a).kerr_rplus, a.r_esc) != rn || aff > a.max_affine;
        const bool crossing = x.z * nx.z < 0;              // the disk plane is z = 0 (no tilt with a spin)
        if (__builtin_amdgcn_ballot_w64(crossing) != 0ull) {
            if (!ended && crossing) {
                const float t_frac = x.z / (x.z - nx.z + 1e-8f);
                const float hx = x.x + t_frac * (nx.x - x.x);
                const float hy = x.y + t_frac * (nx.y - x.y);
                const float hit_r = sqrtf(hx * hx + hy * hy - a2);          // the Boyer-Lindquist radius in the plane
                if (a.r_outer >= hit_r && hit_r >= a.r_inner) {
                    Pending<DIFF> hit;
                    hit.hit_x = hx;
                    hit.hit_y = hy;
                    if (SRC == KERR_EXACT) {
                        // the photon at the hit: its momentum interpolated like the hit point (second order in the step), in
                        // the slot's floats of to_cam.  Its x and y are all the shade needs in the plane (kerr_g_exact makes
                        // L_z, P and U of them: no divide or square root here, inside the march loop)
                        hit.to_cam = mk(p.x + t_frac * (np.x - p.x), p.y + t_frac * (np.y - p.y), 0.0f);
                    } else {
                        hit.to_cam = mk(-v1.x, -v1.y, -v1.z);               // against dx/dl at the START of the step
                    }
                    // DIFF: the hit differentials are the x and y of the two tangents at the END of the step (the reference's
                    // convention, render.py:2928-2949: committed before the hit is interpolated), in words 5..8
                    if (DIFF) { hit.dxx = nxi[0].x; hit.dxy = nxi[0].y; hit.dyx = nxi[1].x; hit.dyy = nxi[1].y; }
                    park_store<DIFF>(n_pend, hit);                          // a free slot is guaranteed (march_tile_body flushes at 2)
                    if (MOM) {
                        g_park[n_pend][5][threadIdx.x] = p.x + t_frac * (np.x - p.x);
                        g_park[n_pend][6][threadIdx.x] = p.y + t_frac * (np.y - p.y);
                        g_park[n_pend][7][threadIdx.x] = p.z + t_frac * (np.z - p.z);
                    }
                    n_pend += 1;
                }
            }
            full = __builtin_amdgcn_ballot_w64(n_pend == 2) != 0ull;
        }
        affine = aff;
        if (DIFF) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                xi[k] = nxi[k];
                pi[k] = npi[k];
            }
        }
        x = nx;
        p = np;
        r = rn;
        step_count += 1;               // the lane's own count: max_iter ends the loop by it (march_tile_body keeps its twin for the totals)
        done = ended ? 2 : (step_count >= a.max_iter ? 3 : 0);
        return true;
    }

    __device__ __forceinline__ void settle(const BhrMarchArgs &a) {
        done = (__builtin_amdgcn_fmed3f(r, kerr(a).kerr_rplus, a.r_esc) != r || affine > a.max_affine) ? 2 : 3;
    }
    __device__ __forceinline__ bool escaped(const BhrMarchArgs &a) const { return done == 2 && !(r < kerr(a).kerr_rplus); }

    __device__ __forceinline__ void flush_one(const BhrMarchArgs &a) {
        if (n_pend > 0) {
            const Pending<DIFF> h = park_pop<DIFF>(n_pend);
            if (DIFF) kerr_shade_hit_lod<SRC>(a, sh, h.hit_x, h.hit_y, h.to_cam, h.dxx, h.dxy, h.dyx, h.dyy);
            else kerr_shade_hit<SRC>(a, sh, h.hit_x, h.hit_y, h.to_cam);
        }
    }
    // The Kerr ray map's build (march_kerr_raymap.hip): where flush_one shades the oldest parked crossing, this stores it as the
    // map's record n_rec of pixel `at`, front to back, and counts on past the slots.  For KERR_EXACT the three to_cam floats are
    // the photon's momentum (p_x, p_y, 0) the step parked.
    __device__ __forceinline__ void record_one(const BhrRayMapArgs &m, size_t at, int &n_rec) {
        if (n_pend > 0) {
            const Pending<false> h = park_pop<false>(n_pend);
            if (n_rec < m.slots) {
                const size_t p = (size_t)m.plane;
                float *q = m.hits + (size_t)n_rec * m.comps * p + at;
                q[0] = h.hit_x;
                q[p] = h.hit_y;
                q[2 * p] = h.to_cam.x;
                q[3 * p] = h.to_cam.y;
                q[4 * p] = h.to_cam.z;
            }
            n_rec += 1;
        }
    }
    // MOM: record_one with the parked momentum behind it -- into the map's momentum planes `mom`, [slot][component] like the
    // hits -- and the second slot's three words moved up with its record
    __device__ __forceinline__ void record_mom(const BhrRayMapArgs &m, float *mom, size_t at, int &n_rec) {
        static_assert(MOM, "record_mom: the momentum is parked by Ray<false, RS, true> alone");
        if (n_pend > 0) {
            const int t = threadIdx.x;
            const V3 ph = mk(g_park[0][5][t], g_park[0][6][t], g_park[0][7][t]);
            if (n_pend == 2) {
                g_park[0][5][t] = g_park[1][5][t];
                g_park[0][6][t] = g_park[1][6][t];
                g_park[0][7][t] = g_park[1][7][t];
            }
            if (n_rec < m.slots) {
                const size_t p = (size_t)m.plane;
                float *q = mom + (size_t)n_rec * 3 * p + at;
                q[0] = ph.x;
                q[p] = ph.y;
                q[2 * p] = ph.z;
            }
            record_one(m, at, n_rec);
        }
    }
    // the escape direction is the direction of dx/dl at the last state
    __device__ __forceinline__ V3 velocity(const BhrMarchArgs &a) const {
        V3 v, d;
        float rr;
        kerr_rhs(kerr(a).kerr_a, kerr(a).kerr_a * kerr(a).kerr_a, x, p, v, d, rr);
        return v;
    }
    __device__ __forceinline__ void finish_at(const BhrMarchArgs &a, int i, int j) { write_pixel(a, i, j, escaped(a), velocity(a), sh); }
    __device__ __forceinline__ void values(const BhrMarchArgs &a, float bk[3], float dk[3]) const { pixel_values(a, escaped(a), velocity(a), sh, bk, dk); }
};

// The Ray the schedules and the Kerr map's kernels march: the Kerr one itself, unless the Ray header that included this file
// derives its own from it (ray_kerr_observer.h, ray_kerr_dv2.h) -- the idiom of ray_strict.h.
#ifndef BHR_RAY_KERR_OBSERVER
#ifndef BHR_RAY_KERR_DV2
template <bool DIFF, int SRC = 0, bool MOM = false>
using Ray = KerrRay<DIFF, SRC, MOM>;
#endif
#endif

}  // namespace
