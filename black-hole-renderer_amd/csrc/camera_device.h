// camera_device.h -- what the moving and panoramic cameras share whatever Ray they launch (ray_observer.h and ray_projected.h
// over the strict Ray, ray_kerr_observer.h over the Kerr one; included behind march_device.h): the pixel directions of the
// panoramic cameras and the sky sample's Doppler scaling.
//
// F, R, U are the camera's forward, right and up; Wf x Hf is the grid the march walks (a.width x a.height: k W x k H under
// supersampling), (i, j) its pixel.  The direction n' of a pixel in the camera's own frame is
//   equirectangular   lon = (((float)i + 0.5f) / (float)Wf - 0.5f) * span_h
//                     lat = (0.5f - ((float)j + 0.5f) / (float)Hf) * span_v
//                     a = cosf(lat) cosf(lon), b = cosf(lat) sinf(lon), c = sinf(lat)
//   fisheye           s = 2.0f / (float)min(Wf, Hf)
//                     x = (((float)i + 0.5f) - (float)Wf / 2) s, y = ((float)Hf / 2 - ((float)j + 0.5f)) s
//                     rho = sqrtf(x x + y y), theta = rho span_h, inv = rho > 0 ? 1.0f / rho : 0.0f
//                     a = cosf(theta), b = sinf(theta) (x inv), c = sinf(theta) (y inv); inside = rho <= 1.0f
//   n'_k = (a F_k + b R_k) + c U_k
// span_h, span_v: the spans in radians (the fisheye's span_h is HALF its full angle), binary64 on the host rounded once.  Every
// operation is f32; sinf / cosf are the device library's accurate functions; how the products and sums are rounded is the
// including object's choice of contraction.  n' is unit to a few ulps and not renormalised.
#pragma once

namespace {

// The sky through the moving camera: the sample scaled by the disk's brightness power of D and its Wien ratios, without the
// brightness law's soft knee.  D is clamped to [0.1, BHR_G_FACTOR_CAP] like g; the result may exceed 1.
__device__ __forceinline__ V3 observer_sky(V3 c, float D) {
    const float Ds = fminf(fmaxf(D, 0.1f), BHR_G_FACTOR_CAP);
    const float I = powf(Ds, BHR_G_LUMINOSITY_POWER);
    const float w = 1.0f - 1.0f / Ds;
    const float g_scale = expf(2.72f * w);
    const float r_s = fminf(expf(2.21f * w) / g_scale, 3.0f);
    const float b_s = fminf(expf(3.13f * w) / g_scale, 3.0f);
    return mk(c.x * (r_s * I), c.y * I, c.z * (b_s * I));
}

// kind: BHR_PROJ_EQUIRECT, else the fisheye (wave-uniform: a kernel argument).  inside: false for a fisheye pixel outside the
// image circle, which has no ray.
__device__ __forceinline__ V3 projected_direction(const BhrMarchArgs &a, int32_t kind, float span_h, float span_v, int i, int j_local, bool &inside) {
    const V3 cr = ld3(a.cr), cu = ld3(a.cu), cf = ld3(a.cf);
    const float px = (float)i + 0.5f, py = (float)(j_local + a.row0) + 0.5f;
    float ca, cb, cc;
    inside = true;
    if (kind == BHR_PROJ_EQUIRECT) {
        const float lon = (px / (float)a.width - 0.5f) * span_h;
        const float lat = (0.5f - py / (float)a.height) * span_v;
        const float cl = cosf(lat);
        ca = cl * cosf(lon);
        cb = cl * sinf(lon);
        cc = sinf(lat);
    } else {
        const float s = 2.0f / (float)min(a.width, a.height);
        const float x = (px - (float)a.width / 2) * s, y = ((float)a.height / 2 - py) * s;
        const float rho = sqrtf(x * x + y * y);
        inside = rho <= 1.0f;
        const float theta = rho * span_h;
        const float inv = rho > 0 ? 1.0f / rho : 0.0f;
        const float st = sinf(theta);
        ca = cosf(theta);
        cb = st * (x * inv);
        cc = st * (y * inv);
    }
    return mk((ca * cf.x + cb * cr.x) + cc * cu.x, (ca * cf.y + cb * cr.y) + cc * cu.y, (ca * cf.z + cb * cr.z) + cc * cu.z);
}

}  // namespace
