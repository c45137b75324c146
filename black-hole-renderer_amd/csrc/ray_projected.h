// ray_projected.h -- the projected Ray of the march (march_projected.o; see march_device.h): the observer Ray whose pixel directions
// are not a pinhole's but an equirectangular panorama's or an equidistant fisheye's (bhr_render_projected).
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
// operation is f32 rounded once, with no contraction (the strict objects' flags); sinf / cosf are the device library's accurate
// functions.  n' is unit to a few ulps and not renormalised.  From n' on the ray is the observer's: aberration, init_along, the
// strict march, D in the disk's g and on the sky (ray_observer.h).
//
// A fisheye pixel outside the image circle has no ray: its lane is initialised like any other and then marked as run out before
// the first step (done = 3).  The tile body never enters the loop with it, counts no step, and stores it through its normal
// exit: escaped() is false and nothing was shaded, so BG and DISK are exactly 0 -- under supersampling the zeros enter the box
// filter, which anti-aliases the rim.
#pragma once
#define BHR_RAY_PROJECTED 1   // ray_observer.h: the schedules' Ray is the one below, derived from the observer's
#include "ray_observer.h"

namespace {

// The kernels of this object take the observer's block with the projection behind it (bhr_internal.h: BhrProjectedMarchArgs).
__device__ __forceinline__ const BhrProjectedMarchArgs &projected(const BhrMarchArgs &a) { return static_cast<const BhrProjectedMarchArgs &>(a); }

template <bool DIFF, int SRC = 0>
struct Ray : ObserverRay<DIFF, SRC> {
    typedef ObserverRay<DIFF, SRC> Base;

    __device__ __forceinline__ void init(const BhrMarchArgs &a, int i, int j_local) {
        const BhrProjectedMarchArgs &q = projected(a);
        const V3 cr = ld3(a.cr), cu = ld3(a.cu), cf = ld3(a.cf);
        const float px = (float)i + 0.5f, py = (float)(j_local + a.row0) + 0.5f;
        float ca, cb, cc;
        bool inside = true;
        if (q.proj_kind == BHR_PROJ_EQUIRECT) {            // wave-uniform: a kernel argument
            const float lon = (px / (float)a.width - 0.5f) * q.span_h;
            const float lat = (0.5f - py / (float)a.height) * q.span_v;
            const float cl = cosf(lat);
            ca = cl * cosf(lon);
            cb = cl * sinf(lon);
            cc = sinf(lat);
        } else {
            const float s = 2.0f / (float)min(a.width, a.height);
            const float x = (px - (float)a.width / 2) * s, y = ((float)a.height / 2 - py) * s;
            const float rho = sqrtf(x * x + y * y);
            inside = rho <= 1.0f;
            const float theta = rho * q.span_h;
            const float inv = rho > 0 ? 1.0f / rho : 0.0f;
            const float st = sinf(theta);
            ca = cosf(theta);
            cb = st * (x * inv);
            cc = st * (y * inv);
        }
        Base::init_aberrated(a, mk((ca * cf.x + cb * cr.x) + cc * cu.x, (ca * cf.y + cb * cr.y) + cc * cu.y,
                                   (ca * cf.z + cb * cr.z) + cc * cu.z), i, j_local);
        if (!inside) this->done = 3;                       // outside the image circle: no step, zeros through the normal store
    }
};

}  // namespace
