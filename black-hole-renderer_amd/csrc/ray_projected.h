// ray_projected.h -- the projected Ray of the march (march_projected.o; see march_device.h): the observer Ray whose pixel directions
// are not a pinhole's but an equirectangular panorama's or an equidistant fisheye's (bhr_render_projected).
//
// The direction n' of a pixel in the camera's own frame is camera_device.h's (which states the formulas; the Kerr camera
// shares them): every operation f32 rounded once, with no contraction (the strict objects' flags).  From n' on the ray is the
// observer's: aberration, init_along, the strict march, D in the disk's g and on the sky (ray_observer.h).
//
// A fisheye pixel outside the image circle has no ray: its lane is initialised like any other and then marked as run out before
// the first step (done = 3).  The tile body never enters the loop with it, counts no step, and stores it through its normal
// exit: escaped() is false and nothing was shaded, so BG and DISK are exactly 0 -- under supersampling the zeros enter the box
// filter, which anti-aliases the rim.
#pragma once
#define BHR_RAY_PROJECTED 1   // ray_observer.h: the schedules' Ray is the one below, derived from the observer's
#include "ray_observer.h"   // (camera_device.h with it)

namespace {

// The kernels of this object take the observer's block with the projection behind it (bhr_internal.h: BhrProjectedMarchArgs).
__device__ __forceinline__ const BhrProjectedMarchArgs &projected(const BhrMarchArgs &a) { return static_cast<const BhrProjectedMarchArgs &>(a); }

template <bool DIFF, int SRC = 0>
struct Ray : ObserverRay<DIFF, SRC> {
    typedef ObserverRay<DIFF, SRC> Base;

    __device__ __forceinline__ void init(const BhrMarchArgs &a, int i, int j_local) {
        const BhrProjectedMarchArgs &q = projected(a);
        bool inside;
        const V3 np = projected_direction(a, q.proj_kind, q.span_h, q.span_v, i, j_local, inside);
        Base::init_aberrated(a, np, i, j_local);
        if (!inside) this->done = 3;                       // outside the image circle: no step, zeros through the normal store
    }
};

}  // namespace
