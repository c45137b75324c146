// ray_observer.h -- the observer Ray of the march (march_observer.o, and under ray_projected.h march_projected.o; see
// march_device.h): the strict Ray seen by a camera that moves.
//
// The camera moves with velocity beta (units of c) as the static observer at its position measures it; that observer's local
// frame is identified with the coordinate axes, as pixel_ray does for the camera that stands still (DESIGN.md "Observer").  A
// pixel whose direction in the moving camera's own frame is n' -- what pixel_ray returns: the basis is the moving camera's -- is
// traced along the static-frame direction
//   D = 1 / (gamma (1 - beta.n'))                                        nu_observed / nu_static of that ray
//   n = (n' + (gamma^2 / (gamma + 1)) (beta.n') beta - gamma beta) D     unit in exact arithmetic, not renormalised
// and everything from there to the last step is the strict Ray's: RK4 loop, step rule, capture, escape, crossings, parking slots.
// D then enters twice: the disk's g-factor is g_doppler g_grav D ahead of its cap (march_device.h: apply_g_factor), and the
// sky sample is scaled like the disk's emission (observer_sky) when the call asks for it.  beta = 0 gives n = n' and D = 1 in
// f32, exactly, and the frame of the strict march bit for bit.  gamma and gamma^2 / (gamma + 1) come from the host, binary64
// rounded once; beta.n', D and n are f32 here, with no contraction (the strict objects' flags).
//
// No ray differentials (their seeds would need the aberration's Jacobian) and the texture source only.  D is one more value
// alive across the march loop, the lane's own.
#pragma once
#define BHR_RAY_OBSERVER 1   // ray_strict.h: the schedules' Ray is the one below, derived from the strict one
#include "ray_strict.h"
#include "camera_device.h"

namespace {

// The kernels of this object take the march's block with the observer behind it (bhr_internal.h: BhrObserverMarchArgs) and hand
// it to the shared schedule as the BhrMarchArgs it is; the observer code reads the tail through this.
__device__ __forceinline__ const BhrObserverMarchArgs &observer(const BhrMarchArgs &a) { return static_cast<const BhrObserverMarchArgs &>(a); }

// (observer_sky, the sky sample through the moving camera, is camera_device.h's: the Kerr camera scales its sky alike)

template <bool DIFF, int SRC = 0>
struct ObserverRay : StrictRay<DIFF, SRC> {
    static_assert(!DIFF && SRC == 0, "the observer march has no ray differentials and the texture source only");
    typedef StrictRay<DIFF, SRC> Base;
    float dopp;    // D of the lane's ray

    __device__ __forceinline__ void init(const BhrMarchArgs &a, int i, int j_local) {
        V3 unused_x, unused_y;
        init_aberrated(a, pixel_ray<false>(a, i, j_local, unused_x, unused_y), i, j_local);
    }
    // the ray of pixel (i, j_local), whose direction in the moving camera's frame is np (ray_projected.h: a projection's is not
    // pixel_ray's)
    __device__ __forceinline__ void init_aberrated(const BhrMarchArgs &a, const V3 np, int i, int j_local) {
        const BhrObserverMarchArgs &o = observer(a);
        const V3 b = ld3(o.obs_beta);
        const float bn = dot(b, np);
        dopp = 1.0f / (o.obs_gamma * (1.0f - bn));
        const float c = o.obs_g2 * bn;
        Base::init_along(a, mk(((np.x + c * b.x) - o.obs_gamma * b.x) * dopp, ((np.y + c * b.y) - o.obs_gamma * b.y) * dopp,
                               ((np.z + c * b.z) - o.obs_gamma * b.z) * dopp), i, j_local);
    }

    // shade the oldest parked crossing (the strict Ray's flush_one with the ray's D in g)
    __device__ __forceinline__ void flush_one(const BhrMarchArgs &a) {
        if (this->n_pend > 0) {
            const Pending<false> h = park_pop<false>(this->n_pend);
            shade_hit<false, 0>(a, a, this->sh, h.hit_x, h.hit_y, h.to_cam, h.dxx, h.dxy, h.dyx, h.dyy, dopp);
        }
    }
    // pixel_values (march_device.h) with the sky sample scaled ahead of the product with 1 - alpha
    __device__ __forceinline__ void values(const BhrMarchArgs &a, float bk[3], float dk[3]) const {
        V3 bg = mk(0, 0, 0);
        if (this->escaped()) {
            bg = sample_skybox(a.sc, normalized(this->d));
            if (observer(a).obs_sky_shift) bg = observer_sky(bg, dopp);
        }
        const float k = 1.0f - this->sh.alpha_total;
        bk[0] = __fmul_rn(bg.x, k);
        bk[1] = __fmul_rn(bg.y, k);
        bk[2] = __fmul_rn(bg.z, k);
        dk[0] = fminf(fmaxf(this->sh.accum.x, 0.0f), 1.0f);
        dk[1] = fminf(fmaxf(this->sh.accum.y, 0.0f), 1.0f);
        dk[2] = fminf(fmaxf(this->sh.accum.z, 0.0f), 1.0f);
    }
    __device__ __forceinline__ void finish_at(const BhrMarchArgs &a, int i, int j) {
        float bk[3], dk[3];
        values(a, bk, dk);
        store_pixel(a, i, j, a.width, bk, dk);
    }
};

// The Ray the schedules march: the observer's itself, unless the Ray header that included this file derives its own from it
// (ray_projected.h).
#ifndef BHR_RAY_PROJECTED
template <bool DIFF, int SRC = 0>
using Ray = ObserverRay<DIFF, SRC>;
#endif

}  // namespace
