// ray_kerr_observer.h -- the Kerr camera's Ray (march_kerr_observer.o; see march_device.h): the Kerr Ray seen by a camera that
// may move and may be panoramic (bhr_render_kerr_view).
//
// The Kerr camera identifies the static observer's local frame at the camera with the Kerr-Schild coordinate axes: the pixel
// direction is the photon's coordinate direction, and KerrRay::init_along makes the momentum from it (ray_kerr.h).  That
// convention stays.  Ahead of it sits the camera model of the Schwarzschild observer and projected marches:
//   n'    the pixel's direction in the camera's own frame: pixel_ray (proj_kind 0, the pinhole) or camera_device.h's
//         equirectangular / fisheye direction (proj_kind BHR_PROJ_*: wave-uniform, a kernel argument)
//   D   = 1 / (gamma (1 - beta.n'))                                        nu_moving / nu_static of that ray
//   n   = (n' + (gamma^2 / (gamma + 1)) (beta.n') beta - gamma beta) D     unit in exact arithmetic, not renormalised
// with beta the velocity the static observer at the camera measures; gamma and gamma^2 / (gamma + 1) come from the host,
// binary64 rounded once.  n takes the place of the pixel direction in init_along, and everything from there to the last step is
// the Kerr Ray's: RK4 loop, step rule, capture at r_plus, escape, crossings, parking slots.  D then enters twice: as a factor of
// the disk's g ahead of its cap in both redshift modes (ray_kerr.h: obs_d -- the static observer's nu_obs turned into the moving
// one's), and on the sky sample when the call asks for it (camera_device.h: observer_sky).  beta = 0 under the pinhole gives
// n = n' and D = 1 in f32, exactly, and the frame of the Kerr march bit for bit: this object has the Kerr object's flags.
//
// A fisheye pixel outside the image circle has no ray: its lane is initialised like any other and then marked as run out before
// the first step (done = 3).  The tile body never enters the loop with it, counts no step, and stores it through its normal
// exit: escaped() is false and nothing was shaded, so BG and DISK are exactly 0 -- under supersampling the zeros enter the box
// filter.
//
// D is one more value alive across the march loop, the lane's own.
#pragma once
#define BHR_RAY_KERR_OBSERVER 1   // ray_kerr.h: the schedules' Ray is the one below, derived from the Kerr one
#include "ray_kerr.h"
#include "camera_device.h"

namespace {

// The kernels of this object take the exact-redshift Kerr block with the camera behind it (bhr_internal.h: BhrKerrViewMarchArgs).
__device__ __forceinline__ const BhrKerrViewMarchArgs &kerr_view(const BhrMarchArgs &a) { return static_cast<const BhrKerrViewMarchArgs &>(a); }

template <bool DIFF, int SRC = 0>
struct Ray : KerrRay<DIFF, SRC> {
    typedef KerrRay<DIFF, SRC> Base;
    float dopp;    // D of the lane's ray

    __device__ __forceinline__ void init(const BhrMarchArgs &a, int i, int j_local) {
        const BhrKerrViewMarchArgs &o = kerr_view(a);
        V3 np;
        bool inside = true;
        if (o.proj_kind == 0) {
            V3 unused_x, unused_y;
            np = pixel_ray<false>(a, i, j_local, unused_x, unused_y);
        } else {
            np = projected_direction(a, o.proj_kind, o.span_h, o.span_v, i, j_local, inside);
        }
        const V3 b = ld3(o.obs_beta);
        const float bn = dot(b, np);
        dopp = 1.0f / (o.obs_gamma * (1.0f - bn));
        const float c = o.obs_g2 * bn;
        Base::init_along(a, mk(((np.x + c * b.x) - o.obs_gamma * b.x) * dopp, ((np.y + c * b.y) - o.obs_gamma * b.y) * dopp,
                               ((np.z + c * b.z) - o.obs_gamma * b.z) * dopp));
        if (!inside) this->done = 3;                       // outside the image circle: no step, zeros through the normal store
    }

    // shade the oldest parked crossing (the Kerr Ray's flush_one with the ray's D in g)
    __device__ __forceinline__ void flush_one(const BhrMarchArgs &a) {
        if (this->n_pend > 0) {
            const Pending<false> h = park_pop<false>(this->n_pend);
            kerr_shade_hit<SRC>(a, this->sh, h.hit_x, h.hit_y, h.to_cam, dopp);
        }
    }
    // pixel_values (march_device.h) with the sky sample scaled ahead of the product with 1 - alpha
    __device__ __forceinline__ void values(const BhrMarchArgs &a, float bk[3], float dk[3]) const {
        V3 bg = mk(0, 0, 0);
        if (this->escaped(a)) {
            bg = sample_skybox(a.sc, normalized(this->velocity(a)));
            if (kerr_view(a).obs_sky_shift) bg = observer_sky(bg, dopp);
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

}  // namespace
