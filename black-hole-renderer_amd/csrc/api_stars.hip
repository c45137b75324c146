// api_stars.hip -- the point stars' entry points (include/bhr.h): bhr_set_stars, bhr_get_stars_info, bhr_stars_resources, and what
// the map's frames and bhr_raymap_read ask of the catalogue (the planes).  The gather kernel is stars.hip's, its launcher
// march_launch.hip's; the frames themselves are launched from render.hip.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "bhr_internal.h"

namespace {

const int32_t kMaxStars = 1 << 22;
const double kPi = 3.14159265358979323846;

void free_catalog(bhr_stars *st) {
    void *bufs[] = {st->d_rec, st->d_off, st->d_plane};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    memset(st, 0, sizeof(*st));
}

// every stream that may still read the catalogue or a plane
int32_t drain(bhr_ctx *ctx) {
    for (auto &f : ctx->slots) {
        if (f.stream) BHR_HIP(hipStreamSynchronize(f.stream));
        if (f.aux_stream) BHR_HIP(hipStreamSynchronize(f.aux_stream));
    }
    BHR_HIP(hipStreamSynchronize(ctx->scene_stream));
    return BHR_OK;
}

template <typename T>
int32_t cat_alloc(bhr_stars *st, T **p, size_t count) {
    *p = nullptr;
    const hipError_t e = hipMalloc((void **)p, count * sizeof(T));
    if (e != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();
        return bhr_fail(BHR_ERR_NOMEM, "bhr_set_stars: hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    }
    st->device_bytes += (int64_t)(count * sizeof(T));
    return BHR_OK;
}

// The grid: about 8 stars per bin, twice as many bins in longitude as in colatitude.
void grid_shape(int32_t n, int32_t *nt, int32_t *np) {
    int32_t t = (int32_t)lround(sqrt((double)n / 16.0));
    t = std::min(std::max(t, 4), 256);
    *nt = t;
    *np = 2 * t;
}

// The bin of a direction (already rounded to f32), in binary64: theta = acos(z), phi = atan2(y, x) in [0, 2 pi).
int32_t bin_of(const float d[3], int32_t nt, int32_t np) {
    const double z = std::min(std::max((double)d[2], -1.0), 1.0);
    const double theta = acos(z);
    double phi = atan2((double)d[1], (double)d[0]);
    if (phi < 0.0) phi += 2.0 * kPi;
    const int32_t t = std::min(std::max((int32_t)floor(theta / kPi * nt), 0), nt - 1);
    const int32_t p = std::min(std::max((int32_t)floor(phi / (2.0 * kPi) * np), 0), np - 1);
    return t * np + p;
}

}  // namespace

size_t bhr_star_plane_floats(const bhr_ctx *ctx) { return (size_t)ctx->rows * ctx->cfg.width * 3 + 4; }

void bhr_stars_release(bhr_ctx *ctx) {
    if (!ctx->stars) return;
    free_catalog(ctx->stars);
    delete ctx->stars;
    ctx->stars = nullptr;
}

void bhr_stars_invalidate(bhr_ctx *ctx) {
    if (ctx->stars) {
        ctx->stars->plane_valid = 0;
        ctx->stars->last_counts = nullptr;
    }
}

int32_t bhr_stars_ensure_plane(bhr_ctx *ctx) {
    bhr_stars *st = ctx->stars;
    if (!st || st->n <= 0) return bhr_fail(BHR_ERR_STATE, "star plane: no star catalogue (bhr_set_stars)");
    if (!ctx->raymap || !ctx->raymap->built) return bhr_fail(BHR_ERR_STATE, "star plane: no ray map has been built (bhr_raymap_build)");
    if (st->plane_valid) return BHR_OK;
    BHR_TRY(bhr_enter(ctx));           // the scene stream, behind the frames in flight (one of them may read the plane this rewrites)
    if (!st->d_plane) BHR_TRY(cat_alloc(st, &st->d_plane, bhr_star_plane_floats(ctx)));
    const bhr_raymap &rm = *ctx->raymap;
    BHR_TRY(bhr_launch_stars_gather(ctx, &rm.cam, rm.a, 1.0f, 0.0f, st->d_plane, ctx->stream));
    st->plane_valid = 1;
    st->last_counts = (const unsigned int *)(st->d_plane + (size_t)ctx->rows * ctx->cfg.width * 3);
    return BHR_OK;
}

int32_t bhr_stars_frame_plane(bhr_ctx *ctx, const bhr_camera *cam, float c, float s, const float **plane) {
    bhr_stars *st = ctx->stars;
    *plane = nullptr;
    if (c == 1.0f && s == 0.0f) {
        // cached, gathered on the scene stream before the frame took its slot (render.hip); the slot's stream waits for that stream
        if (!st->plane_valid) return bhr_fail(BHR_ERR_STATE, "star plane: the build view's plane was not prepared");
        *plane = st->d_plane;
        return BHR_OK;
    }
    bhr_frame_slot &f = bhr_slot(ctx);
    if (!f.d_star_plane) BHR_TRY(bhr_dev_alloc(&f.d_star_plane, bhr_star_plane_floats(ctx)));
    BHR_TRY(bhr_launch_stars_gather(ctx, cam, ctx->raymap->a, c, s, f.d_star_plane, ctx->stream));
    st->last_counts = (const unsigned int *)(f.d_star_plane + (size_t)ctx->rows * ctx->cfg.width * 3);
    *plane = f.d_star_plane;
    return BHR_OK;
}

extern "C" {

int32_t bhr_set_stars(bhr_ctx *ctx, const bhr_star *stars, int32_t n, const bhr_star_params *p) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_set_stars: null ctx");
    if (n < 0 || n > kMaxStars) return bhr_fail(BHR_ERR_INVALID, "bhr_set_stars: %d stars (0 .. %d)", n, kMaxStars);
    if (n > 0 && !stars) return bhr_fail(BHR_ERR_INVALID, "bhr_set_stars: null catalogue of %d stars", n);
    const bhr_star_params par = p ? *p : bhr_star_params{32.0f, 10.0f};
    if (!(par.max_magnification >= 1.0f && par.max_magnification <= 1e6f))
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_stars: max_magnification %g (1 .. 1e6)", (double)par.max_magnification);
    if (!(par.max_span_deg > 0.0f && par.max_span_deg <= 60.0f))
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_stars: max_span_deg %g (above 0, at most 60)", (double)par.max_span_deg);
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_stars: needs a whole-frame context (rows %d of %d)", ctx->rows, ctx->cfg.height);
    // the host's copy: directions normalized in binary64 and rounded once
    std::vector<bhr_star> cat((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
        const bhr_star &s = stars[k];
        const double x = s.dir[0], y = s.dir[1], z = s.dir[2];
        const double norm = sqrt(x * x + y * y + z * z);
        if (!(isfinite(x) && isfinite(y) && isfinite(z)) || !(fabs(norm - 1.0) <= 1e-3))
            return bhr_fail(BHR_ERR_INVALID, "bhr_set_stars: star %d: direction (%g, %g, %g) of norm %g is not a unit vector (within 1e-3)", k, x, y, z, norm);
        for (int c = 0; c < 3; ++c)
            if (!(isfinite(s.flux[c]) && s.flux[c] >= 0.0f))
                return bhr_fail(BHR_ERR_INVALID, "bhr_set_stars: star %d: flux[%d] = %g (finite and not negative)", k, c, (double)s.flux[c]);
        cat[(size_t)k] = s;
        cat[(size_t)k].dir[0] = (float)(x / norm);
        cat[(size_t)k].dir[1] = (float)(y / norm);
        cat[(size_t)k].dir[2] = (float)(z / norm);
    }
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(drain(ctx));               // the frames in flight read the catalogue and the planes
    if (n == 0) {
        bhr_stars_release(ctx);
        return BHR_OK;
    }
    if (!ctx->stars) {
        ctx->stars = new (std::nothrow) bhr_stars();
        if (!ctx->stars) return bhr_fail(BHR_ERR_NOMEM, "bhr_set_stars: out of host memory");
        memset(ctx->stars, 0, sizeof(bhr_stars));
    }
    bhr_stars *st = ctx->stars;
    free_catalog(st);
    // a counting sort into the bins; within a bin the stars keep the catalogue's order
    int32_t nt = 0, np = 0;
    grid_shape(n, &nt, &np);
    const size_t bins = (size_t)nt * np;
    std::vector<int32_t> off(bins + 1, 0), bin((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
        bin[(size_t)k] = bin_of(cat[(size_t)k].dir, nt, np);
        off[(size_t)bin[(size_t)k] + 1] += 1;
    }
    for (size_t b = 0; b < bins; ++b) off[b + 1] += off[b];
    std::vector<int32_t> at(off.begin(), off.end() - 1);
    std::vector<float> rec((size_t)n * 6);
    for (int32_t k = 0; k < n; ++k) {
        float *r = rec.data() + (size_t)(at[(size_t)bin[(size_t)k]]++) * 6;
        for (int c = 0; c < 3; ++c) {
            r[c] = cat[(size_t)k].dir[c];
            r[3 + c] = cat[(size_t)k].flux[c];
        }
    }
    int32_t rc = BHR_OK;
    if ((rc = cat_alloc(st, &st->d_rec, rec.size())) || (rc = cat_alloc(st, &st->d_off, off.size())) ||
        (rc = cat_alloc(st, &st->d_plane, bhr_star_plane_floats(ctx)))) {
        bhr_stars_release(ctx);        // everything freed: the context has no catalogue
        return rc;
    }
    BHR_HIP(hipMemcpyAsync(st->d_rec, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    BHR_HIP(hipMemcpyAsync(st->d_off, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    st->n = n;
    st->bins_theta = nt;
    st->bins_phi = np;
    st->params = par;
    st->cos_span = (float)cos((double)par.max_span_deg * kPi / 180.0);
    st->plane_valid = 0;
    st->last_counts = nullptr;
    return BHR_OK;
}

int32_t bhr_get_stars_info(bhr_ctx *ctx, bhr_stars_info *out) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_get_stars_info: bad argument");
    memset(out, 0, sizeof(*out));
    const bhr_stars *st = ctx->stars;
    if (!st || st->n <= 0) return BHR_OK;
    out->n = st->n;
    out->bins_theta = st->bins_theta;
    out->bins_phi = st->bins_phi;
    out->params = st->params;
    out->device_bytes = st->device_bytes;
    if (st->last_counts) {
        BHR_TRY(bhr_enter(ctx));       // behind the frame whose gather counted
        unsigned int c[4] = {0, 0, 0, 0};
        BHR_HIP(hipMemcpyAsync(c, st->last_counts, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
        BHR_HIP(hipStreamSynchronize(ctx->stream));
        out->images = c[0];
        out->capped = c[1];
        out->skipped_span = c[2];
    }
    return BHR_OK;
}

int32_t bhr_stars_resources(int32_t rot, int32_t out[3]) {
    if (!out) return bhr_fail(BHR_ERR_INVALID, "bhr_stars_resources: null argument");
    const void *f = bhr_stars_kernel(rot ? 1 : 0);
    if (!f) return bhr_fail(BHR_ERR_STATE, "bhr_stars_resources: no gather kernel in this library");
    hipFuncAttributes at;
    BHR_HIP(hipFuncGetAttributes(&at, f));
    out[0] = at.numRegs;
    out[1] = (int32_t)at.sharedSizeBytes;
    out[2] = (int32_t)at.localSizeBytes;
    return BHR_OK;
}

}  // extern "C"
