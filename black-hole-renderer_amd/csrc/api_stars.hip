// api_stars.hip -- the point stars' entry points (include/bhr.h): bhr_set_stars, bhr_get_stars_info, bhr_stars_resources, their
// Kerr twins bhr_set_kerr_stars, bhr_get_kerr_stars_info, bhr_kerr_stars_resources, and what a map's frames and its plane reader
// ask of its catalogue (the planes).  A context has a catalogue per kind of map (bhr_internal.h: bhr_stars); everything here is
// written once and takes the kind.  The gather kernel is stars.hip's, its launcher march_launch.hip's; the frames themselves are
// launched from render.hip.
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

// what the refusals call the two catalogues' setters and their maps' builds
const char *setter_name(int32_t kind) { return kind == BHR_RAYMAP_KERR ? "bhr_set_kerr_stars" : "bhr_set_stars"; }
const char *build_name(int32_t kind) { return kind == BHR_RAYMAP_KERR ? "bhr_kerr_raymap_build" : "bhr_raymap_build"; }
const char *kind_word(int32_t kind) { return kind == BHR_RAYMAP_KERR ? "Kerr " : ""; }

template <typename T>
int32_t cat_alloc(bhr_stars *st, const char *who, T **p, size_t count) {
    *p = nullptr;
    const hipError_t e = hipMalloc((void **)p, count * sizeof(T));
    if (e != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();
        return bhr_fail(BHR_ERR_NOMEM, "%s: hipMalloc(%zu bytes) failed: %s", who, count * sizeof(T), hipGetErrorString(e));
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

void bhr_stars_release(bhr_ctx *ctx, int32_t kind) {
    bhr_stars *&st = bhr_stars_of(ctx, kind);
    if (!st) return;
    free_catalog(st);
    delete st;
    st = nullptr;
}

void bhr_stars_invalidate(bhr_ctx *ctx, int32_t kind) {
    if (bhr_stars *st = bhr_stars_of(ctx, kind)) {
        st->plane_valid = 0;
        st->last_counts = nullptr;
    }
}

int32_t bhr_stars_ensure_plane(bhr_ctx *ctx, int32_t kind) {
    bhr_stars *st = bhr_stars_of(ctx, kind);
    const bhr_raymap *rm = bhr_stars_map(ctx, kind);
    if (!st || st->n <= 0) return bhr_fail(BHR_ERR_STATE, "star plane: no star catalogue (%s)", setter_name(kind));
    if (!rm || !rm->built) return bhr_fail(BHR_ERR_STATE, "star plane: no ray map has been built (%s)", build_name(kind));
    if (st->plane_valid) return BHR_OK;
    BHR_TRY(bhr_enter(ctx));           // the scene stream, behind the frames in flight (one of them may read the plane this rewrites)
    if (!st->d_plane) BHR_TRY(cat_alloc(st, setter_name(kind), &st->d_plane, bhr_star_plane_floats(ctx)));
    BHR_TRY(bhr_launch_stars_gather(ctx, st, &rm->cam, rm->a, 1.0f, 0.0f, st->d_plane, ctx->stream));
    st->plane_valid = 1;
    st->last_counts = (const unsigned int *)(st->d_plane + (size_t)ctx->rows * ctx->cfg.width * 3);
    return BHR_OK;
}

int32_t bhr_stars_frame_plane(bhr_ctx *ctx, int32_t kind, const bhr_camera *cam, float c, float s, const float **plane) {
    bhr_stars *st = bhr_stars_of(ctx, kind);
    *plane = nullptr;
    if (c == 1.0f && s == 0.0f) {
        // cached, gathered on the scene stream before the frame took its slot (render.hip); the slot's stream waits for that stream
        if (!st->plane_valid) return bhr_fail(BHR_ERR_STATE, "star plane: the build view's plane was not prepared");
        *plane = st->d_plane;
        return BHR_OK;
    }
    // the slot's plane is the frame's own, whichever kind of map the slot's last frame came from: its gather runs on the slot's
    // stream ahead of the shade launch that reads it
    bhr_frame_slot &f = bhr_slot(ctx);
    if (!f.d_star_plane) BHR_TRY(bhr_dev_alloc(&f.d_star_plane, bhr_star_plane_floats(ctx)));
    BHR_TRY(bhr_launch_stars_gather(ctx, st, cam, bhr_stars_map(ctx, kind)->a, c, s, f.d_star_plane, ctx->stream));
    st->last_counts = (const unsigned int *)(f.d_star_plane + (size_t)ctx->rows * ctx->cfg.width * 3);
    *plane = f.d_star_plane;
    return BHR_OK;
}

// ---- what a map's entry points refuse of its catalogue, and its plane reader (api_raymap.hip, api_kerr_raymap.hip) --------------------

int32_t bhr_stars_check_map(const bhr_ctx *ctx, int32_t kind, const char *who) {
    if (bhr_have_stars(ctx, kind) && bhr_stars_map(ctx, kind)->ss > 1)
        return bhr_fail(BHR_ERR_STATE, "%s: a %sstar catalogue is set (%s, %d stars) and the map is supersampled (factor %d); point stars need a map with one ray per pixel",
                        who, kind_word(kind), setter_name(kind), bhr_stars_of(ctx, kind)->n, bhr_stars_map(ctx, kind)->ss);
    return BHR_OK;
}

int32_t bhr_stars_check_shutter(const bhr_ctx *ctx, int32_t kind, const char *who) {
    if (bhr_have_stars(ctx, kind))
        return bhr_fail(BHR_ERR_STATE, "%s: a %sstar catalogue is set (%s, %d stars); shutter frames from the map have no point stars -- remove it (n = 0) first", who,
                        kind_word(kind), setter_name(kind), bhr_stars_of(ctx, kind)->n);
    return BHR_OK;
}

int32_t bhr_stars_read_plane(bhr_ctx *ctx, int32_t kind, const char *who, void *out, int64_t bytes) {
    if (!bhr_have_stars(ctx, kind)) return bhr_fail(BHR_ERR_STATE, "%s: no %sstar catalogue has been set (%s)", who, kind_word(kind), setter_name(kind));
    BHR_TRY(bhr_stars_check_map(ctx, kind, who));
    const size_t want = (size_t)bhr_stars_map(ctx, kind)->a.plane * 12;
    if (bytes != (int64_t)want) return bhr_fail(BHR_ERR_INVALID, "%s: plane %d has %zu bytes, caller gave %lld", who, BHR_RAYMAP_STARS, want, (long long)bytes);
    BHR_TRY(bhr_stars_ensure_plane(ctx, kind));
    BHR_TRY(bhr_enter(ctx));
    BHR_HIP(hipMemcpyAsync(out, bhr_stars_of(ctx, kind)->d_plane, want, hipMemcpyDeviceToHost, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    return BHR_OK;
}

namespace {

// bhr_set_stars / bhr_set_kerr_stars: the kind's catalogue replaced (n = 0: removed)
int32_t set_catalog(bhr_ctx *ctx, int32_t kind, const bhr_star *stars, int32_t n, const bhr_star_params *p) {
    const char *who = setter_name(kind);
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "%s: null ctx", who);
    if (n < 0 || n > kMaxStars) return bhr_fail(BHR_ERR_INVALID, "%s: %d stars (0 .. %d)", who, n, kMaxStars);
    if (n > 0 && !stars) return bhr_fail(BHR_ERR_INVALID, "%s: null catalogue of %d stars", who, n);
    const bhr_star_params par = p ? *p : bhr_star_params{32.0f, 10.0f};
    if (!(par.max_magnification >= 1.0f && par.max_magnification <= 1e6f))
        return bhr_fail(BHR_ERR_INVALID, "%s: max_magnification %g (1 .. 1e6)", who, (double)par.max_magnification);
    if (!(par.max_span_deg > 0.0f && par.max_span_deg <= 60.0f))
        return bhr_fail(BHR_ERR_INVALID, "%s: max_span_deg %g (above 0, at most 60)", who, (double)par.max_span_deg);
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "%s: needs a whole-frame context (rows %d of %d)", who, ctx->rows, ctx->cfg.height);
    // the host's copy: directions normalized in binary64 and rounded once
    std::vector<bhr_star> cat((size_t)n);
    for (int32_t k = 0; k < n; ++k) {
        const bhr_star &s = stars[k];
        const double x = s.dir[0], y = s.dir[1], z = s.dir[2];
        const double norm = sqrt(x * x + y * y + z * z);
        if (!(isfinite(x) && isfinite(y) && isfinite(z)) || !(fabs(norm - 1.0) <= 1e-3))
            return bhr_fail(BHR_ERR_INVALID, "%s: star %d: direction (%g, %g, %g) of norm %g is not a unit vector (within 1e-3)", who, k, x, y, z, norm);
        for (int c = 0; c < 3; ++c)
            if (!(isfinite(s.flux[c]) && s.flux[c] >= 0.0f))
                return bhr_fail(BHR_ERR_INVALID, "%s: star %d: flux[%d] = %g (finite and not negative)", who, k, c, (double)s.flux[c]);
        cat[(size_t)k] = s;
        cat[(size_t)k].dir[0] = (float)(x / norm);
        cat[(size_t)k].dir[1] = (float)(y / norm);
        cat[(size_t)k].dir[2] = (float)(z / norm);
    }
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(drain(ctx));               // the frames in flight read the catalogue and the planes
    if (n == 0) {
        bhr_stars_release(ctx, kind);
        return BHR_OK;
    }
    bhr_stars *&slot = bhr_stars_of(ctx, kind);
    if (!slot) {
        slot = new (std::nothrow) bhr_stars();
        if (!slot) return bhr_fail(BHR_ERR_NOMEM, "%s: out of host memory", who);
        memset(slot, 0, sizeof(bhr_stars));
    }
    bhr_stars *st = slot;
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
    if ((rc = cat_alloc(st, who, &st->d_rec, rec.size())) || (rc = cat_alloc(st, who, &st->d_off, off.size())) ||
        (rc = cat_alloc(st, who, &st->d_plane, bhr_star_plane_floats(ctx)))) {
        bhr_stars_release(ctx, kind);  // everything freed: the context has no catalogue of this kind
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

int32_t catalog_info(bhr_ctx *ctx, int32_t kind, bhr_stars_info *out) {
    memset(out, 0, sizeof(*out));
    const bhr_stars *st = bhr_stars_of(ctx, kind);
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

}  // namespace

extern "C" {

int32_t bhr_set_stars(bhr_ctx *ctx, const bhr_star *stars, int32_t n, const bhr_star_params *p) { return set_catalog(ctx, BHR_RAYMAP_SCHWARZSCHILD, stars, n, p); }
int32_t bhr_set_kerr_stars(bhr_ctx *ctx, const bhr_star *stars, int32_t n, const bhr_star_params *p) { return set_catalog(ctx, BHR_RAYMAP_KERR, stars, n, p); }

int32_t bhr_get_stars_info(bhr_ctx *ctx, bhr_stars_info *out) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_get_stars_info: bad argument");
    return catalog_info(ctx, BHR_RAYMAP_SCHWARZSCHILD, out);
}

int32_t bhr_get_kerr_stars_info(bhr_ctx *ctx, bhr_stars_info *out) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_get_kerr_stars_info: bad argument");
    return catalog_info(ctx, BHR_RAYMAP_KERR, out);
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

// the Kerr map's STARS shade kernels (march_kerr_raymap.hip): exact: the exact redshift's; rot: the turned one
int32_t bhr_kerr_stars_resources(int32_t exact, int32_t rot, int32_t out[3]) {
    if (!out) return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_stars_resources: null argument");
    const void *f = bhr_march_kernel_kerr_raymap(rot ? BHR_MK_KERR_RAYMAP_SHADE_STARS_ROT : BHR_MK_KERR_RAYMAP_SHADE_STARS, exact ? 1 : 0, 0);
    if (!f) return bhr_fail(BHR_ERR_STATE, "bhr_kerr_stars_resources: no STARS shade kernel in this library");
    hipFuncAttributes at;
    BHR_HIP(hipFuncGetAttributes(&at, f));
    out[0] = at.numRegs;
    out[1] = (int32_t)at.sharedSizeBytes;
    out[2] = (int32_t)at.localSizeBytes;
    return BHR_OK;
}

}  // extern "C"
