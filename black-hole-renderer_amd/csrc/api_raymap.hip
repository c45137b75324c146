// api_raymap.hip -- the owner of a context's ray maps, and the Schwarzschild map's entry points (include/bhr.h).
// The owner: what a map of either kind (bhr_raymap, bhr_internal.h) needs done the same way -- its planes, the tail of a build,
// the plane reader, free -- once, taking the map; api_kerr_raymap.hip keeps the Kerr map's refusals and entry points over it.
// The entry points: build, read, info, free, and the refusals of bhr_raymap_render, bhr_raymap_render_view and
// bhr_raymap_render_shutter (the frames themselves are launched from render.hip, next to bhr_render: they take a frame slot
// like any other).  The kernels are march_raymap.hip's and march_kerr_raymap.hip's, their launchers march_launch.hip's.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bhr_internal.h"

namespace {

// one plane of a map object
template <typename T>
int32_t plane_alloc(bhr_raymap *rm, const char *who, T **p, size_t count) {
    *p = nullptr;
    const hipError_t e = hipMalloc((void **)p, count * sizeof(T));
    if (e != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();
        return bhr_fail(BHR_ERR_NOMEM, "%s: hipMalloc(%zu bytes) failed: %s", who, count * sizeof(T), hipGetErrorString(e));
    }
    rm->device_bytes += (int64_t)(count * sizeof(T));
    return BHR_OK;
}

// every stream that may still read the map
int32_t drain(bhr_ctx *ctx) {
    for (auto &f : ctx->slots) {
        if (f.stream) BHR_HIP(hipStreamSynchronize(f.stream));
        if (f.aux_stream) BHR_HIP(hipStreamSynchronize(f.aux_stream));
    }
    BHR_HIP(hipStreamSynchronize(ctx->scene_stream));
    return BHR_OK;
}

int32_t fetch(bhr_ctx *ctx, void *dst, const void *d_src, size_t bytes) {
    BHR_HIP(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    return BHR_OK;
}

// what a context has to be for a map: whole frame, one ray per pixel, the texture source (a supersampled map has a factor of
// its own, option "raymap_supersample"; the context's stays off)
int32_t check_context(const bhr_ctx *ctx, const char *who, int32_t code) {
    if (ctx->ss > 1 || ctx->ada_k > 1)
        return bhr_fail(code, "%s: supersampling is on (factor %d); a ray map holds one ray per pixel", who, ctx->ss > 1 ? ctx->ss : ctx->ada_k);
    if (ctx->disk_source != BHR_DISK_TEXTURE)
        return bhr_fail(code, "%s: the disk source is Disk V2 (%d); a ray map shades the disk texture", who, ctx->disk_source);
    return BHR_OK;
}

}  // namespace

// Shared by bhr_raymap_render_view, bhr_raymap_render_shutter and the Kerr ray map's view frames (api_kerr_raymap.hip), in
// binary64: is `cam` the build camera `b` turned rigidly
// about z -- same height, pitch and escape radius, same distance from the axis, and right / up / forward the build's turned by
// the angle between the two positions in the xy plane?  On the axis build_camera takes a fallback basis that does not turn with
// the position: refused.  Gives the turn's cosine and sine, rounded once.
int32_t bhr_raymap_turn_of_build(const bhr_camera &b, const bhr_camera *cam, const char *who, float *rot_c, float *rot_s) {
    if (!(cam->pos[2] == b.pos[2] && cam->pixel_width == b.pixel_width && cam->pixel_height == b.pixel_height && cam->r_escape == b.r_escape))
        return bhr_fail(BHR_ERR_INVALID, "%s: the camera's height, pixel pitch or escape radius (%g, %g x %g, %g) is not the build's (%g, %g x %g, %g)", who,
                        (double)cam->pos[2], (double)cam->pixel_width, (double)cam->pixel_height, (double)cam->r_escape, (double)b.pos[2],
                        (double)b.pixel_width, (double)b.pixel_height, (double)b.r_escape);
    const double bx = b.pos[0], by = b.pos[1], cx = cam->pos[0], cy = cam->pos[1];
    const double rb = sqrt(bx * bx + by * by), rc = sqrt(cx * cx + cy * cy);
    if (!(rb >= 1e-6 && rc >= 1e-6))
        return bhr_fail(BHR_ERR_INVALID, "%s: a camera on the z axis (distance %g, the build's %g) has no turn about it", who, rc, rb);
    if (!(fabs(rc - rb) <= 1e-5 * rb))
        return bhr_fail(BHR_ERR_INVALID, "%s: the camera is %.9g from the z axis, the build's %.9g: not a turn of it", who, rc, rb);
    const double angle = atan2(bx * cy - by * cx, bx * cx + by * cy);
    const double c = cos(angle), s = sin(angle);
    const float *have[3] = {cam->right, cam->up, cam->forward};
    const float *from[3] = {b.right, b.up, b.forward};
    const char *names[3] = {"right", "up", "forward"};
    for (int v = 0; v < 3; ++v) {
        const double want[3] = {c * from[v][0] - s * from[v][1], s * from[v][0] + c * from[v][1], (double)from[v][2]};
        for (int k = 0; k < 3; ++k)
            if (!(fabs((double)have[v][k] - want[k]) <= 1e-5))
                return bhr_fail(BHR_ERR_INVALID, "%s: the camera's %s[%d] is %.9g, the build's turned by %.9g rad has %.9g: not a turn of it", who, names[v],
                                k, (double)have[v][k], angle, want[k]);
    }
    *rot_c = (float)c;
    *rot_s = (float)s;
    return BHR_OK;
}

namespace {

// point stars (bhr_set_stars): a supersampled map's shade kernels have no STARS variant
int32_t check_stars(const bhr_ctx *ctx, const char *who) { return bhr_stars_check_map(ctx, BHR_RAYMAP_SCHWARZSCHILD, who); }

// polarisation (bhr_set_polarization): the Stokes kernel walks the build view's records of a map with one ray per pixel
int32_t check_polar(const bhr_ctx *ctx, const char *who, const char *what) {
    if (bhr_have_polar(ctx)) return bhr_fail(BHR_ERR_STATE, "%s: a polarisation is set (bhr_set_polarization) and %s -- switch it off (NULL) first", who, what);
    return BHR_OK;
}

void free_planes(bhr_raymap *rm) {
    BhrRayMapArgs &a = rm->a;
    void *bufs[] = {a.steps, a.status, a.dir, a.crossings, a.hits, a.over_count, a.over_list, a.stats, rm->mom};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    memset(&a, 0, sizeof(a));
    rm->mom = nullptr;
    rm->has_mom = 0;
    rm->built = 0;
    rm->alloc_slots = rm->alloc_comps = rm->alloc_ss = 0;
    rm->over_cap = 0;
    rm->device_bytes = 0;
}

// K slots of `comps` floats over `plane` pixels with an overflow list for factor ss; a failed allocation leaves the object empty
int32_t alloc_planes(bhr_raymap *rm, const char *who, int32_t K, int32_t comps, size_t plane, int32_t ss) {
    BhrRayMapArgs &a = rm->a;
    // the fix kernel's grid is sized in blocks of 256 entries of the list's capacity; a supersampled map lists whole k x k
    // groups, k^2-aligned (k^2 divides 256)
    const size_t over_cap = (plane + 255) / 256 * 256;
    if (over_cap % 256 != 0 || over_cap % (size_t)(ss * ss) != 0 || over_cap > (size_t)INT32_MAX)
        return bhr_fail(BHR_ERR_STATE, "%s: an overflow list of %zu entries for factor %d", who, over_cap, ss);
    int32_t rc = BHR_OK;
    if ((rc = plane_alloc(rm, who, &a.steps, plane)) || (rc = plane_alloc(rm, who, &a.status, plane)) || (rc = plane_alloc(rm, who, &a.dir, 3 * plane)) ||
        (rc = plane_alloc(rm, who, &a.crossings, plane)) || (rc = plane_alloc(rm, who, &a.hits, (size_t)K * comps * plane)) ||
        (rc = plane_alloc(rm, who, &a.over_count, 16)) || (rc = plane_alloc(rm, who, &a.over_list, over_cap)) ||
        (rc = plane_alloc(rm, who, &a.stats, 8 + BHR_STEP_CELL))) {
        free_planes(rm);               // a later build starts clean; the context is as it was
        return rc;
    }
    a.slots = K;
    a.comps = comps;
    a.plane = (int64_t)plane;
    rm->alloc_slots = K;
    rm->alloc_comps = comps;
    rm->alloc_ss = ss;
    rm->over_cap = (int32_t)over_cap;
    return BHR_OK;
}

// the star plane of the build view under the map's own kind of catalogue is stale when the map changes; so are the Stokes planes
// of the last frame: the Schwarzschild map's, or under a Kerr polarisation a Kerr map frame's
void invalidate_consumers(bhr_ctx *ctx, const bhr_raymap *rm) {
    bhr_stars_invalidate(ctx, rm->kind);
    if (rm->kind == BHR_RAYMAP_KERR && bhr_have_kerr_polar(ctx)) bhr_polar_invalidate(ctx);
    if (rm->kind != BHR_RAYMAP_SCHWARZSCHILD) return;
    bhr_polar_invalidate(ctx);
}

}  // namespace

// ---- what the two maps of a context share (bhr_internal.h) ----------------------------------------------------------------------------

void bhr_raymap_release(bhr_ctx *ctx, bhr_raymap **map) {
    bhr_raymap *rm = *map;
    if (!rm) return;
    free_planes(rm);
    *map = nullptr;
    invalidate_consumers(ctx, rm);
    delete rm;
}

int32_t bhr_raymap_free_map(bhr_ctx *ctx, bhr_raymap **map) {
    if (!*map) return BHR_OK;
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(drain(ctx));               // the frames in flight read the map
    bhr_raymap_release(ctx, map);
    return BHR_OK;
}

int32_t bhr_raymap_build_into(bhr_ctx *ctx, bhr_raymap **map, const char *who, const bhr_camera *cam, uint32_t flags, bhr_march_variant v, int32_t K, int32_t ss) {
    const bool diff = bhr_want_diff(ctx, flags);
    const int32_t comps = diff ? 9 : 5;
    const size_t plane = (size_t)ctx->rows * ctx->cfg.width * (size_t)(ss * ss);

    BHR_TRY(bhr_enter(ctx));           // behind the frames in flight: they may be reading the map this build rewrites
    if (!*map) {
        *map = new bhr_raymap();
        memset(*map, 0, sizeof(bhr_raymap));
        (*map)->kind = v == BHR_MV_NONE ? BHR_RAYMAP_SCHWARZSCHILD : BHR_RAYMAP_KERR;
    }
    bhr_raymap *rm = *map;
    rm->built = 0;
    invalidate_consumers(ctx, rm);
    if (rm->a.hits && (rm->alloc_slots != K || rm->alloc_comps != comps || rm->alloc_ss != ss)) {
        BHR_TRY(drain(ctx));
        free_planes(rm);
    }
    if (!rm->a.hits) BHR_TRY(alloc_planes(rm, who, K, comps, plane, ss));
    // a Kerr map built under a Kerr polarisation (bhr_set_kerr_polarization) keeps the photon's momentum per stored crossing in
    // planes of its own; a build without one gives them back
    const bool want_mom = rm->kind == BHR_RAYMAP_KERR && bhr_have_kerr_polar(ctx);
    rm->has_mom = 0;
    if (want_mom && !rm->mom) BHR_TRY(plane_alloc(rm, who, &rm->mom, (size_t)K * 3 * plane));
    if (!want_mom && rm->mom) {
        BHR_TRY(drain(ctx));
        (void)hipFree(rm->mom);
        rm->mom = nullptr;
        rm->device_bytes -= (int64_t)((size_t)K * 3 * plane * sizeof(float));
    }
    const BhrRayMapArgs &a = rm->a;
    // records beyond a pixel's crossings stay zero
    BHR_HIP(hipMemsetAsync(a.hits, 0, (size_t)K * comps * plane * sizeof(float), ctx->stream));
    BHR_HIP(hipMemsetAsync(a.over_count, 0, 16 * sizeof(unsigned int), ctx->stream));
    BHR_HIP(hipMemsetAsync(a.stats, 0, (8 + BHR_STEP_CELL) * sizeof(unsigned long long), ctx->stream));
    if (rm->mom) BHR_HIP(hipMemsetAsync(rm->mom, 0, (size_t)K * 3 * plane * sizeof(float), ctx->stream));
    BHR_TRY(bhr_launch_raymap_build(ctx, cam, flags, a, ss, v, rm->mom));
    std::vector<unsigned long long> stats(8 + BHR_STEP_CELL);
    unsigned int over = 0;
    BHR_TRY(fetch(ctx, stats.data(), a.stats, stats.size() * sizeof(unsigned long long)));
    BHR_TRY(fetch(ctx, &over, a.over_count, sizeof(over)));
    unsigned long long steps = 0;
    for (int k = 0; k < BHR_STEP_LANES; ++k) steps += stats[8 + (size_t)k * BHR_STEP_STRIDE];
    rm->ray_steps = steps;
    rm->crossings_stored = stats[0];
    rm->overflow_pixels = over;
    rm->diff = diff ? 1 : 0;
    rm->slots = K;
    rm->ss = ss;
    rm->cam = *cam;
    if (rm->kind == BHR_RAYMAP_KERR) {
        rm->kerr_spin = ctx->kerr_spin;
        rm->kerr_redshift = ctx->kerr_redshift;
    }
    rm->has_mom = rm->mom ? 1 : 0;
    rm->built = 1;
    return BHR_OK;
}

int32_t bhr_raymap_read_plane(bhr_ctx *ctx, const bhr_raymap *rm, const char *who, int32_t which, void *out, int64_t bytes) {
    const BhrRayMapArgs &a = rm->a;
    const size_t plane = (size_t)a.plane;
    size_t want = 0;
    switch (which) {
    case BHR_RAYMAP_STEPS: case BHR_RAYMAP_STATUS: case BHR_RAYMAP_CROSSINGS: want = plane * 4; break;
    case BHR_RAYMAP_ESCAPE_DIR: want = plane * 12; break;
    case BHR_RAYMAP_HITS: want = (size_t)a.slots * a.comps * plane * 4; break;
    default: return bhr_fail(BHR_ERR_INVALID, "%s: unknown plane %d", who, which);
    }
    if (bytes != (int64_t)want) return bhr_fail(BHR_ERR_INVALID, "%s: plane %d has %zu bytes, caller gave %lld", who, which, want, (long long)bytes);
    BHR_TRY(bhr_enter(ctx));
    if (which == BHR_RAYMAP_STEPS) return fetch(ctx, out, a.steps, want);
    if (which == BHR_RAYMAP_STATUS) return fetch(ctx, out, a.status, want);
    if (which == BHR_RAYMAP_CROSSINGS) return fetch(ctx, out, a.crossings, want);
    // the device planes are [component][pixel]; the caller gets [pixel][component]
    const int nc = which == BHR_RAYMAP_ESCAPE_DIR ? 3 : a.comps, ns = which == BHR_RAYMAP_ESCAPE_DIR ? 1 : a.slots;
    std::vector<float> tmp((size_t)nc * plane);
    float *o = (float *)out;
    for (int s = 0; s < ns; ++s) {
        const float *src = which == BHR_RAYMAP_ESCAPE_DIR ? a.dir : a.hits + (size_t)s * nc * plane;
        BHR_TRY(fetch(ctx, tmp.data(), src, tmp.size() * sizeof(float)));
        float *os = o + (size_t)s * plane * nc;
        for (int c = 0; c < nc; ++c)
            for (size_t p = 0; p < plane; ++p) os[p * nc + c] = tmp[(size_t)c * plane + p];
    }
    return BHR_OK;
}

// ---- the Schwarzschild map's own -------------------------------------------------------------------------------------------------------

int32_t bhr_raymap_check_render(bhr_ctx *ctx, float t_offset, uint32_t flags) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_render: null ctx");
    BHR_TRY(bhr_kerr_refuse(ctx, "bhr_raymap_render", "a ray map holds Schwarzschild rays"));
    if (flags & ~(uint32_t)(BHR_SKIP_BLOOM | BHR_LENS_FLARE))
        return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_render: flags %u (BHR_SKIP_BLOOM and BHR_LENS_FLARE only)", flags);
    if (!isfinite(t_offset)) return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_render: t_offset is not finite");
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_render: needs a whole-frame context (rows %d of %d)", ctx->rows, ctx->cfg.height);
    if (!ctx->raymap || !ctx->raymap->built) return bhr_fail(BHR_ERR_STATE, "bhr_raymap_render: no ray map has been built (bhr_raymap_build)");
    BHR_TRY(check_context(ctx, "bhr_raymap_render", BHR_ERR_STATE));
    BHR_TRY(check_stars(ctx, "bhr_raymap_render"));
    if (ctx->raymap->ss > 1) BHR_TRY(check_polar(ctx, "bhr_raymap_render", "the map is supersampled; the Stokes planes need a map with one ray per pixel"));
    return BHR_OK;
}

// bhr_raymap_render_view's refusals, before anything is launched: the disk is not tilted, and `cam` is the build camera turned
// rigidly about z (bhr_raymap_turn_of_build).
int32_t bhr_raymap_check_render_view(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags, float *rot_c, float *rot_s) {
    const char *who = "bhr_raymap_render_view";
    if (!ctx || !cam) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    BHR_TRY(bhr_kerr_refuse(ctx, who, "a ray map holds Schwarzschild rays"));
    if (flags & ~(uint32_t)(BHR_SKIP_BLOOM | BHR_LENS_FLARE))
        return bhr_fail(BHR_ERR_INVALID, "%s: flags %u (BHR_SKIP_BLOOM and BHR_LENS_FLARE only)", who, flags);
    if (!isfinite(cam->t_offset)) return bhr_fail(BHR_ERR_INVALID, "%s: t_offset is not finite", who);
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "%s: needs a whole-frame context (rows %d of %d)", who, ctx->rows, ctx->cfg.height);
    if (ctx->cfg.disk_tilt_deg != 0.0f)
        return bhr_fail(BHR_ERR_INVALID, "%s: the disk is tilted by %g degrees; a turn about z is a symmetry of an untilted disk only", who,
                        (double)ctx->cfg.disk_tilt_deg);
    if (!ctx->raymap || !ctx->raymap->built) return bhr_fail(BHR_ERR_STATE, "%s: no ray map has been built (bhr_raymap_build)", who);
    BHR_TRY(check_context(ctx, who, BHR_ERR_STATE));
    BHR_TRY(bhr_raymap_turn_of_build(ctx->raymap->cam, cam, who, rot_c, rot_s));
    BHR_TRY(check_stars(ctx, who));
    return check_polar(ctx, who, "the Stokes planes are the build view's; turned views have none");
}

// bhr_raymap_render_shutter's refusals (include/bhr.h), before anything is launched.  A sample with the build camera's pose,
// field for field, is the still camera -- on any disk, turn (1, 0); any other has to pass bhr_raymap_render_view's checks.
int32_t bhr_raymap_check_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags, BhrShutterArgs *smp, bool *turned) {
    const char *who = "bhr_raymap_render_shutter";
    if (!ctx || !cams) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    BHR_TRY(bhr_kerr_refuse(ctx, who, "a ray map holds Schwarzschild rays"));
    if (n < 1 || n > BHR_SHUTTER_MAX_SAMPLES) return bhr_fail(BHR_ERR_INVALID, "%s: %d samples (1 .. %d)", who, n, BHR_SHUTTER_MAX_SAMPLES);
    if (flags & ~(uint32_t)(BHR_SKIP_BLOOM | BHR_LENS_FLARE))
        return bhr_fail(BHR_ERR_INVALID, "%s: flags %u (BHR_SKIP_BLOOM and BHR_LENS_FLARE only)", who, flags);
    for (int j = 0; j < n; ++j)
        if (!isfinite(cams[j].t_offset)) return bhr_fail(BHR_ERR_INVALID, "%s: sample %d: t_offset is not finite", who, j);
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "%s: needs a whole-frame context (rows %d of %d)", who, ctx->rows, ctx->cfg.height);
    if (!ctx->raymap || !ctx->raymap->built) return bhr_fail(BHR_ERR_STATE, "%s: no ray map has been built (bhr_raymap_build)", who);
    BHR_TRY(check_context(ctx, who, BHR_ERR_STATE));
    const bhr_camera &b = ctx->raymap->cam;
    memset(smp, 0, sizeof(*smp));
    *turned = false;
    for (int j = 0; j < n; ++j) {
        const bhr_camera &c = cams[j];
        BhrShutterSample &o = smp->smp[j];
        o.t = c.t_offset;
        o.c = 1.0f;
        o.s = 0.0f;
        for (int k = 0; k < 3; ++k) o.cp[k] = c.pos[k];
        bool still = c.pixel_width == b.pixel_width && c.pixel_height == b.pixel_height && c.r_escape == b.r_escape;
        for (int k = 0; k < 3; ++k)
            still = still && c.pos[k] == b.pos[k] && c.right[k] == b.right[k] && c.up[k] == b.up[k] && c.forward[k] == b.forward[k];
        if (still) continue;
        char sample[64];
        snprintf(sample, sizeof(sample), "%s: sample %d", who, j);
        if (ctx->cfg.disk_tilt_deg != 0.0f)
            return bhr_fail(BHR_ERR_INVALID, "%s: the disk is tilted by %g degrees and the camera is not the build's; a turn about z is a symmetry of an untilted disk only",
                            sample, (double)ctx->cfg.disk_tilt_deg);
        BHR_TRY(bhr_raymap_turn_of_build(b, &c, sample, &o.c, &o.s));
        *turned = *turned || !(o.c == 1.0f && o.s == 0.0f);
    }
    smp->n = n;
    smp->inv = 1.0f / (float)n;
    // point stars: the fused and the supersampled shade kernels have no STARS variant
    BHR_TRY(bhr_stars_check_shutter(ctx, BHR_RAYMAP_SCHWARZSCHILD, who));
    return check_polar(ctx, who, "shutter frames from the map have no Stokes planes");
}

extern "C" {

int32_t bhr_raymap_build(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags) {
    if (!ctx || !cam) return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_build: null argument");
    BHR_TRY(bhr_kerr_refuse(ctx, "bhr_raymap_build", "a ray map holds Schwarzschild rays"));
    if (flags & ~(uint32_t)BHR_SKIP_DIFFERENTIALS) return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_build: flags %u (BHR_SKIP_DIFFERENTIALS only)", flags);
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_build: needs a whole-frame context (rows %d of %d)", ctx->rows, ctx->cfg.height);
    BHR_TRY(check_context(ctx, "bhr_raymap_build", BHR_ERR_INVALID));
    const int32_t K = ctx->opt.raymap_slots;
    if (K < 1 || K > 8) return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_build: raymap_slots %d (1 .. 8)", K);
    // the map's own factor: the map of the fine frame, k rows x k W (the context's own supersampling stays off, check_context)
    const int32_t ss = ctx->opt.raymap_ss;
    if (ss != 1 && ss != 2 && ss != 4 && ss != 8) return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_build: raymap_supersample %d (1, 2, 4 or 8)", ss);
    if ((int64_t)ss * ss * ctx->cfg.width * ctx->cfg.height >= ((int64_t)1 << 31))
        return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_build: %d x %d rays of a %dx%d frame exceed 2^31", ss, ss, ctx->cfg.width, ctx->cfg.height);
    return bhr_raymap_build_into(ctx, &ctx->raymap, "bhr_raymap_build", cam, flags, BHR_MV_NONE, K, ss);
}

int32_t bhr_raymap_read(bhr_ctx *ctx, int32_t which, void *out, int64_t bytes) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_read: bad argument");
    if (!ctx->raymap || !ctx->raymap->built) return bhr_fail(BHR_ERR_STATE, "bhr_raymap_read: no ray map has been built (bhr_raymap_build)");
    // the build view's star plane (include/bhr.h "point stars"), gathered now if the map or the catalogue changed since
    if (which == BHR_RAYMAP_STARS) return bhr_stars_read_plane(ctx, BHR_RAYMAP_SCHWARZSCHILD, "bhr_raymap_read", out, bytes);
    return bhr_raymap_read_plane(ctx, ctx->raymap, "bhr_raymap_read", which, out, bytes);
}

int32_t bhr_raymap_get_info(bhr_ctx *ctx, bhr_raymap_info *out) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_get_info: bad argument");
    if (!bhr_raymap_fill_info(ctx, ctx->raymap, out)) return BHR_OK;
    out->diff = ctx->raymap->diff;
    out->supersample = ctx->raymap->ss;
    return BHR_OK;
}

int32_t bhr_raymap_free(bhr_ctx *ctx) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_raymap_free: null ctx");
    return bhr_raymap_free_map(ctx, &ctx->raymap);
}

}  // extern "C"
