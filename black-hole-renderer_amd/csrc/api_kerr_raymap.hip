// api_kerr_raymap.hip -- the Kerr ray map's entry points (include/bhr.h): build, read, info, free, and the refusals of
// bhr_kerr_raymap_render, bhr_kerr_raymap_render_view and bhr_kerr_raymap_render_shutter (the frames themselves are launched from render.hip, next to
// bhr_raymap_render: they take a frame slot like any other).  The map is a bhr_raymap object of its own, ctx->kerr_raymap, of
// the Kerr kind; nothing of the Schwarzschild map's state is shared or touched.  This file holds what is Kerr's alone -- what
// such a map asks of a context, of a build and of a frame; building, reading and freeing the object is api_raymap.hip's, for
// both kinds.  The kernels are march_kerr_raymap.hip's, their launchers march_launch.hip's.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bhr_internal.h"

namespace {

const char *redshift_name(int32_t mode) { return mode == BHR_REDSHIFT_EXACT ? "exact" : "model"; }

// What the Kerr march refuses of a context (tilt, anti-aliasing, Disk V2, adaptive supersampling, row blocks), and supersampling:
// the context marches one Kerr ray per pixel for every map call (a supersampled map has a factor of its own, option
// "kerr_raymap_supersample" = map_ss, which the refusal names when it is on).
int32_t check_context(const bhr_ctx *ctx, const char *who, int32_t map_ss = 1) {
    BHR_TRY(bhr_variant_frame_check(ctx, bhr_variant_of(ctx), 0, who, (double)ctx->kerr_spin));
    if (ctx->ss > 1 && map_ss > 1)
        return bhr_fail(BHR_ERR_INVALID, "%s: supersampling is on (factor %d); a Kerr ray map holds one ray per pixel -- kerr_raymap_supersample %d is the map's own factor, bhr_set_supersample stays at 1", who, ctx->ss, map_ss);
    if (ctx->ss > 1) return bhr_fail(BHR_ERR_INVALID, "%s: supersampling is on (factor %d); a Kerr ray map holds one ray per pixel", who, ctx->ss);
    return BHR_OK;
}

}  // namespace

// cam null: bhr_kerr_raymap_render (the build camera, no turn); else bhr_kerr_raymap_render_view, whose camera has to be the
// build's turned rigidly about z.
int32_t bhr_kerr_raymap_check_render(bhr_ctx *ctx, const char *who, const bhr_camera *cam, float t_offset, uint32_t flags, float *rot_c, float *rot_s) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "%s: null ctx", who);
    if (flags & ~(uint32_t)(BHR_SKIP_BLOOM | BHR_LENS_FLARE))
        return bhr_fail(BHR_ERR_INVALID, "%s: flags %u (BHR_SKIP_BLOOM and BHR_LENS_FLARE only)", who, flags);
    if (!isfinite(t_offset)) return bhr_fail(BHR_ERR_INVALID, "%s: t_offset is not finite", who);
    const bhr_raymap *rm = ctx->kerr_raymap;
    if (!rm || !rm->built) return bhr_fail(BHR_ERR_STATE, "%s: no Kerr ray map has been built (bhr_kerr_raymap_build)", who);
    // a Kerr ray's path depends on the spin, a record's meaning on the redshift mode (to_cam or the photon's momentum)
    if (!ctx->kerr_on || ctx->kerr_spin != rm->kerr_spin || ctx->kerr_redshift != rm->kerr_redshift)
        return bhr_fail(BHR_ERR_STATE, "%s: the map was built for spin %g with the %s redshift, the context now has %s %g with the %s redshift; build it again (bhr_kerr_raymap_build)",
                        who, (double)rm->kerr_spin, redshift_name(rm->kerr_redshift), ctx->kerr_on ? "spin" : "no Kerr march, spin",
                        (double)ctx->kerr_spin, redshift_name(ctx->kerr_redshift));
    BHR_TRY(check_context(ctx, who));
    if (cam) BHR_TRY(bhr_raymap_turn_of_build(rm->cam, cam, who, rot_c, rot_s));
    // a Kerr polarisation (bhr_set_kerr_polarization): the Stokes kernel walks the build view's records and needs the photon's
    // momentum with each, which only a build under the polarisation keeps
    if (bhr_have_kerr_polar(ctx)) {
        if (cam && !(*rot_c == 1.0f && *rot_s == 0.0f))
            return bhr_fail(BHR_ERR_STATE, "%s: a Kerr polarisation is set (bhr_set_kerr_polarization) and the Stokes planes are the build view's; turned views have none -- switch it off (NULL) first", who);
        if (!rm->has_mom)
            return bhr_fail(BHR_ERR_STATE, "%s: a Kerr polarisation is set (bhr_set_kerr_polarization) and the map was built without the photon momenta it needs; build it again (bhr_kerr_raymap_build)", who);
    }
    // a Kerr line (bhr_set_kerr_line): the line pass walks the build view's records of a k = 1 map into a reserved row
    BHR_TRY(bhr_kerr_line_check_render(ctx, rm, who, cam && !(*rot_c == 1.0f && *rot_s == 0.0f), false));
    // Kerr point stars (bhr_set_kerr_stars): a supersampled Kerr map's shade kernels have no STARS variant
    return bhr_stars_check_map(ctx, BHR_RAYMAP_KERR, who);
}

// bhr_kerr_raymap_render_shutter's refusals (include/bhr.h), before anything is launched: everything bhr_kerr_raymap_render
// refuses, then the samples as bhr_raymap_check_render_shutter takes them -- a sample with the build camera's pose, field for
// field, is the still camera, turn (1, 0); any other has to be a turn of the build camera about z (the spin axis: no tilt to ask
// about, the Kerr march refuses one).
int32_t bhr_kerr_raymap_check_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags, BhrShutterArgs *smp, bool *turned) {
    const char *who = "bhr_kerr_raymap_render_shutter";
    if (!ctx || !cams) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    if (n < 1 || n > BHR_SHUTTER_MAX_SAMPLES) return bhr_fail(BHR_ERR_INVALID, "%s: %d samples (1 .. %d)", who, n, BHR_SHUTTER_MAX_SAMPLES);
    if (flags & ~(uint32_t)(BHR_SKIP_BLOOM | BHR_LENS_FLARE))
        return bhr_fail(BHR_ERR_INVALID, "%s: flags %u (BHR_SKIP_BLOOM and BHR_LENS_FLARE only)", who, flags);
    for (int j = 0; j < n; ++j)
        if (!isfinite(cams[j].t_offset)) return bhr_fail(BHR_ERR_INVALID, "%s: sample %d: t_offset is not finite", who, j);
    BHR_TRY(bhr_kerr_disk_refuse(ctx, who, "a shutter frame from the Kerr ray map shades the disk texture"));
    // the Kerr Stokes kernel walks one frame's records: a mean of frames has no Stokes planes (bhr_raymap_render_shutter likewise)
    if (bhr_have_kerr_polar(ctx))
        return bhr_fail(BHR_ERR_STATE, "%s: a Kerr polarisation is set (bhr_set_kerr_polarization) and shutter frames from the map have no Stokes planes -- switch it off (NULL) first", who);
    // ... and no line profile (bhr_set_kerr_line)
    if (ctx->kerr_raymap) BHR_TRY(bhr_kerr_line_check_render(ctx, ctx->kerr_raymap, who, false, true));
    float c1 = 1.0f, s0 = 0.0f;
    BHR_TRY(bhr_kerr_raymap_check_render(ctx, who, nullptr, 0.0f, flags, &c1, &s0));
    const bhr_camera &b = ctx->kerr_raymap->cam;
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
        BHR_TRY(bhr_raymap_turn_of_build(b, &c, sample, &o.c, &o.s));
        *turned = *turned || !(o.c == 1.0f && o.s == 0.0f);
    }
    smp->n = n;
    smp->inv = 1.0f / (float)n;
    // Kerr point stars: the fused and the supersampled shade kernels have no STARS variant
    return bhr_stars_check_shutter(ctx, BHR_RAYMAP_KERR, who);
}

extern "C" {

int32_t bhr_kerr_raymap_build(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags) {
    const char *who = "bhr_kerr_raymap_build";
    if (!ctx || !cam) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    if (ctx->rows != ctx->cfg.height)      // (such a context takes no spin either: said first, as what it is)
        return bhr_fail(BHR_ERR_INVALID, "%s: needs a whole-frame context (rows %d of %d)", who, ctx->rows, ctx->cfg.height);
    if (!ctx->kerr_on)
        return bhr_fail(BHR_ERR_STATE, "%s: no spin is set and the Kerr march is not forced (bhr_set_spin, bhr_set_redshift); bhr_raymap_build is the ray map of a hole that does not spin", who);
    if (flags) return bhr_fail(BHR_ERR_INVALID, "%s: flags %u (none are defined)", who, flags);
    // the map's own factor: the map of the fine frame, k rows x k W (the context's own supersampling stays off, check_context)
    const int32_t ss = ctx->opt.kerr_raymap_ss;
    BHR_TRY(check_context(ctx, who, ss));
    BHR_TRY(bhr_kerr_disk_refuse(ctx, who, "a frame from the Kerr ray map shades the disk texture"));
    if (ctx->kerr_aa)
        return bhr_fail(BHR_ERR_INVALID, "%s: the Kerr anti-aliasing is on (bhr_set_kerr_anti_alias) and a Kerr ray map's record has no differential words; switch it off first", who);
    const int32_t K = ctx->opt.raymap_slots;
    if (K < 1 || K > 8) return bhr_fail(BHR_ERR_INVALID, "%s: raymap_slots %d (1 .. 8)", who, K);
    if (ctx->opt.raymap_ss != 1)
        return bhr_fail(BHR_ERR_INVALID, "%s: raymap_supersample %d; a Kerr ray map has no supersampled form (1 only)", who, ctx->opt.raymap_ss);
    if (ss != 1 && ss != 2 && ss != 4 && ss != 8) return bhr_fail(BHR_ERR_INVALID, "%s: kerr_raymap_supersample %d (1, 2, 4 or 8)", who, ss);
    if ((int64_t)ss * ss * ctx->cfg.width * ctx->cfg.height >= ((int64_t)1 << 31))
        return bhr_fail(BHR_ERR_INVALID, "%s: %d x %d rays of a %dx%d frame exceed 2^31", who, ss, ss, ctx->cfg.width, ctx->cfg.height);
    // the momentum build and the Kerr Stokes kernel have no supersampled twin
    if (ss > 1 && bhr_have_kerr_polar(ctx))
        return bhr_fail(BHR_ERR_INVALID, "%s: kerr_raymap_supersample %d while a Kerr polarisation is set (bhr_set_kerr_polarization); the Stokes planes need a map with one ray per pixel -- set the factor to 1 or switch the polarisation off (NULL) first", who, ss);
    // ... and the Kerr line pass none either
    if (ss > 1 && bhr_have_kerr_line(ctx))
        return bhr_fail(BHR_ERR_INVALID, "%s: kerr_raymap_supersample %d while a Kerr line is set (bhr_set_kerr_line); the line pass needs a map with one ray per pixel -- set the factor to 1 or switch the line off (NULL) first", who, ss);
    BHR_TRY(bhr_kerr_camera_check(ctx, cam, who));
    // k x k Kerr rays per pixel, no differentials; the context's variant (BHR_MV_KERR or BHR_MV_KERR_EXACT) marches them
    return bhr_raymap_build_into(ctx, &ctx->kerr_raymap, who, cam, BHR_SKIP_DIFFERENTIALS, bhr_variant_of(ctx), K, ss);
}

int32_t bhr_kerr_raymap_read(bhr_ctx *ctx, int32_t which, void *out, int64_t bytes) {
    const char *who = "bhr_kerr_raymap_read";
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "%s: bad argument", who);
    if (!ctx->kerr_raymap || !ctx->kerr_raymap->built) return bhr_fail(BHR_ERR_STATE, "%s: no Kerr ray map has been built (bhr_kerr_raymap_build)", who);
    // the build view's star plane under the Kerr catalogue, gathered now if the map or the catalogue changed since
    if (which == BHR_RAYMAP_STARS) return bhr_stars_read_plane(ctx, BHR_RAYMAP_KERR, who, out, bytes);
    // the per-record g and w planes of the last frame whose Kerr line pass kept them (option "kerr_line_samples")
    if (which == BHR_RAYMAP_LINE_G || which == BHR_RAYMAP_LINE_W) return bhr_kerr_line_read_samples(ctx, who, which, out, bytes);
    if (which == BHR_RAYMAP_MOMENTUM) {
        // the momentum planes of a build under a Kerr polarisation: [slot][component][pixel] on the device, [slot][pixel][component] out
        const bhr_raymap *rm = ctx->kerr_raymap;
        if (!rm->has_mom) return bhr_fail(BHR_ERR_STATE, "%s: the map was built without the photon momenta (bhr_set_kerr_polarization, then bhr_kerr_raymap_build)", who);
        const size_t plane = (size_t)rm->a.plane, want = (size_t)rm->a.slots * 3 * plane * sizeof(float);
        if (bytes != (int64_t)want) return bhr_fail(BHR_ERR_INVALID, "%s: plane %d has %zu bytes, caller gave %lld", who, which, want, (long long)bytes);
        BHR_TRY(bhr_enter(ctx));
        std::vector<float> tmp((size_t)rm->a.slots * 3 * plane);
        BHR_HIP(hipMemcpyAsync(tmp.data(), rm->mom, want, hipMemcpyDeviceToHost, ctx->stream));
        BHR_HIP(hipStreamSynchronize(ctx->stream));
        float *o = (float *)out;
        for (size_t s = 0; s < (size_t)rm->a.slots; ++s)
            for (size_t c = 0; c < 3; ++c)
                for (size_t p = 0; p < plane; ++p) o[(s * plane + p) * 3 + c] = tmp[(s * 3 + c) * plane + p];
        return BHR_OK;
    }
    return bhr_raymap_read_plane(ctx, ctx->kerr_raymap, who, which, out, bytes);
}

int32_t bhr_kerr_raymap_info(bhr_ctx *ctx, bhr_kerr_raymap_desc *out) {
    if (!ctx || !out) return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_raymap_info: bad argument");
    if (!bhr_raymap_fill_info(ctx, ctx->kerr_raymap, out)) return BHR_OK;
    out->redshift = ctx->kerr_raymap->kerr_redshift;
    out->spin = ctx->kerr_raymap->kerr_spin;
    return BHR_OK;
}

// never fails for want of a map: 1 then
int32_t bhr_kerr_raymap_get_supersample(bhr_ctx *ctx, int32_t *k) {
    if (!ctx || !k) return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_raymap_get_supersample: bad argument");
    const bhr_raymap *rm = ctx->kerr_raymap;
    *k = rm && rm->built ? rm->ss : 1;
    return BHR_OK;
}

int32_t bhr_kerr_raymap_free(bhr_ctx *ctx) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_raymap_free: null ctx");
    return bhr_raymap_free_map(ctx, &ctx->kerr_raymap);
}

}  // extern "C"
