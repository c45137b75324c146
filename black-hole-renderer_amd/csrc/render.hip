// render.hip -- the kinds of frame on a frame slot (marched, under any march variant; shutter; from a ray map of either kind,
// its view and its shutter), and the one place that rotates the slots and keeps the last frame's record.
// One frame: march -> bloom H -> bloom V + combine (-> lens flare).  Frames alternate between the context's two
// frame slots (bhr_frame_slot): frame n + 1 is launched on the other slot's stream into its own buffers and overlaps
// the tail and the post-passes of frame n.  The scene is only read; everything that writes it or reads a frame goes
// through bhr_enter, which orders the scene stream behind both slots.
#include <math.h>

#include "bhr_internal.h"

namespace {

// What a frame's body reports back for the last-frame record (frame_on_next_slot): its marches' supersampling factor, how many
// of them the frame is the mean of, and whether each was refined adaptively.
struct frame_marches {
    int32_t ss, samples;
    bool adaptive;
};

// The post-pass of the frame on slot k behind its march (a shutter frame's: behind the last accumulation and the pack):
// bloom H -> bloom V + combine (-> lens flare), and the frame's end events.
int32_t post_on_slot(bhr_ctx *ctx, uint32_t flags, int k, int ring) {
    bhr_frame_slot &f = ctx->slots[k];
    const int with_bloom = (flags & BHR_SKIP_BLOOM) ? 0 : 1;
    if (with_bloom) BHR_TRY(bhr_launch_bloom_h(ctx, nullptr, 0));
    // the V kernel clears the counter cell BHR_MAX_FRAME_SLOTS frames ahead: no frame that may be in flight on another
    // slot's stream is counting into it (the next frames' marches may already be running)
    unsigned long long *zero_cell = ctx->d_steps_ring + (size_t)((ring + BHR_MAX_FRAME_SLOTS) % BHR_TIMING_RING) * BHR_STEP_CELL;
    // what the frame stores: the layers the context's consumers asked for (bhr_set_outputs); the lens flare works on the f32
    // frame, so a flared frame keeps it and quantises afterwards
    uint32_t want = ctx->out_want;
    if (flags & BHR_LENS_FLARE) want = (want | BHR_OUT_F32) & ~BHR_OUT_U8;
    if (ctx->dither) want = (want | BHR_OUT_F32) & ~BHR_OUT_U8;      // dithered rows: the same route (quantize.hip)
    // a graded frame (bhr_set_grade): the V pass stores BLUR only -- zeros for a BHR_SKIP_BLOOM frame -- and the grade kernel
    // writes FINAL, the authority for everything made on demand, and the undithered u8 rows where they are wanted (grade.hip)
    const bool graded = ctx->grade_on != 0;
    if (graded) want = BHR_OUT_BLUR;
    BHR_TRY(bhr_frame_post(ctx, with_bloom, want, zero_cell));
    if ((flags & BHR_LENS_FLARE) && ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "bhr_render: the lens flare needs whole-frame sums; use bhr_group_render for row blocks");
    if (graded) {
        const bool keep = ctx->grade.keep_hdr != 0, rows_u8 = (ctx->out_want & BHR_OUT_U8) && !ctx->dither;
        if (flags & BHR_LENS_FLARE) {
            // the flare sits in front of the sensor response: s -> the HDR plane, + flare without the upper clip, then the grade
            BHR_TRY(bhr_launch_grade_sum(ctx));
            BHR_TRY(bhr_frame_flare(ctx, true));
            BHR_TRY(bhr_launch_grade(ctx, true, true, rows_u8));
        } else {
            BHR_TRY(bhr_launch_grade(ctx, false, keep, rows_u8));
        }
        f.have |= BHR_OUT_F32 | (keep ? BHR_OUT_HDR : 0u) | (rows_u8 ? BHR_OUT_U8 : 0u);
        if (ctx->dither && (ctx->out_want & BHR_OUT_U8)) BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_U8));
    } else if (flags & BHR_LENS_FLARE) {
        // every slot has its own flare scratch (glow, sums): the frames' flare passes overlap like the rest
        BHR_TRY(bhr_frame_flare(ctx, false));
        if (ctx->out_want & BHR_OUT_U8) BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_U8));
    } else if (ctx->dither && (ctx->out_want & BHR_OUT_U8)) {
        BHR_TRY(bhr_ensure_outputs(ctx, BHR_OUT_U8));
    }
    BHR_HIP(hipEventRecord(ctx->ring_ev[ring * 3 + 2], f.stream));
    BHR_HIP(hipEventRecord(f.done, f.stream));
    return BHR_OK;
}

// One marched frame on slot k.  req: the march variant of the frame with its payload, resolved by the entry point (none: the
// context's arithmetic picks the march).
int32_t render_on_slot(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags, int k, int ring, frame_marches *fm, const bhr_variant_request &req) {
    bhr_frame_slot &f = ctx->slots[k];
    BHR_TRY(bhr_frame_begin(ctx, flags));
    // an adaptively supersampled frame: the k = 1 march, then detect + refinement inside the same march bracket
    const bool adaptive = ctx->ada_k > 1;
    const bhr_march_call call = {cam, flags, f.stream, /* slot */ ring, /* time_untimed */ false, /* defer_end */ adaptive, ctx->ss, /* keep_start */ false, req};
    *fm = {call.ss, 1, adaptive};
    BHR_TRY(bhr_launch_march(ctx, call));              // records the ring slot's march events
    if (adaptive) BHR_TRY(bhr_launch_adaptive(ctx, call));
    // the march's end is the timing ring's event (recorded by the launcher): an event of its own between the march and the
    // H pass is another ~5 us barrier packet in the frame's stream (kernel-trace gaps: 10 us with two records, 0 with none)
    f.march_done = ctx->ring_ev[ring * 3 + 1];
    return post_on_slot(ctx, flags, k, ring);
}

// The end of a shutter frame on slot k, marched or from the ray map: closes the march bracket behind the last sample -- the
// samples count into the frame's one ring cell and share its events -- then the post-pass on the resolved layers.
int32_t shutter_close_on_slot(bhr_ctx *ctx, uint32_t flags, int k, int ring) {
    bhr_frame_slot &f = ctx->slots[k];
    BHR_HIP(hipEventRecord(ctx->ring_ev[ring * 3 + 1], f.stream));
    f.march_done = ctx->ring_ev[ring * 3 + 1];
    if (f.frame_split) BHR_TRY(bhr_launch_bloom_pack(ctx));            // the resolved disk layer -> the H pass's operands, bg + disk
    return post_on_slot(ctx, flags, k, ring);
}

// A shutter frame on slot k (bhr_render_shutter): n skip-bloom marches into the slot's layers, each followed by its
// accumulation launch (shutter.hip), then the post-pass on the resolved layers as bhr_bloom runs it.  All on the slot's
// stream; a two-stream hybrid sample forks onto the slot's second stream and joins before its accumulation, and the next
// sample's fork waits for that accumulation.  The samples count into the frame's one ring cell and share its events: the
// march bracket runs from the first sample's start to behind the last accumulation.
int32_t shutter_on_slot(bhr_ctx *ctx, const bhr_camera *cams, int n, uint32_t flags, int k, int ring, frame_marches *fm) {
    bhr_frame_slot &f = ctx->slots[k];
    BHR_TRY(bhr_frame_begin(ctx, flags));              // the frame's post-pass and its buffers, before anything is launched
    const bool adaptive = ctx->ada_k > 1;
    *fm = {ctx->ss, n, adaptive};
    for (int j = 0; j < n; ++j) {
        // skip-bloom marches: they leave the split post-pass's packed operands alone
        const bhr_march_call call = {&cams[j], flags | BHR_SKIP_BLOOM, f.stream, /* slot */ ring, /* time_untimed */ false, /* defer_end */ true, ctx->ss,
                                     /* keep_start */ j > 0};
        BHR_TRY(bhr_launch_march(ctx, call));
        if (adaptive) BHR_TRY(bhr_launch_adaptive(ctx, call));
        if (n > 1) BHR_TRY(bhr_launch_shutter_accumulate(ctx, j, n));
    }
    return shutter_close_on_slot(ctx, flags, k, ring);
}

// The fix launch of a map frame: the strict fix kernel over the map's overflow list (a grid for the list's capacity).
bhr_march_part raymap_fix_part(const bhr_raymap &rm) {
    return {nullptr, 0, /* first */ 0, /* last */ 1, BHR_MATH_STRICT, /* repair */ 2, rm.a.over_count, rm.a.over_list, rm.over_cap};
}

// The launches of one frame from the map `rm` under `call`: the shade kernel over the stored records, turned by (c, s), then the
// strict fix kernel over the overflow list (which, unless the call defers it, records the ring slot's march-end event).
// With a star catalogue of the map's own kind set (bhr_set_stars; a Kerr map's bhr_set_kerr_stars) the view's star plane comes
// first -- the cached one of the build view, or the gather of the turned view into the slot's own plane, on the frame's stream
// ahead of its march bracket -- and the shade kernel is the STARS one.  A map asks its own kind's catalogue and never the other.
// Under call's Kerr variant both launches take the Kerr map's kernels (march_launch.hip).
int32_t raymap_frame_launches(bhr_ctx *ctx, const bhr_march_call &call, const bhr_raymap &rm, float c, float s) {
    const float *stars = nullptr;
    if (bhr_have_stars(ctx, rm.kind)) BHR_TRY(bhr_stars_frame_plane(ctx, rm.kind, call.cam, c, s, &stars));
    BHR_TRY(bhr_launch_raymap_shade(ctx, call, rm.a, rm.diff != 0, c, s, stars));
    const bhr_march_part part = raymap_fix_part(rm);
    return bhr_launch_march(ctx, call, &part);
}

// A frame from the map `rm` on slot k (bhr_raymap_render, bhr_kerr_raymap_render): the shade kernel over the stored records, then
// the fix kernel over the map's overflow list (its count is the device's: a grid for the list's capacity, as the hybrid march
// launches it), inside one march bracket, then the post-pass as behind any march.  The ring cell counts the re-march only.
// rot_c, rot_s: the turn of `cam` from the build camera (the _render_view calls; 1, 0 for the build view).  The fix kernel
// marches the overflow pixels from `cam`, the frame's own camera.  A Kerr map's frame runs under the context's Kerr variant.
int32_t raymap_on_slot(bhr_ctx *ctx, const bhr_raymap &rm, const bhr_camera *cam, uint32_t flags, int k, int ring, frame_marches *fm, float rot_c = 1.0f, float rot_s = 0.0f) {
    bhr_frame_slot &f = ctx->slots[k];
    const bool kerr = rm.kind == BHR_RAYMAP_KERR;
    BHR_TRY(bhr_frame_begin(ctx, flags));
    // a supersampled map: the call carries the map's factor, so both launches work on the fine frame and the fix launch takes
    // march_fix_ss_kernel, which resolves the overflow list's whole groups
    const bhr_march_call call = {cam, flags, f.stream, /* slot */ ring, /* time_untimed */ false, /* defer_end */ false, /* ss */ rm.ss, /* keep_start */ false,
                                 {kerr ? bhr_variant_of(ctx) : BHR_MV_NONE}};
    *fm = {rm.ss, 1, false};
    BHR_TRY(raymap_frame_launches(ctx, call, rm, rot_c, rot_s));
    f.march_done = ctx->ring_ev[ring * 3 + 1];
    // a polarisation is set (bhr_set_polarization): the Stokes pass over the same records into the slot's own planes, behind the
    // frame's march bracket and ahead of its post-pass -- the frame's end event covers it, so a read waits for it like for the rest.
    // It reads the scene (shade_hit samples the disk texture), so it replaces f.march_done by an event of the slot's own behind it.
    // The Schwarzschild kind's alone.
    if (!kerr && bhr_have_polar(ctx)) {
        BHR_TRY(bhr_polar_frame(ctx, call, rm));
        ctx->stokes_slot = k;
    }
    // ... and a Kerr map's frame under a Kerr polarisation (bhr_set_kerr_polarization) by the Kerr Stokes kernel, likewise
    if (kerr && bhr_have_kerr_polar(ctx)) {
        BHR_TRY(bhr_kerr_polar_frame(ctx, call, rm));
        ctx->stokes_slot = k;
    }
    // ... and under a Kerr line (bhr_set_kerr_line) by the line pass into the device row of option "kerr_line_row", behind both
    if (kerr && bhr_have_kerr_line(ctx)) BHR_TRY(bhr_kerr_line_frame(ctx, call, rm, k));
    return post_on_slot(ctx, flags, k, ring);
}

// A shutter frame from the context's ray map on slot k (bhr_raymap_render_shutter): the mean of n frames from the map, then the
// post-pass on the resolved layers as behind shutter_on_slot's last accumulation.  Two routes to the same bits.  Fused (a map
// without overflow pixels, option "raymap_shutter_fused" not 0, n > 1): one launch shades every pixel under all n samples and
// stores the mean.  Unfused: shutter_on_slot with a map frame in place of each march -- the shade launch and the strict fix
// launch over the overflow list as raymap_on_slot issues them, as a skip-bloom call, then the accumulation launch; a later
// sample keeps the frame's march-start event and the march-end event is recorded once behind the last accumulation.
// The map `rm` is of either kind.  A Kerr map's frame (bhr_kerr_raymap_render_shutter) runs under the context's Kerr variant:
// both routes' launches take the Kerr map's kernels by the call's variant, and its option is
// "kerr_raymap_shutter_fused".
int32_t raymap_shutter_on_slot(bhr_ctx *ctx, const bhr_raymap &rm, const bhr_camera *cams, const BhrShutterArgs &smp, bool turned, uint32_t flags, int k, int ring,
                               frame_marches *fm) {
    bhr_frame_slot &f = ctx->slots[k];
    const bool kerr = rm.kind == BHR_RAYMAP_KERR;
    const bhr_variant_request req = {kerr ? bhr_variant_of(ctx) : BHR_MV_NONE};
    const bool fused = kerr ? ctx->opt.kerr_raymap_shutter_fused != 0 : ctx->opt.raymap_shutter_fused != 0;
    const int n = smp.n;
    // the layers are the strict arithmetic's; the post-pass on the resolved layers is the one bhr_bloom would run on them in this
    // context -- the context's arithmetic decides its kernels (exact f32 under strict, split f16 under fast / hybrid)
    BHR_TRY(bhr_frame_begin(ctx, flags & ~(uint32_t)BHR_FORCE_STRICT));
    *fm = {rm.ss, n, false};
    ctx->shutter_ev_n = 0;            // option "shutter_timing": the fused route has no accumulation launch to bracket
    // (a supersampled map always goes sample by sample: there is no fused supersampled kernel, whatever "raymap_shutter_fused" says)
    if (n > 1 && rm.overflow_pixels == 0 && fused && rm.ss == 1) {
        // no march launch follows the fused one: nothing counts into the frame's counter cell, which was cleared ahead of time
        const bhr_march_call call = {&cams[0], flags | BHR_SKIP_BLOOM, f.stream, /* slot */ ring, /* time_untimed */ false, /* defer_end */ true, /* ss */ 1,
                                     /* keep_start */ false, req};
        BHR_TRY(bhr_launch_raymap_shade_shutter(ctx, call, rm.a, rm.diff != 0, smp, turned));
    } else {
        for (int j = 0; j < n; ++j) {
            const bhr_march_call call = {&cams[j], flags | BHR_SKIP_BLOOM, f.stream, /* slot */ ring, /* time_untimed */ false, /* defer_end */ true, /* ss */ rm.ss,
                                         /* keep_start */ j > 0, req};
            BHR_TRY(raymap_frame_launches(ctx, call, rm, smp.smp[j].c, smp.smp[j].s));
            if (n > 1) BHR_TRY(bhr_launch_shutter_accumulate(ctx, j, n));
        }
    }
    return shutter_close_on_slot(ctx, flags, k, ring);
}

// A frame on the context's next frame slot: orders the slot's stream behind the scene stream, points the launchers at the
// slot, runs `body(slot, ring slot, what it marched)` and keeps the books (slot rotation, timing ring, the last frame's record --
// only for a body that launched everything: a failed frame leaves the record of the one before it whole).  exclusive: slot 0,
// behind every frame in flight (launches that use per-context scratch).
template <class Body>
int32_t frame_on_next_slot(bhr_ctx *ctx, uint32_t flags, bool exclusive, Body body) {
    ctx->stream = ctx->scene_stream;
    if (exclusive) BHR_TRY(bhr_enter(ctx));
    const int k = (ctx->n_slots > 1 && !exclusive) ? ctx->next_slot : 0;
    BHR_TRY(bhr_alloc_slot(ctx, k));
    bhr_frame_slot &f = ctx->slots[k];
    if (!(flags & BHR_SKIP_BLOOM)) BHR_TRY(bhr_bloom_prepare(ctx));   // one-off tables, on the scene stream
    if (f.stream != ctx->scene_stream) {
        BHR_HIP(hipEventRecord(ctx->scene_ev, ctx->scene_stream));    // everything the scene stream has been given so far
        BHR_HIP(hipStreamWaitEvent(f.stream, ctx->scene_ev, 0));
    }
    const int ring = (int)(ctx->ring_head % BHR_TIMING_RING);
    ctx->active_slot = k;
    ctx->stream = f.stream;
    frame_marches fm = {1, 1, false};
    const int32_t rc = body(k, ring, &fm);
    ctx->stream = ctx->scene_stream;
    f.in_flight = 1;
    BHR_TRY(rc);
    if (ctx->n_slots > 1 && !exclusive) ctx->next_slot = (k + 1) % ctx->n_slots;
    ctx->ring_head += 1;
    // every frame here is timed: its march bracket is its ring slot's, closed by the launcher or by shutter_close_on_slot
    const bhr_fine_frame fr = bhr_fine(ctx, fm.ss);
    ctx->last = {1, ring, /* march_timed */ 1, flags, (uint64_t)fr.width * fr.rows * (uint64_t)fm.samples, fm.adaptive};
    if (fm.adaptive) {
        ctx->ada_info_slot = k;
        ctx->ada_info_math = bhr_resolve_math(ctx, flags);
    }
    return BHR_OK;
}

// The flag word of a frame from the map: the strict arithmetic, the build's choice of differentials.
uint32_t raymap_frame_flags(const bhr_ctx *ctx, uint32_t flags) {
    return flags | BHR_FORCE_STRICT | (ctx->raymap->diff ? 0u : BHR_SKIP_DIFFERENTIALS);
}

}  // namespace

extern "C" {

int32_t bhr_render(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags) {
    if (!ctx || !cam) return bhr_fail(BHR_ERR_INVALID, "bhr_render: null argument");
    const bhr_variant_request req = {bhr_variant_of(ctx)};          // a spin, the exact redshift: the context's own variant
    BHR_TRY(bhr_variant_frame_check(ctx, req.variant, flags, "bhr_render", (double)ctx->kerr_spin));
    BHR_TRY(bhr_kerr_camera_check(ctx, cam, "bhr_render"));
    if ((ctx->ss > 1 || ctx->ada_k > 1) && (flags & (BHR_PERSISTENT | BHR_ROW_COSTS)))
        return bhr_fail(BHR_ERR_INVALID, "bhr_render: BHR_PERSISTENT and BHR_ROW_COSTS are not available with supersampling (factor %d)", ctx->ss > 1 ? ctx->ss : ctx->ada_k);
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    if (ctx->n_slots > 1 && ctx->opt.calibrate_streams && !ctx->streams_calibrated && !ctx->calibrating &&
        !(flags & (BHR_PERSISTENT | BHR_ROW_COSTS)) && ++ctx->two_slot_frames > 8)
        BHR_TRY(bhr_calibrate_slot_streams(ctx, cam, flags));
    // launches that use per-context scratch (work queue of the persistent schedule, row-cost profile) stay on one slot
    const bool exclusive = (flags & (BHR_PERSISTENT | BHR_ROW_COSTS)) != 0;
    return frame_on_next_slot(ctx, flags, exclusive, [&](int k, int ring, frame_marches *fm) { return render_on_slot(ctx, cam, flags, k, ring, fm, req); });
}

// The frame of a request that names its variant (bhr_render_observer, bhr_render_projected, bhr_render_delayed,
// bhr_render_kerr_view), behind the
// entry point's checks of its own payload: the variant's refusals (bhr_variant_frame_check), then the frame.  Everything that
// can refuse does so before the frame takes a slot; like bhr_render_shutter the frame neither triggers nor counts towards the
// calibration of slot 1's stream.
static int32_t variant_frame(bhr_ctx *ctx, const bhr_camera *cam, const bhr_variant_request &req, uint32_t flags, const char *who) {
    BHR_TRY(bhr_variant_frame_check(ctx, req.variant, flags, who, (double)ctx->kerr_spin));
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    return frame_on_next_slot(ctx, flags, false, [&](int k, int ring, frame_marches *fm) { return render_on_slot(ctx, cam, flags, k, ring, fm, req); });
}

// The velocity of a moving camera, as bhr_render_observer and bhr_render_projected take it.
static int32_t observer_beta_check(const bhr_observer *obs, const char *who) {
    const double b2 = (double)obs->beta[0] * obs->beta[0] + (double)obs->beta[1] * obs->beta[1] + (double)obs->beta[2] * obs->beta[2];
    if (!(b2 <= 0.995 * 0.995))       // a NaN fails the comparison too
        return bhr_fail(BHR_ERR_INVALID, "%s: observer velocity (%g, %g, %g): |beta| = %g, at most 0.995 and no NaN", who, (double)obs->beta[0],
                        (double)obs->beta[1], (double)obs->beta[2], sqrt(b2));
    return BHR_OK;
}

// The kind and the field of view of a panoramic camera, as bhr_render_projected and bhr_render_kerr_view take them.
static int32_t projection_check(const bhr_projection *proj, const char *who) {
    if (proj->kind != BHR_PROJ_EQUIRECT && proj->kind != BHR_PROJ_FISHEYE)
        return bhr_fail(BHR_ERR_INVALID, "%s: projection kind %d (BHR_PROJ_EQUIRECT or BHR_PROJ_FISHEYE)", who, proj->kind);
    const bool eq = proj->kind == BHR_PROJ_EQUIRECT;
    if (!(proj->fov_h_deg > 0.0f && proj->fov_h_deg <= 360.0f))       // a NaN fails the comparison too
        return bhr_fail(BHR_ERR_INVALID, "%s: %s projection with fov_h_deg = %g: in (0, 360] and no NaN", who, eq ? "equirectangular" : "fisheye", (double)proj->fov_h_deg);
    if (eq && !(proj->fov_v_deg > 0.0f && proj->fov_v_deg <= 180.0f))
        return bhr_fail(BHR_ERR_INVALID, "%s: equirectangular projection with fov_v_deg = %g: in (0, 180] and no NaN", who, (double)proj->fov_v_deg);
    return BHR_OK;
}
static const bhr_observer observer_at_rest = {{0.0f, 0.0f, 0.0f}, 0};   // a call without a velocity: at rest, with a plain sky

// One frame as a moving camera sees it (include/bhr.h).
int32_t bhr_render_observer(bhr_ctx *ctx, const bhr_camera *cam, const bhr_observer *obs, uint32_t flags) {
    const char *who = "bhr_render_observer";
    if (!ctx || !cam || !obs) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    BHR_TRY(observer_beta_check(obs, who));
    return variant_frame(ctx, cam, {BHR_MV_OBSERVER, obs}, flags, who);
}

// One frame under an equirectangular or fisheye projection, from a camera that may move (include/bhr.h): bhr_render_observer's
// frame marched by the projected object.  obs null: the camera stands still, which is the observer at rest with a plain sky.
int32_t bhr_render_projected(bhr_ctx *ctx, const bhr_camera *cam, const bhr_projection *proj, const bhr_observer *obs, uint32_t flags) {
    const char *who = "bhr_render_projected";
    if (!ctx || !cam || !proj) return bhr_fail(BHR_ERR_INVALID, "%s: null argument (ctx, cam and proj are needed)", who);
    BHR_TRY(projection_check(proj, who));
    const bhr_observer o = obs ? *obs : observer_at_rest;
    BHR_TRY(observer_beta_check(&o, who));
    return variant_frame(ctx, cam, {BHR_MV_PROJECTED, &o, proj}, flags, who);
}

// One frame of the spinning hole through the Kerr camera (include/bhr.h): bhr_render's Kerr frame marched by the Kerr camera's
// object, under the context's redshift.  obs null: the camera hovers (the static observer); proj null: the pinhole.
int32_t bhr_render_kerr_view(bhr_ctx *ctx, const bhr_camera *cam, const bhr_observer *obs, const bhr_projection *proj, uint32_t flags) {
    const char *who = "bhr_render_kerr_view";
    if (!ctx || !cam) return bhr_fail(BHR_ERR_INVALID, "%s: null argument (ctx and cam are needed)", who);
    if (!ctx->kerr_on)
        return bhr_fail(BHR_ERR_INVALID, "%s: a Kerr view without the Kerr march: set a spin, or force_kerr at spin 0, first (bhr_set_spin)", who);
    if (ctx->kerr_aa)
        return bhr_fail(BHR_ERR_INVALID, "%s: a Kerr view with the Kerr anti-aliasing on (bhr_set_kerr_anti_alias): the differential seeds would need the aberration's Jacobian; switch it off first", who);
    BHR_TRY(bhr_kerr_disk_refuse(ctx, who, "the Kerr camera's march shades the disk texture"));
    if (proj) BHR_TRY(projection_check(proj, who));
    const bhr_observer o = obs ? *obs : observer_at_rest;
    BHR_TRY(observer_beta_check(&o, who));
    const bhr_march_variant v = ctx->kerr_redshift == BHR_REDSHIFT_EXACT ? BHR_MV_KERR_VIEW_EXACT : BHR_MV_KERR_VIEW;
    BHR_TRY(bhr_kerr_camera_check(ctx, cam, who));
    return variant_frame(ctx, cam, {v, &o, proj}, flags, who);
}

// One frame with every disk crossing shaded at its emission time (include/bhr.h): bhr_render's frame marched by the delay object.
int32_t bhr_render_delayed(bhr_ctx *ctx, const bhr_camera *cam, const bhr_light_delay *d, uint32_t flags) {
    const char *who = "bhr_render_delayed";
    if (!ctx || !cam || !d) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    if (!(d->scale >= 0.0f && d->scale <= 16.0f))       // a NaN fails the comparison too
        return bhr_fail(BHR_ERR_INVALID, "%s: light delay with scale = %g: in [0, 16] and no NaN", who, (double)d->scale);
    if (d->reserved != 0) return bhr_fail(BHR_ERR_INVALID, "%s: light delay with reserved = %d: must be 0", who, d->reserved);
    return variant_frame(ctx, cam, {BHR_MV_DELAYED, nullptr, nullptr, d}, flags, who);
}

// One frame as the mean of n marches (include/bhr.h).  One frame of one frame slot: the next frame takes the other slot.
// It neither triggers nor counts towards the calibration of slot 1's stream (the frames that does times are bhr_render's).
int32_t bhr_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags) {
    if (!ctx || !cams) return bhr_fail(BHR_ERR_INVALID, "bhr_render_shutter: null argument");
    BHR_TRY(bhr_kerr_refuse(ctx, "bhr_render_shutter", "shutter frames march Schwarzschild rays"));
    if (n < 1 || n > BHR_SHUTTER_MAX_SAMPLES) return bhr_fail(BHR_ERR_INVALID, "bhr_render_shutter: %d samples (1 .. %d)", n, BHR_SHUTTER_MAX_SAMPLES);
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "bhr_render_shutter: needs a whole-frame context (rows %d of %d)", ctx->rows, ctx->cfg.height);
    if (flags & (BHR_PERSISTENT | BHR_ROW_COSTS))
        return bhr_fail(BHR_ERR_INVALID, "bhr_render_shutter: BHR_PERSISTENT and BHR_ROW_COSTS are not available for shutter frames");
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    return frame_on_next_slot(ctx, flags, false, [&](int k, int ring, frame_marches *fm) { return shutter_on_slot(ctx, cams, n, flags, k, ring, fm); });
}

// A frame from the ray map (include/bhr.h): the build camera with the caller's t_offset, the strict arithmetic, the build's
// choice of differentials.  Like bhr_render_shutter it neither triggers nor counts towards the calibration of slot 1's stream.
int32_t bhr_raymap_render(bhr_ctx *ctx, float t_offset, uint32_t flags) {
    BHR_TRY(bhr_raymap_check_render(ctx, t_offset, flags));
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    bhr_camera cam = ctx->raymap->cam;
    cam.t_offset = t_offset;
    if (bhr_have_stars(ctx)) BHR_TRY(bhr_stars_ensure_plane(ctx));   // the build view's star plane, once per (map, catalogue)
    const uint32_t fl = raymap_frame_flags(ctx, flags);
    return frame_on_next_slot(ctx, fl, false, [&](int k, int ring, frame_marches *fm) { return raymap_on_slot(ctx, *ctx->raymap, &cam, fl, k, ring, fm); });
}

// A frame from the ray map seen from the build camera turned about z (include/bhr.h): bhr_raymap_render's frame in every other
// respect -- slot, timing ring, counters, post-pass and consumers.
int32_t bhr_raymap_render_view(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags) {
    float rot_c = 1.0f, rot_s = 0.0f;
    BHR_TRY(bhr_raymap_check_render_view(ctx, cam, flags, &rot_c, &rot_s));
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    const bhr_camera view = *cam;
    if (bhr_have_stars(ctx) && rot_c == 1.0f && rot_s == 0.0f) BHR_TRY(bhr_stars_ensure_plane(ctx));   // angle 0: bhr_raymap_render's plane
    const uint32_t fl = raymap_frame_flags(ctx, flags);
    return frame_on_next_slot(ctx, fl, false, [&](int k, int ring, frame_marches *fm) { return raymap_on_slot(ctx, *ctx->raymap, &view, fl, k, ring, fm, rot_c, rot_s); });
}

// A frame from the Kerr ray map (include/bhr.h): the build camera with the caller's t_offset, under the flags as they are -- the
// post-pass is the one behind a marched Kerr frame of this context.  Like bhr_raymap_render it neither triggers nor counts
// towards the calibration of slot 1's stream.
int32_t bhr_kerr_raymap_render(bhr_ctx *ctx, float t_offset, uint32_t flags) {
    float rot_c = 1.0f, rot_s = 0.0f;
    BHR_TRY(bhr_kerr_raymap_check_render(ctx, "bhr_kerr_raymap_render", nullptr, t_offset, flags, &rot_c, &rot_s));
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    bhr_camera cam = ctx->kerr_raymap->cam;
    cam.t_offset = t_offset;
    if (bhr_have_stars(ctx, BHR_RAYMAP_KERR)) BHR_TRY(bhr_stars_ensure_plane(ctx, BHR_RAYMAP_KERR));   // the build view's star plane, once per (Kerr map, Kerr catalogue)
    return frame_on_next_slot(ctx, flags, false, [&](int k, int ring, frame_marches *fm) { return raymap_on_slot(ctx, *ctx->kerr_raymap, &cam, flags, k, ring, fm); });
}

// ... seen from the build camera turned about z (include/bhr.h): bhr_kerr_raymap_render's frame in every other respect.
int32_t bhr_kerr_raymap_render_view(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags) {
    float rot_c = 1.0f, rot_s = 0.0f;
    if (!cam) return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_raymap_render_view: null argument");
    BHR_TRY(bhr_kerr_raymap_check_render(ctx, "bhr_kerr_raymap_render_view", cam, cam->t_offset, flags, &rot_c, &rot_s));
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    const bhr_camera view = *cam;
    if (bhr_have_stars(ctx, BHR_RAYMAP_KERR) && rot_c == 1.0f && rot_s == 0.0f) BHR_TRY(bhr_stars_ensure_plane(ctx, BHR_RAYMAP_KERR));   // angle 0: bhr_kerr_raymap_render's plane
    return frame_on_next_slot(ctx, flags, false, [&](int k, int ring, frame_marches *fm) { return raymap_on_slot(ctx, *ctx->kerr_raymap, &view, flags, k, ring, fm, rot_c, rot_s); });
}

// Motion blur from the ray map (include/bhr.h): one frame as the mean of n frames from the map, no march.  A frame like
// bhr_raymap_render's in slot, timing ring and calibration; the strict arithmetic, the build's choice of differentials.
int32_t bhr_raymap_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags) {
    BhrShutterArgs smp;
    bool turned = false;
    BHR_TRY(bhr_raymap_check_render_shutter(ctx, cams, n, flags, &smp, &turned));
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    const uint32_t fl = raymap_frame_flags(ctx, flags);
    return frame_on_next_slot(ctx, fl, false, [&](int k, int ring, frame_marches *fm) { return raymap_shutter_on_slot(ctx, *ctx->raymap, cams, smp, turned, fl, k, ring, fm); });
}

// Motion blur from the Kerr ray map (include/bhr.h): one frame as the mean of n frames from the Kerr map, no march.  A frame like
// bhr_kerr_raymap_render's in slot, timing ring and calibration, under the flags as they are and the context's Kerr variant.
int32_t bhr_kerr_raymap_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags) {
    BhrShutterArgs smp;
    bool turned = false;
    BHR_TRY(bhr_kerr_raymap_check_render_shutter(ctx, cams, n, flags, &smp, &turned));
    BHR_HIP(hipSetDevice(ctx->cfg.device));
    return frame_on_next_slot(ctx, flags, false,
                              [&](int k, int ring, frame_marches *fm) { return raymap_shutter_on_slot(ctx, *ctx->kerr_raymap, cams, smp, turned, flags, k, ring, fm); });
}

}  // extern "C"
