/*
 * bhr.h -- C ABI of libbhr_hip.so, the MI355X (gfx950) Schwarzschild ray tracer.
 *
 * The reference (hwuu/black-hole-renderer) has no FFI: its renderer boundary is
 * the Python class TaichiRenderer (render.py:2189-4028) whose device half is
 * JIT-compiled Taichi.  This header is the boundary a maintainer would bind in
 * its place; each entry point names the reference interface it replaces.  The
 * ctypes binding that mirrors TaichiRenderer lives in
 * black-hole-renderer_amd/renderer.py; INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - every call returns 0 on success or a negative bhr_status; bhr_last_error()
 *    returns a thread-local message for the last failure on the calling thread;
 *  - a bhr_ctx owns one HIP device, one stream and all its device buffers.  It
 *    is not thread-safe; distinct contexts may be driven from distinct threads
 *    or processes (one process per GPU, or one process driving N devices);
 *  - host pointers are plain row-major float32 arrays owned by the caller and
 *    copied during the call; nothing in this ABI is a torch/Taichi type;
 *  - images handed back to the host are (rows, width, 3) float32, x fastest,
 *    i.e. already in the (H, W, 3) order TaichiRenderer.render() returns after
 *    its final transpose (render.py:3923);
 *  - the library never falls back to a CPU path: without a HIP device
 *    bhr_create() fails with BHR_ERR_NO_DEVICE.
 */
#ifndef BHR_H
#define BHR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BHR_ABI_VERSION 1

#if defined(__GNUC__)
#define BHR_API __attribute__((visibility("default")))
#else
#define BHR_API
#endif

typedef struct bhr_ctx bhr_ctx;

typedef enum {
    BHR_OK = 0,
    BHR_ERR_INVALID = -1,      /* bad argument / shape mismatch (reference: AssertionError, ValueError) */
    BHR_ERR_NO_DEVICE = -2,    /* no usable HIP device */
    BHR_ERR_HIP = -3,          /* a HIP runtime call failed; see bhr_last_error() */
    BHR_ERR_STATE = -4,        /* call sequence violated (e.g. background before bhr_bg_init) */
    BHR_ERR_NOMEM = -5
} bhr_status;

/* Constructor arguments of TaichiRenderer.__init__ (render.py:2199-2208), plus
 * the device ordinal and the row block [row0,row1) of the image this context
 * renders (0,height for a whole frame; row blocks are the multi-GPU tiles). */
typedef struct {
    int32_t width, height;
    int32_t row0, row1;
    float step_size;            /* h_base                   (default 0.1)  */
    float r_max;                /* escape radius floor      (default 10)   */
    float r_disk_inner;         /* default 2.0  */
    float r_disk_outer;         /* default 15.0 */
    float disk_tilt_deg;        /* default 0    */
    int32_t anti_alias;         /* 0 = "disabled", 1 = "lod_radius"        */
    float aa_strength;          /* default 1.0  */
    float disk_rotation_speed;  /* t_offset = frame * this (render.py:3897) */
    int32_t device;             /* HIP device ordinal */
    int32_t math_mode;          /* BHR_MATH_FAST (0), BHR_MATH_STRICT (1) or BHR_MATH_HYBRID (2) */
} bhr_config;

/* math_mode: FAST uses v_rsq/v_rcp/v_sqrt and FMA contraction inside the RK4 loop (the analogue
 * of Taichi's fast_math=True default).  STRICT evaluates render.py:2854-3006 operation by operation
 * with IEEE sqrt/divide: ray paths, step counts and hit points are bit-identical to a strict f32
 * evaluation of the reference, at roughly twice the march time. */
#define BHR_MATH_FAST 0
#define BHR_MATH_STRICT 1
/* HYBRID: the strict arithmetic where the geodesic is unstable, the fast arithmetic elsewhere.  The only rays that
 * amplify rounding are those whose impact parameter b = |pos x dir| lies near the critical b_c = (3 sqrt 3 / 2) r_s of
 * the photon sphere (they wind around it; the deflection grows like -ln|b / b_c - 1|).  8x8-pixel tiles whose rays
 * have b within a band around b_c are marched by the STRICT kernel -- bit-identical paths, as math_mode 1 -- and all
 * other tiles by the FAST kernel, as two launches over complementary tile lists.  Pixels stay within the 1e-4 bar of
 * the reference's statements on every fixture; ray-step totals within 2e-4.  Schedules / disk sources
 * without a tile-list form (BHR_PERSISTENT, Disk V2) run STRICT.  With anti_alias = 1 the mip level is a
 * truncated function of the ray differentials, which rounding noise flips on level boundaries: the fast tiles' kernel
 * then carries guards -- a lane within a guard band of a level boundary (or of another switch of the algorithm: a disk
 * crossing in the terminating step, a step that ends on the disk plane, the disk's edges) hands its pixel to a third
 * launch that marches it with the strict arithmetic.  The guards are also on for tilted disks (the plane function of a
 * step that ends on a tilted plane rounds to exactly 0 for ~1e-6 of the crossings, which the reference's sign test never
 * registers); with tilt 0 and no anti-aliasing they are off (BHR_HYBRID_REPAIR=1 / 0 in the environment forces them). */
#define BHR_MATH_HYBRID 2

/* Camera uniforms exactly as TaichiRenderer.render() uploads them
 * (render.py:3880-3892): build_camera() in f64 on the host, cast to f32. */
typedef struct {
    float pos[3], right[3], up[3], forward[3];
    float pixel_width, pixel_height;
    float r_escape;             /* max(r_max, 2*|cam_pos|)  (render.py:3884) */
    float t_offset;             /* frame * disk_rotation_speed */
} bhr_camera;

/* bhr_render flags */
#define BHR_SKIP_DIFFERENTIALS 1u  /* render(skip_differentials=True): plain bilinear disk lookup */
#define BHR_SKIP_BLOOM         2u  /* render(skip_bloom=True) */
#define BHR_PERSISTENT         4u  /* persistent waves + queue refill instead of the tile schedule */
#define BHR_FORCE_FAST         8u  /* this call only: fast arithmetic regardless of bhr_config.math_mode */
#define BHR_FORCE_STRICT      16u  /* this call only: strict arithmetic regardless of bhr_config.math_mode */
#define BHR_ROW_COSTS         64u  /* also accumulate ray-steps per 8-row band (bhr_get_row_costs): the cost profile row blocks are balanced with */
#define BHR_LENS_FLARE        32u  /* add the lens flare to the final layer on the device (render.py:3920-4028) */
#define BHR_FORCE_HYBRID     256u  /* this call only: hybrid arithmetic regardless of bhr_config.math_mode */
#define BHR_GATHER_U8        512u  /* bhr_group_render: gather the QUANTISED rows ((H, W, 3) u8, save_image's truncation, render.py:423)
                                      on ctxs[0]'s device -- a quarter of the f32 bytes over xGMI; the pipelined schedule
                                      ships every row chunk as soon as its V pass has written it */
#define BHR_GROUP_SERIAL    1024u  /* bhr_group_render: the serial schedule (march -> H -> halo -> V -> gather, each behind the other
                                      on the tile's stream); same bytes as the pipelined one */
#define BHR_GROUP_PIPELINED 2048u  /* bhr_group_render: the pipelined schedule (halo pull under the V pass of the middle rows, row
                                      chunks pushed while the next chunk's V kernel runs).  Neither flag: pipelined where the
                                      tiles sit on distinct devices, serial where they share one */
#define BHR_GROUP_ASYNC     8192u  /* bhr_group_render: return once the frame is SUBMITTED (frames whose rows are stored by the kernels
                                      themselves: a GATHER flag, split-f16 post-pass, no lens flare, no host output; any other frame
                                      synchronises as before).  The next frame may be submitted at once: a tile's H pass waits, on
                                      the device, for its neighbours' previous V passes before it stores into their halo rows.
                                      bhr_group_sync / bhr_read_gathered* / any synchronous call waits for the frames in flight;
                                      per-tile counters describe the LAST frame submitted */
#define BHR_GROUP_TIME_MARCH 4096u /* bhr_group_render / bhr_tile_render: also record every tile's march-end event (bhr_counters.march_ms /
                                      bloom_ms of the tiles; frame_ms is always available).  Off by default: the record is a ~5 us bubble
                                      between the march and the H pass of every tile */
#define BHR_GATHER_PEER      128u  /* bhr_group_render: gather the tiles into one (H, W, 3) buffer on ctxs[0]'s device with
                                      hipMemcpyPeerAsync (xGMI), one copy per tile on the tile's own stream */

/* selectors for bhr_read_layer */
typedef enum {
    BHR_LAYER_FINAL = 0,  /* clip(bg + disk + blur, 0, 1)           render.py:3918 */
    BHR_LAYER_BG = 1,     /* image_field  = skybox * (1 - alpha)    render.py:3017 */
    BHR_LAYER_DISK = 2,   /* disk_layer_field = clamp(accum, 0, 1)  render.py:3018 */
    BHR_LAYER_BLUR = 3,   /* blur_field after the V pass            render.py:3108 */
    BHR_LAYER_HDR = 4     /* the scene-linear plane h of a graded frame (bhr_set_grade, keep_hdr); read only */
} bhr_layer;

typedef struct {
    uint64_t ray_steps;      /* executed while-loop iterations of the last march (render.py:2854) */
    uint64_t rays;           /* pixels marched by the last bhr_render */
    float march_ms;          /* HIP-event time of the march kernel, on the ctx stream */
    float bloom_ms;          /* H pass + V pass + combine */
    float frame_ms;          /* first launch .. last launch of bhr_render */
    float background_ms;     /* last bhr_generate_background */
    float compose_ms;        /* last bhr_compose_texture (compose + mip chain) */
    int32_t march_vgprs;     /* registers per lane of the march kernel that ran (hipFuncGetAttributes) */
    int32_t march_lds_bytes;
    /* sums over the bhr_render calls since bhr_timing_reset (at most the last
     * BHR_TIMING_RING - 2 calls), each launch bracketed by its own HIP events on its frame slot's stream */
    int32_t frames_timed;
    float march_ms_sum;
    float bloom_ms_sum;
    uint64_t ray_steps_sum;  /* ray_steps of one frame x frames_timed is NOT assumed: summed per frame */
    /* With two frames in flight the march launches of successive frames overlap, so march_ms_sum counts shared time
     * twice.  march_busy_ms = length of the UNION of the timed frames' [march start, march end] intervals: the time
     * during which at least one march kernel of this context was running; span_ms = first march start .. last frame end. */
    float march_busy_ms;
    float span_ms;
} bhr_counters;

#define BHR_TIMING_RING 512

BHR_API const char *bhr_last_error(void);
BHR_API int32_t bhr_abi_version(void);
BHR_API int32_t bhr_device_count(void);

/* ---- lifetime: TaichiRenderer.__init__ / garbage collection -------------- */
BHR_API int32_t bhr_create(const bhr_config *cfg, bhr_ctx **out);
BHR_API void bhr_destroy(bhr_ctx *ctx);
BHR_API int32_t bhr_sync(bhr_ctx *ctx);

/* ---- scene data ----------------------------------------------------------- */
/* texture_field.from_numpy(skybox): (tex_h, tex_w, 3) f32   render.py:2232-2233 */
BHR_API int32_t bhr_set_skybox(bhr_ctx *ctx, const float *rgb, int32_t tex_h, int32_t tex_w);
/* The Milky-Way glow of generate_skybox (render.py:296-341) added to the uploaded sky on the device, followed by
 * its clip(0, 1): upload the sky WITHOUT the glow (nebula + stars, the order-sensitive host part), call this once.
 * bhr_get_skybox reads the texture back ((tex_h, tex_w, 3) f32).  Asynchronous / synchronous. */
BHR_API int32_t bhr_skybox_add_glow(bhr_ctx *ctx);
/* generate_skybox's nebula and star splats (render.py:167-295) on the device, into the (tex_h, tex_w, 3) skybox a
 * previous bhr_set_skybox allocated.  The host supplies what comes out of NumPy's random stream: the 1/16-resolution
 * nebula noise as u8 (coarse_h, coarse_w, 3) with Pillow's fixed-point BILINEAR coefficients for both passes (kh:
 * (tex_w, ksize_h) 22-bit weights, bounds_h: (tex_w, 2) first source column and tap count; kv / bounds_v likewise for
 * rows), and per star its centre (cx, cy: f32 texel coordinates), colour (n, 3) and blob values (n, (2 patch_r + 1)^2).
 * The device reproduces Pillow's resize, `sky = 0.003 + resized / 255.0 * 0.04` and np.add.at's accumulation order bit
 * for bit.  Follow with bhr_skybox_add_glow.  Synchronises. */
BHR_API int32_t bhr_skybox_build(bhr_ctx *ctx, int32_t tex_h, int32_t tex_w, const uint8_t *coarse_rgb, int32_t coarse_h,
                                 int32_t coarse_w, const int32_t *kh, const int32_t *bounds_h, int32_t ksize_h,
                                 const int32_t *kv, const int32_t *bounds_v, int32_t ksize_v, int32_t n_stars,
                                 const float *cx, const float *cy, const float *colors, const float *vals, int32_t patch_r);
BHR_API int32_t bhr_get_skybox(bhr_ctx *ctx, float *out);
/* disk_texture_field.from_numpy + generate_disk_mipmaps(levels=4) + padded
 * upload (render.py:2235-2251, update_disk_texture 2292-2312).  (n_r, n_phi, 4)
 * f32.  The first call fixes (n_r, n_phi); later calls must match
 * (reference: AssertionError at render.py:2299 -> BHR_ERR_INVALID).  The mip
 * chain is built on the device and stored packed (1.33x, not 5x). */
BHR_API int32_t bhr_set_disk_texture(bhr_ctx *ctx, const float *rgba, int32_t n_r, int32_t n_phi);
/* disk_texture_field.to_numpy() */
BHR_API int32_t bhr_get_disk_texture(bhr_ctx *ctx, float *rgba_out);
/* disk_mips_field.to_numpy(): level `level` only, (n_r>>level, n_phi>>level, 4) */
BHR_API int32_t bhr_get_disk_mip(bhr_ctx *ctx, int32_t level, float *rgba_out);
BHR_API int32_t bhr_num_mip_levels(bhr_ctx *ctx);

/* ---- procedural disk-texture pipeline ------------------------------------- */
/* init_background_layer (render.py:3491-3547): allocates comp (13,n_r,n_phi),
 * uploads edge[n_r], omega_rows[n_r], initial stats; az_freq/az_shear are the
 * two RNG draws the host makes. */
BHR_API int32_t bhr_bg_init(bhr_ctx *ctx, int32_t n_r, int32_t n_phi, int32_t az_freq, float az_shear,
                    const float *edge, const float *omega_rows);
/* generate_background(t) -> _generate_background_kernel  (render.py:3549-3562, 3332-3451) */
BHR_API int32_t bhr_generate_background(bhr_ctx *ctx, float t);
/* accumulate_entity_layer's upload half: staging (6,n_r,n_phi) -> comp[5..10]
 * (render.py:3651-3653, 3455-3471) */
BHR_API int32_t bhr_set_entity_staging(bhr_ctx *ctx, const float *staging);
/* upload_parametric_state's comp upload: all 13 planes (render.py:2336-2353) */
BHR_API int32_t bhr_set_comp(bhr_ctx *ctx, const float *comp13);
/* _comp_field.to_numpy() (render.py:3666) */
BHR_API int32_t bhr_read_comp(bhr_ctx *ctx, float *comp13_out);
/* _zero_comp_slice / _fill_comp_slice (render.py:3475-3487) */
BHR_API int32_t bhr_fill_comp_slice(bhr_ctx *ctx, int32_t idx, float value);
/* _param_stats_field / _param_row_stats_field uploads (render.py:3708-3712):
 * stats = {density_p98, struct_scale}; row_stats (n_r, 2) = {max, p70} */
BHR_API int32_t bhr_set_compose_stats(bhr_ctx *ctx, float density_p98, float struct_scale, const float *row_stats);
/* _compose_disk_texture_kernel + mip chain (render.py:3755-3767, 3805-3817) */
BHR_API int32_t bhr_compose_texture(bhr_ctx *ctx, float t_offset, int32_t enable_rt, float color_temp);
/* eval_noise (render.py:3769-3790): coords (n,3); mode 0 simplex, 1 fbm */
BHR_API int32_t bhr_eval_noise(bhr_ctx *ctx, const float *coords, int64_t n, int32_t mode, int32_t octaves,
                       float persistence, float lacunarity, float *out);

/* ---- the hot path: TaichiRenderer.render() (render.py:3865-3923) ----------
 * Launches the fused ray-march kernel for rows [row0,row1), then (unless
 * BHR_SKIP_BLOOM) the bloom H pass, V pass and final combine.  Asynchronous; results stay
 * in HBM until read.  Successive calls alternate between the context's two frame slots (own stream and frame
 * buffers, shared read-only scene), so frame n + 1 overlaps the tail and the post-passes of frame n; every other
 * entry point is ordered (on the device) behind the frames in flight: reads return the last frame rendered, scene
 * updates never race a march.  BHR_FRAME_SLOTS=1 in the environment of bhr_create: one frame at a time.  (Every BHR_*
 * environment switch of the library is read once, by bhr_create.) */
BHR_API int32_t bhr_render(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags);
/* Motion blur: one frame as the mean of n marches over a shutter.  cams[0 .. n - 1] (1 <= n <= 64) are the samples' cameras,
 * each with its own position, basis and t_offset (the samplers roll the disk by phi + t_offset * Omega(r), so the Keplerian
 * roll within the exposure is the camera's t_offset).  For each layer L in {BG, DISK}:
 *   L_j  is, bit for bit, what bhr_render(ctx, &cams[j], flags | BHR_SKIP_BLOOM) stores for that layer -- under the context's
 *        arithmetic, disk source, anti-aliasing, supersampling or adaptive supersampling, hybrid lists and guards;
 *   acc  = L_0, then acc = acc + L_j for j = 1 .. n - 1 in that order, one f32 addition per channel;
 *   L    = acc * (1.0f / (float)n): the reciprocal rounded to f32 once, the product once, no FMA contraction anywhere.
 * For n = 1 this is L_0 itself.  BLUR and FINAL are what bhr_bloom computes from the resolved BG and DISK under the frame's
 * arithmetic (BHR_SKIP_BLOOM in flags suppresses them); BHR_LENS_FLARE then adds what bhr_lens_flare adds.  The resolved
 * DISK stays in [0, 1], so the split-f16 post-pass applies whenever it would for a marched frame.  bhr_set_outputs,
 * bhr_read_final_u8 / _u16, the dither, the PNG and JPEG sinks and the y4m stream work on the frame as on any other.
 * The n marches, the accumulation (csrc/shutter.hip) and the post-pass are ONE frame of ONE frame slot, all on that slot's
 * stream: the next bhr_render or bhr_render_shutter takes the other slot, as after a bhr_render.  bhr_counters: rays and
 * ray_steps are the sums over the n marches (under adaptive supersampling rays counts the refinement of the last sample
 * only); the frame has one entry in the timing ring, its march bracket from the first sample's start to behind the last
 * accumulation.  Asynchronous.
 * BHR_ERR_INVALID, with nothing launched and the context as it was: ctx or cams NULL, n < 1 or n > 64, a row-block
 * context, BHR_PERSISTENT or BHR_ROW_COSTS in flags. */
BHR_API int32_t bhr_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags);
/* Ray map: march a view once, re-shade it for every frame, read the geometry passes.  A ray's path depends on the camera
 * and the geometry of bhr_config only (step size, escape radius, disk radii, tilt, differentials or not) -- not on the skybox,
 * the disk texture or t_offset.  bhr_raymap_build marches the whole-frame view `cam` once with the STRICT arithmetic (whatever
 * the context's math_mode) and keeps, per pixel, what the march finds before it shades anything:
 *   STEPS      executed while-loop iterations (i32)
 *   STATUS     0 captured (r < r_s), 1 escaped: the pixel samples the sky (beyond r_escape or past the affine limit), 2 ran out
 *              of iterations (i32)
 *   ESCAPE_DIR the normalized direction handed to the skybox lookup, zeros unless STATUS is 1 (f32 x 3)
 *   CROSSINGS  annulus crossings of the ray, counting past the slots (i32)
 *   HITS       the first K crossings front to back, exactly as the march parks them: hit_x, hit_y, to_cam[3] and, with
 *              differentials, dxx, dxy, dyx, dyy (f32 x 5 or 9); records beyond min(CROSSINGS, K) are zero
 * K = option "raymap_slots" at the time of the build (1..8, default 4).  A pixel with more than K crossings is also put on an
 * overflow list.  flags: BHR_SKIP_DIFFERENTIALS or 0.  Synchronises; ordered behind the frames in flight.  Device memory: 24
 * bytes per pixel plus K x 20 (K x 36 with differentials) plus 4 for the overflow list; allocated at the first build, reused by
 * later builds of the same K and record size, released by bhr_raymap_free or bhr_destroy.
 * bhr_raymap_render(ctx, t, flags) is a frame: bit for bit the frame bhr_render(ctx, &cam_t, flags | BHR_FORCE_STRICT |
 * <the build's BHR_SKIP_DIFFERENTIALS>) leaves, cam_t the build camera with t_offset = t, under the scene as it is at the time
 * of the call -- BG, DISK, BLUR, FINAL and everything made from them on demand (u8 and u16 rows, dither, grade, HDR plane, lens
 * flare, PNG and JPEG sinks, the y4m stream).  One kernel shades the stored records with the march's own device functions
 * (csrc/march_raymap.hip); the strict fix kernel re-marches the pixels of the overflow list in the same frame.  flags:
 * BHR_SKIP_BLOOM, BHR_LENS_FLARE.  The frame takes the next frame slot like any other and has one entry in the timing ring, its
 * march bracket the shade and overflow launches; bhr_counters: rays = W H, ray_steps the steps of the overflow re-march only
 * (bhr_raymap_info.ray_steps has the build's, equal to a strict bhr_render's).  It neither counts towards nor runs the
 * calibration of slot 1's stream.  Asynchronous.  The map is read-only shared state like the scene: scene updates
 * (bhr_set_skybox, bhr_set_disk_texture, bhr_compose_texture, the lifecycle calls) do not invalidate it.
 * bhr_raymap_read copies one plane to the host, (rows, W[, 3]) and HITS as (K, rows, W, 5 | 9); bytes must be the plane's size.
 * bhr_raymap_get_info never fails for want of a map: built = 0 then.  bhr_raymap_free is ordered behind the frames in flight.
 * Supersampled maps.  Option "raymap_supersample" (1, 2, 4 or 8; default 1) is the map's OWN factor k, read by
 * bhr_raymap_build as "raymap_slots" is; the map in memory keeps the factor it was built with, and a build with another one
 * reallocates.  The context's bhr_set_supersample / bhr_set_adaptive_supersample stay at 1 for every map call and are refused
 * as below.  With k > 1 the map is the map of the fine frame: built by the strict march of bhr_set_supersample's fine camera
 * (pixel pitch / k) of `cam`, every plane k rows x k W, the overflow list in fine pixel indices -- a k x k group with any ray
 * over K is listed whole.  bhr_raymap_info: width and rows stay the output frame's, supersample = k, crossings_stored,
 * overflow_pixels (a multiple of k^2) and ray_steps count fine rays, ray_steps equal to that of a strict bhr_render of the
 * view with bhr_set_supersample(k).  bhr_raymap_read hands out the fine planes, (k rows, k W[, 3]) and (K, k rows, k W, 5 | 9).
 * Device memory: k^2 x (24 + K x 20 | 36 + 4) bytes per output pixel.
 * The frame: BG and DISK of bhr_raymap_render(ctx, t, flags) are bit for bit those of bhr_render(ctx', &cam_t, flags |
 * BHR_FORCE_STRICT | <the build's BHR_SKIP_DIFFERENTIALS>), ctx' a context of the same configuration with
 * bhr_set_supersample(ctx', k), and so is everything made from them.  The shade kernel shades each fine record list and resolves
 * the k x k groups in the wave with bhr_set_supersample's filter (pairwise tree, times 1 / k^2); the groups of the overflow
 * list are marched and resolved by the strict supersampled fix kernel.  bhr_counters: rays = k^2 W H.
 * bhr_raymap_render_view and bhr_raymap_render_shutter take such a map with their checks and meanings unchanged (the camera is
 * compared with the build camera as passed, at the output pitch): their frames are that k x k filter of the fine frames they
 * are defined by below; a shutter frame resolves each sample first, then takes the mean, always sample by sample.
 * Refusals, with nothing launched and the context as it was --
 *   BHR_ERR_STATE:   render or read before a build (or after bhr_raymap_free); render while supersampling, adaptive
 *                    supersampling or a Disk V2 source is on (the map stays; switch back and it renders again);
 *   BHR_ERR_INVALID: build or render on a row-block context; build with supersampling or adaptive supersampling on or with a
 *                    Disk V2 source (surface or volume); any other flag bit; a non-finite t_offset; "raymap_slots" outside 1..8
 *                    (refused by bhr_set_option; a BHR_RAYMAP_SLOTS outside it by the build); "raymap_supersample" not 1, 2, 4
 *                    or 8 (likewise; BHR_RAYMAP_SUPERSAMPLE by the build), or a build with k^2 W H >= 2^31; an unknown plane or
 *                    a wrong size;
 *   BHR_ERR_NOMEM:   a failed allocation: everything the call allocated is freed again and the context stays usable.
 *
 * bhr_raymap_render_view(ctx, cam, flags): a frame from the map seen from `cam`, the build camera turned rigidly about the z
 * axis (the cameras of an orbit: camera.orbit_position), with t_offset = cam->t_offset.  It needs a disk that is not tilted
 * (bhr_config.disk_tilt_deg == 0): the turn is then a symmetry of everything a ray's path depends on -- the hole, the disk
 * plane, the two disk radii, the escape sphere -- and in exact arithmetic the ray of pixel (i, j) of `cam` is the ray of pixel
 * (i, j) of the build camera turned by the same angle.  The shade kernel turns the xy parts of the stored hit points, to_cam
 * vectors, hit differentials and escape directions by that angle (its cosine and sine computed in binary64 and rounded once)
 * and shades them as bhr_raymap_render does; the pixels of the overflow list are marched from `cam` by the strict fix kernel
 * and are the strict frame's bit for bit.  Such a frame is the strict march of the build view's rays, not bit-identical to
 * bhr_render of `cam`: it is as far from it as two strict marches of symmetric views are from each other (the f32 rounding of
 * the march; per-channel RMSE of a few 1e-5 for a camera 6 r_s out, single chaotic pixels near the photon ring up to some 1e-2
 * for a camera 2.6 r_s out).  With `cam` the build camera itself (angle 0) the frame is bhr_raymap_render's bit for bit.  In
 * every other respect it is a frame like bhr_raymap_render's: frame slot, timing-ring entry, counters, post-pass, sinks, grade,
 * dither and lens flare; flags BHR_SKIP_BLOOM, BHR_LENS_FLARE.  Asynchronous.
 * Checked in binary64 before anything is launched: pos[2], pixel_width, pixel_height and r_escape equal the build camera's; the
 * distance of pos from the z axis is at least 1e-6 (on the axis the camera basis does not turn with the position) and equals
 * the build's within 1e-5 relative; right, up and forward each equal the build's turned by the angle between the two positions
 * in the xy plane, within 1e-5 absolute.
 * Refusals, with nothing launched and the context as it was --
 *   BHR_ERR_INVALID: ctx or cam NULL; a tilted disk; a camera that is no such turn of the build's; any other flag bit; a
 *                    non-finite t_offset; a row-block context;
 *   BHR_ERR_STATE:   everything bhr_raymap_render refuses with it.
 *
 * bhr_raymap_render_shutter(ctx, cams, n, flags): motion blur from the map -- one frame as the mean of n frames from the map,
 * with no march at all.  cams[0 .. n - 1] (1 <= n <= 64) are the samples' cameras, each with its own t_offset.  What differs
 * between the samples of one exposure is what the map leaves free: the disk's roll (t_offset, an argument of the samplers)
 * and the orbit camera's turn about z (the turn bhr_raymap_render_view applies to the stored records).  A sample is accepted
 *   - if its pose equals the build camera's field for field (everything but t_offset), on any disk, tilted or not: the still
 *     camera, whose turn is (1, 0);
 *   - else if it passes exactly the checks of bhr_raymap_render_view: the disk is not tilted and the camera is a turn of the
 *     build camera about z within the tolerances above, checked in binary64; its cosine and sine are computed as there.
 * For each layer L in {BG, DISK}:
 *   L_j  is, bit for bit, what bhr_raymap_render_view(ctx, &cams[j], BHR_SKIP_BLOOM) stores for that layer for a turned
 *        camera, and what bhr_raymap_render(ctx, cams[j].t_offset, BHR_SKIP_BLOOM) stores for a camera with the build pose;
 *   acc  = L_0, then acc = acc + L_j for j = 1 .. n - 1 in that order, one f32 addition per channel;
 *   L    = acc * (1.0f / (float)n): the reciprocal rounded to f32 once, the product once, no FMA contraction anywhere
 * -- bhr_render_shutter's mean, word for word (tests/shutter_ref.py restates it).  For n = 1 this is L_0 itself.  BG and DISK
 * are the STRICT arithmetic's whatever the context's math_mode.  BLUR and FINAL are what bhr_bloom computes from the resolved
 * BG and DISK in this context -- its kernels follow the context's arithmetic as bhr_bloom's do: the exact f32 post-pass in a
 * strict context (the frame is then the strict frame throughout), the split-f16 one in a fast or hybrid context (BHR_SKIP_BLOOM
 * in flags suppresses them); BHR_LENS_FLARE then adds what bhr_lens_flare adds.  u8 / u16 rows, dither, grade, HDR plane, the
 * sinks and the y4m stream work on the frame as on any other.
 * Two routes give these bits.  A map without overflow pixels takes ONE launch (csrc/march_raymap.hip:
 * raymap_shade_shutter_kernel) that shades a pixel's records under all n (t_offset, cos, sin, camera position) and keeps the
 * running sums on the chip: no layer goes through memory between the samples.  A map with overflow pixels -- or any map
 * while option "raymap_shutter_fused" is 0 -- runs, per sample, the shade launch and the strict fix launch over the overflow
 * list as bhr_raymap_render[_view] issues them, then bhr_render_shutter's accumulation launch (csrc/shutter.hip).
 * The frame takes the next frame slot like bhr_raymap_render and runs on that slot's stream; one timing-ring entry, its march
 * bracket from the first shade launch to behind the last launch that writes BG / DISK; it neither counts towards nor runs the
 * calibration of slot 1's stream.  bhr_counters: rays = n W H, ray_steps the sum of the overflow re-marches' steps (0 for a
 * map without overflow pixels).  Asynchronous.
 * Refusals, with nothing launched and the context as it was --
 *   BHR_ERR_INVALID: ctx or cams NULL; n < 1 or n > 64; a flag bit other than BHR_SKIP_BLOOM / BHR_LENS_FLARE; a non-finite
 *                    t_offset in any sample; a row-block context; a sample that is neither the build pose nor an admissible
 *                    turn (a turned camera over a tilted disk included) -- the message names the sample index;
 *   BHR_ERR_STATE:   everything bhr_raymap_render refuses with it. */
#define BHR_RAYMAP_STEPS 0
#define BHR_RAYMAP_STATUS 1
#define BHR_RAYMAP_ESCAPE_DIR 2
#define BHR_RAYMAP_CROSSINGS 3
#define BHR_RAYMAP_HITS 4
typedef struct {
    int32_t built, diff, slots;         /* a map exists; it holds the differential records; K */
    int32_t width, rows;                /* of the output frame, whatever the factor */
    int32_t supersample;                /* the map's own factor k (option "raymap_supersample"): the planes are k rows x k W */
    int64_t crossings_stored;           /* sum over the (fine) pixels of min(CROSSINGS, K) */
    int64_t overflow_pixels;            /* (fine) pixels on the overflow list: CROSSINGS > K; with k > 1 whole k x k groups */
    int64_t device_bytes;
    uint64_t ray_steps;                 /* of the build: those of a strict bhr_render of the view */
    bhr_camera cam;                     /* the view the map was built for */
} bhr_raymap_info;
BHR_API int32_t bhr_raymap_build(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags);
BHR_API int32_t bhr_raymap_render(bhr_ctx *ctx, float t_offset, uint32_t flags);
BHR_API int32_t bhr_raymap_render_view(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags);
BHR_API int32_t bhr_raymap_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags);
BHR_API int32_t bhr_raymap_read(bhr_ctx *ctx, int32_t plane, void *out, int64_t bytes);
BHR_API int32_t bhr_raymap_get_info(bhr_ctx *ctx, bhr_raymap_info *out);
BHR_API int32_t bhr_raymap_free(bhr_ctx *ctx);
/* ---- point stars: a star catalogue rendered through the ray map (csrc/stars.hip, csrc/api_stars.hip; DESIGN 4 "Point stars") ----
 * The sky texture conserves surface brightness: near the hole a baked star is smeared into a dim arc.  A real star is
 * unresolved -- its images stay points and their flux is multiplied by the lensing magnification.  With a catalogue set, a frame
 * from the ray map adds those images to the sky.
 * A star is a unit direction u on the celestial sphere in the sky's own convention (theta = acos(u.z), phi = atan2(u.y, u.x), as
 * sample_skybox takes a direction) and an RGB flux Phi in units of sky value x steradian: a patch of sky of solid angle Omega
 * that contains the star has the mean radiance Phi / Omega.
 * Cells and triangles.  Cell (i, j), 0 <= i < W - 1, 0 <= j < rows - 1, has the pixel centres (i, j), (i+1, j), (i, j+1),
 * (i+1, j+1) as corners P00, P10, P01, P11 and is cut into T0 = (P00, P10, P01) and T1 = (P11, P01, P10).  For a triangle with
 * corner pixels a, b, c: e_a, e_b, e_c are the map's stored escape directions (for a turned view turned about z exactly as the
 * shade kernel turns them), n_a, n_b, n_c the normalized camera-side pixel directions.  A triangle is USED when all three rays
 * escaped (status 1) and min(e_a.e_b, e_b.e_c, e_c.e_a) >= cos(max_span); otherwise it contributes nothing (the huge sky patches
 * of high-order images and of cells that straddle the shadow or a fold, whose magnification is of the order
 * (pixel angle / span)^2).
 * Solid angles (Van Oosterom and Strackee, the triple product on differences so that it does not cancel):
 *   Omega(a, b, c) = 2 atan2(|a . ((b - a) x (c - a))|, 1 + a.b + b.c + c.a),  Omega_sky = Omega(e_a, e_b, e_c),
 *   Omega_cam = Omega(n_a, n_b, n_c).
 * Inside test and weights: with s_c = u . (e_a x e_b), s_a = u . (e_b x e_c), s_b = u . (e_c x e_a) (evaluated as
 * u . ((e_a - u) x (e_b - u)) and so on, the same determinants without the cancellation) the star is inside when all three are
 * >= 0, or all three are <= 0 (a parity-flipped image: real, and kept), and u . (e_a + e_b + e_c) > 0.  The barycentric weights
 * are w_x = s_x / (s_a + s_b + s_c); a zero sum contributes nothing.  The image lies at the weighted mean of the three corner
 * positions, so inside the cell.
 * Deposit: D = Phi / (2 Omega_cam) * min(Omega_cam / Omega_sky, max_magnification) -- the triangle's mean radiance over half a
 * pixel's area, capped on the critical curve -- spread over the cell's four corner pixels with the bilinear (tent) weights of
 * the image position.  A pixel receives star light from its four adjacent cells only; without a hole Omega_sky = Omega_cam and
 * every star in the frame deposits Phi / (2 Omega_cam) in total.
 * The star plane S, (rows, W, 3) f32, is the sum of all deposits: per cell and corner one running f32 sum, T0's stars then T1's,
 * each in the catalogue's binned order; a pixel adds its four cells in the order (j-1, i-1), (j-1, i), (j, i-1), (j, i).  No
 * floating-point atomics: two gathers of the same map and catalogue give the same bits.
 * The frame: BG = fl((sky_sample + S) * (1 - alpha_total)) per channel -- the plane is added to the sky sample ahead of the
 * march's own product; DISK is untouched.  BG may exceed 1; FINAL clips as ever, the HDR plane and the grade carry the rest.  A
 * pixel on the map's overflow list is stored by the strict fix kernel as without a catalogue and receives NO star light.
 * bhr_set_stars copies the catalogue (directions normalized in binary64 and rounded once), sorts it into an equirectangular grid
 * of bins and uploads it; n = 0 removes it; p = NULL means max_magnification 32 and max_span_deg 10.  It synchronises.
 *   BHR_ERR_INVALID, the context unchanged: ctx NULL (or stars NULL with n > 0); n < 0 or n > 2^22; a direction that is
 *     non-finite or whose norm is not within 1e-3 of 1; a negative or non-finite flux; max_magnification outside [1, 1e6];
 *     max_span_deg outside (0, 60]; a row-block context.
 *   BHR_ERR_NOMEM: with everything freed -- the context then has no catalogue.
 * With a catalogue set, bhr_raymap_render and bhr_raymap_render_view launch the gather kernel and the shade kernel that adds the
 * plane.  The plane of the un-turned build view is computed once per (map, catalogue) and reused; the plane of a turned view is
 * computed per frame into storage of the frame slot.  A view at angle 0 uses the cached plane and is bhr_raymap_render's frame
 * bit for bit.  Refused with BHR_ERR_STATE naming the stars, nothing launched, map and catalogue kept:
 * bhr_raymap_render_shutter, and any render from (or plane read of) a map with supersample > 1.  Without a catalogue every call is exactly what it
 * is without this section.  bhr_render, bhr_render_shutter, bhr_render_observer, the Kerr march and the Kerr ray map IGNORE the
 * catalogue (the Kerr map has one of its own: bhr_set_kerr_stars, below).
 * bhr_raymap_read(ctx, BHR_RAYMAP_STARS, out, rows * W * 12) returns the build view's plane, computing it if needed;
 * BHR_ERR_STATE without a map or without a catalogue.
 * bhr_get_stars_info: the catalogue (n = 0: none) and the counts of the last gather launched -- images: deposits (star, used
 * triangle); capped: used triangles whose magnification exceeded the cap; skipped_span: triangles of three escaped rays dropped
 * by the span rule.  bhr_stars_resources: VGPRs, LDS bytes and scratch bytes of the gather kernel (rot: the turned one). */
#define BHR_RAYMAP_STARS 5
typedef struct { float dir[3]; float flux[3]; } bhr_star;
typedef struct { float max_magnification; float max_span_deg; } bhr_star_params;
typedef struct {
    int32_t n;                          /* stars in the catalogue; 0: none */
    int32_t bins_theta, bins_phi;       /* the grid of bins */
    int32_t reserved;
    bhr_star_params params;
    int64_t device_bytes;
    int64_t images, capped, skipped_span;   /* of the last gather */
} bhr_stars_info;
BHR_API int32_t bhr_set_stars(bhr_ctx *ctx, const bhr_star *stars, int32_t n, const bhr_star_params *p);
BHR_API int32_t bhr_get_stars_info(bhr_ctx *ctx, bhr_stars_info *out);
BHR_API int32_t bhr_stars_resources(int32_t rot, int32_t out[3]);
/* ---- polarisation: Stokes I, Q, U of the disk through the ray map (csrc/march_polar.hip, csrc/api_polar.hip; DESIGN 4 "Polarisation") ----
 * With a polarisation set, a frame of bhr_raymap_render is followed on its own frame slot and stream by one more pass over the
 * map's records, which stores three f32 planes (rows, W) and a grid of cell means; the frame's layers and rows are what they are
 * without it.  Units r_s = 1, F(r) = 1 - 1 / r.  For a pixel: C the camera position, D the unit direction its ray is launched
 * along, (R, U, Fwd) the camera's basis; the photon arrives travelling along -D.  N = normalize(C x D) is the unit normal of the
 * ray's plane, which is parallel-transported along a Schwarzschild ray, so the angle psi between the polarisation vector and N,
 * measured about the photon direction, is the same at the gas and at the camera (Connors, Piran and Stark 1980).  A ray with
 * |C x D| < 1e-6 |C| is radial and adds nothing to Q and U.  Per stored crossing k, front to back:
 *   P = (hit_x, hit_y, hit_y tan_t), r_hat = P / |P|, r = max(|P|, 1 + 1e-3), w = to_cam;
 *   K = normalize(K0 - (K0 . N) N), K0 = (w . r_hat) / sqrt(F(r)) r_hat + (w - (w . r_hat) r_hat): the photon's direction in the
 *     static observer's orthonormal frame, in the ray's plane;
 *   the gas: v_hat = normalize(r_hat x n), n = (0, -sin_t, cos_t) the disk normal (the g-factor's v_hat, with its fallback),
 *     beta = min(r Omega / sqrt(F), 0.99), Omega = sqrt(0.5 / r^3), gamma = 1 / sqrt(1 - beta^2);
 *   in the gas frame: n' = [K + ((gamma - 1)(K . v_hat) - gamma beta) v_hat] / (gamma (1 - beta K . v_hat));
 *   the field: B' = normalize(b_r r_hat + b_phi v_hat + b_z n), e' = n' x B', s2 = |e'|^2, e_hat = e' / sqrt(s2) -- the electric
 *     vector of synchrotron light is perpendicular to the projected field; the polarised weight is p_k = fraction s2, which goes
 *     to 0 continuously where the photon runs along the field (s2 = 0 adds nothing);
 *   back in the static frame: f = e_hat + (gamma - 1)(e_hat . v_hat) v_hat - gamma beta (e_hat . v_hat) K, a unit vector
 *     perpendicular to K; cos psi = f . N, sin psi = f . (N x K);
 *   at the camera: f_c = cos psi N + sin psi (N x (-D)); the sky-plane axes are e_x = normalize(R - (R . D) D) and e_y = D x e_x
 *     with its sign flipped if e_y . U < 0; x = f_c . e_x, y = f_c . e_y, cos 2chi = (x^2 - y^2) / (x^2 + y^2),
 *     sin 2chi = 2 x y / (x^2 + y^2): chi is counted from image-right towards image-up;
 *   c_k = the Rec. 709 luma (0.2126, 0.7152, 0.0722) of what the crossing added to the disk accumulator (after minus before).
 * I = sum c_k, Q = sum p_k c_k cos 2chi_k, U = sum p_k c_k sin 2chi_k, each one f32 running sum in record order.  A crossing
 * outside [r_disk_inner, r_disk_outer] adds nothing; a pixel on the map's overflow list (more crossings than slots) has
 * I = Q = U = 0.  The cell grid: means of I, Q and U over cell x cell pixel cells, ceil(rows / cell) x ceil(W / cell) of them,
 * edge cells over the pixels they have; summed in a fixed order without floating-point atomics, so two runs give the same bits.
 * bhr_set_polarization: p NULL switches it off (the default).  It synchronises.  BHR_ERR_INVALID, the context unchanged: a field
 *   that is zero or not finite; fraction outside [0, 1]; cell other than 8, 16 or 32; reserved words other than 0; a row-block
 *   (group or tile) context; a spin set (bhr_set_spin); a Disk V2 source.
 * With a polarisation set, refused with BHR_ERR_STATE naming it and nothing launched: bhr_raymap_render_shutter,
 *   bhr_raymap_render_view, and bhr_raymap_render from a map with supersample > 1.
 * bhr_read_stokes: plane 0, 1, 2 = I, Q, U of the last frame of bhr_raymap_render, rows * W floats; bhr_read_stokes_cells: its
 *   cell grid, dims[0] x dims[1] x 3 floats (I, Q, U means; at most ceil(rows / 8) ceil(W / 8) 3) and the grid's rows and columns
 *   in dims; out NULL returns dims only.  BHR_ERR_STATE where no such frame has been rendered since the polarisation was set or
 *   the map was built.  Both synchronise.
 * bhr_stokes_resources: VGPRs, LDS bytes and scratch bytes of the Stokes kernel (diff: the one of a map with differentials). */
typedef struct {
    float b_r, b_phi, b_z;              /* the field in the gas frame: radial, along the orbit, along the disk normal */
    float fraction;                     /* Pi_0: the degree of polarisation of light emitted across the field, 0 .. 1 */
    int32_t cell;                       /* pixels per side of a cell of the grid: 8, 16 or 32 */
    int32_t reserved[3];                /* 0 */
} bhr_polarization;
BHR_API int32_t bhr_set_polarization(bhr_ctx *ctx, const bhr_polarization *p);
BHR_API int32_t bhr_read_stokes(bhr_ctx *ctx, int32_t plane, float *out);
BHR_API int32_t bhr_read_stokes_cells(bhr_ctx *ctx, float *out, int32_t dims[2]);
BHR_API int32_t bhr_stokes_resources(int32_t diff, int32_t out[3]);
/* ---- Kerr polarisation: the same planes for the frames of bhr_kerr_raymap_render (csrc/march_kerr_polar.hip; DESIGN 4 "Kerr polarisation") ----
 * The struct, the planes, the cell grid, c_k, I, Q, U, the convention for chi and both reads are those above.  What differs is how
 * a crossing's polarisation gets from the gas to the camera: by the Walker-Penrose constant, in the march's Kerr-Schild chart
 * (units r_s = 1, M = 1/2, a = A M; g = eta + f l l, l_mu = (1, l); csrc/ray_kerr.h).  For the traced photon, covariant momentum
 * (-1, p), contravariant k = (1 + f u, p - f u l), u = 1 + l . p, and a polarisation vector f parallel-transported along it,
 *   kappa1 = k^t (x . f) - f^t (x . k) + a (k^x f^y - k^y f^x),   kappa2 = x . (k x f) - a (k^t f^z - k^z f^t)
 * are conserved (bold spatial parts, Euclidean dot and cross).  Per stored crossing at (hx, hy, 0) with the photon's momentum p
 * there (kept per record by a build under the polarisation):
 *   r = sqrt(hx^2 + hy^2 - a^2), f = 1 / r, l = ((r hx + a hy) / Q, (r hy - a hx) / Q, 0), Q = hx^2 + hy^2;
 *   the gas's 4-velocity u of the context's redshift mode -- model: speed beta = min(r_s Omega / sqrt(1 - 1 / r_s), 0.99), r_s =
 *     max(r, 1 + 1e-3), Kerr's Omega, along the orbit as the static observer at the hit measures it; exact: the circular geodesic
 *     outside the ISCO, the plunge with the ISCO's E and L inside it (the g-factor's gas in either mode);
 *   the tetrad by Gram-Schmidt under g: u, e_phi from v_hat = r_hat x n (the sense of the disk), e_z = d_z, e_r from r_hat;
 *   n'_(i) = (k . e_(i)) / (-k . u), normalized (the interpolated p is null to second order in its step only); B' = normalize(b_r, b_phi, b_z) in (e_r, e_phi, e_z); e' = n' x B', s2 = |e'|^2,
 *     p_k = fraction s2; f_em = (e'_(i) / sqrt(s2)) e_(i); kappa_em = kappa(hit, k, f_em).
 * At the camera C with the photon Ray::init launches along the pixel direction D (momentum p_c): e_x, e_y the sky-plane axes
 * above, lifted to E_x = (p_c . e_x, e_x), E_y = (p_c . e_y, e_y); (alpha, beta) solves alpha kappa(E_x) + beta kappa(E_y) =
 * kappa_em; cos 2chi = (alpha^2 - beta^2) / (alpha^2 + beta^2), sin 2chi = 2 alpha beta / (alpha^2 + beta^2).  A pixel whose
 * 2 x 2 system is singular (the radial ray of a hole that does not spin) adds to I only.
 * bhr_set_kerr_polarization: the validation of bhr_set_polarization's struct; BHR_ERR_STATE without the Kerr march (bhr_set_spin);
 *   NULL switches it off; it synchronises.  A Kerr map built while it is set keeps the momenta (slots x 3 floats per pixel more);
 *   bhr_kerr_raymap_render from a map built without them, and bhr_kerr_raymap_render_view with a turned camera, are BHR_ERR_STATE
 *   while it is set.  A change of spin or redshift mode makes the planes unreadable until the next such frame.
 * bhr_kerr_stokes_resources: VGPRs, LDS bytes and scratch bytes of the Kerr Stokes kernel of a redshift mode. */
/* bhr_kerr_raymap_read(ctx, BHR_RAYMAP_MOMENTUM, out, slots * rows * W * 12): the momenta (p_x, p_y, p_z) of a map that keeps them,
 * (slots, rows, W, 3) in record order, zeros behind a pixel's crossings; BHR_ERR_STATE for a map built without them. */
#define BHR_RAYMAP_MOMENTUM 6
BHR_API int32_t bhr_set_kerr_polarization(bhr_ctx *ctx, const bhr_polarization *p);
BHR_API int32_t bhr_kerr_stokes_resources(int32_t redshift, int32_t out[3]);
/* image_field/disk_layer_field/blur_field .to_numpy() and the final image,
 * for the context's rows: (row1-row0, width, 3) f32.  Synchronises. */
BHR_API int32_t bhr_read_layer(bhr_ctx *ctx, int32_t layer, float *out);
/* field.from_numpy() for a frame layer: replaces the context's rows of FINAL, BG, DISK or BLUR with
 * caller data, e.g. to post-process a frame composed elsewhere.  Synchronises.  A DISK layer holds finite values >= 0
 * (a march writes clamp(accum, 0, 1)): one with a negative or non-finite value is refused with BHR_ERR_INVALID and the
 * layer keeps its contents -- the bloom folds the reference's `lum > 0` test away, which holds for non-negative layers
 * only. */
BHR_API int32_t bhr_write_layer(bhr_ctx *ctx, int32_t layer, const float *in);
/* self._bloom_kernel(disk_layer_field, bright_field, blur_field, 0, 0.4, int(0.02 W), (W / 640)^2) followed by
 * clip(img + disk + blur, 0, 1) (render.py:3914-3918), standalone on the layers currently in the context:
 * BLUR <- bloom(DISK), FINAL <- clip(BG + DISK + BLUR, 0, 1).  Whole-frame context (row blocks need their
 * neighbours' halo rows: bhr_group_render).  Asynchronous.  The kernels follow the context's arithmetic as for a
 * rendered frame (and the "bloom_split" option), except that a DISK layer written with a value above 3.99 -- more than
 * the split-f16 kernels' halves carry -- goes through the exact f32 kernels until a march or another write replaces
 * it: the result is the same function of the layers under every arithmetic. */
BHR_API int32_t bhr_bloom(bhr_ctx *ctx);
/* What bhr_render keeps in memory of a frame besides the bg / disk layers.  TaichiRenderer.render() returns the f32 frame
 * (BHR_OUTPUT_F32, the default); the video loop, the PNG sink and the u8 row-block gather only ever read the quantised
 * rows (BHR_OUTPUT_U8: save_image's truncation fused into the V pass's epilogue, 3 bytes per pixel instead of 12);
 * blur_field (BHR_OUTPUT_BLUR) is internal to the reference's render().  A layer that was not kept is produced on demand
 * by whichever call needs it (bhr_read_layer, bhr_read_final_u8, the sinks): the frame's V pass runs again for it, same
 * kernels, same bits.  mask: any non-empty combination. */
#define BHR_OUTPUT_F32 1u
#define BHR_OUTPUT_BLUR 2u
#define BHR_OUTPUT_U8 4u
BHR_API int32_t bhr_set_outputs(bhr_ctx *ctx, uint32_t mask);
/* Supersampling: k x k rays per pixel on an ordered grid, k = 1 (default: one ray per pixel), 2, 4 or 8.  The BG and DISK
 * layers of a W x H frame with factor k are the k x k box filter of those a k = 1 context renders of the same view at
 * kW x kH (same camera, skybox, disk source and math mode), bit for bit: the sample (sx, sy) of output pixel (i, j) is the
 * ray of fine pixel (k i + sx, k j + sy), with the value the single-sample march stores for it (bg (1 - A) rounded once,
 * clamp(accum, 0, 1)); per channel each sub-sample row is summed as a pairwise tree (adjacent pairs, then pairs of those
 * sums, ...), the k row sums by the same tree, and the sum multiplied once by 1 / k^2.  The march takes the context's
 * camera (pitch pw, ph) and marches the fine grid at pw / k, ph / k.  Everything after the march -- bloom, combine, lens
 * flare, u8 quantisation, PNG and video sinks -- runs at W x H on the resolved layers.  A hybrid frame with guards
 * re-marches a k x k group with the strict arithmetic as soon as one of its rays is flagged (bhr_hybrid_repairs counts
 * output pixels).  Counters: rays = k^2 W H, ray_steps those of the kW x kH march.  Ordered behind the frames in flight.
 * BHR_ERR_INVALID: k not in {1, 2, 4, 8}, a row-block context (k > 1), or k^2 W H >= 2^31.  With k > 1, bhr_render with
 * BHR_PERSISTENT or BHR_ROW_COSTS, bhr_group_render*, bhr_tile_export and bhr_tile_render return BHR_ERR_INVALID. */
BHR_API int32_t bhr_set_supersample(bhr_ctx *ctx, int32_t k);
/* Adaptive supersampling: one ray per pixel, and k x k rays only where the k = 1 frame's neighbours differ.  k = 2, 4 or 8
 * and a threshold T (f32); k = 1 turns supersampling off.  bhr_set_supersample keeps its meaning (every pixel) and turns
 * adaptivity off.  A frame of a W x H whole-frame context is then this function of (view, k, T):
 *  1. Base frame.  The context's ordinary k = 1 march (its arithmetic, hybrid lists, guards and fix list included) gives the
 *     layers BG1, DISK1.
 *  2. Contrast.  For pixel p = (i, j), over its edge neighbours n in {(i-1, j), (i+1, j), (i, j-1), (i, j+1)} inside the
 *     frame, both layers L in {BG1, DISK1} and the three channels: c(p) = max |L[p] - L[n]|, each difference one f32
 *     subtraction.  A 1 x 1 frame has c = 0.
 *  3. Refined set.  R = {p : c(p) > T}, an f32 comparison: T = +inf refines nothing, any T < 0 every pixel; NaN is refused.
 *  4. Refined pixels.  For p in R, BG and DISK are the values pixel p has in the frame bhr_set_supersample(k) renders of the
 *     same view (same fine grid at pitch pw / k, ph / k, same pairwise tree, same 1 / k^2), the k x k group marched with: the
 *     strict arithmetic under strict (and wherever hybrid resolves to strict: Disk V2 sources); the fast one under fast;
 *     under hybrid the strict one if the 8 x 8 tile of the FINE frame that holds the group (k divides 8: exactly one does) is
 *     a strict tile by the rule a bhr_set_supersample(k) hybrid frame classifies by (same band, padding and edge-on wedge),
 *     else the fast one -- WITHOUT guards: one ray on a switch weighs 1 / k^2.  Disk V2 sources: the base march's.
 *  5. Other pixels keep BG1, DISK1.  Everything the march stores besides the two layers (the split-f16 post-pass's inputs) is
 *     rewritten for refined pixels: bloom, combine, lens flare, quantisation, PNG and video sinks run unchanged.
 * The frame does not depend on the order in which the device listed R.  A contrast criterion cannot see what no k = 1 ray
 * hit: a star (or any feature) smaller than a pixel that falls between the k = 1 rays of a smooth neighbourhood is not
 * refined, whatever T >= 0.  Counters: rays = W H + k^2 |R|, ray_steps = base march + refinement; the march's time includes
 * detection and refinement.  Ordered behind the frames in flight.  BHR_ERR_INVALID: NaN threshold, k not in {1, 2, 4, 8}, a
 * row-block context (k > 1), k^2 W H >= 2^31.  While adaptive, bhr_render with BHR_PERSISTENT or BHR_ROW_COSTS,
 * bhr_group_render*, bhr_tile_export and bhr_tile_render return BHR_ERR_INVALID, as with bhr_set_supersample(k > 1). */
BHR_API int32_t bhr_set_adaptive_supersample(bhr_ctx *ctx, int32_t k, float threshold);
/* out = {refined pixels |R| of the last adaptive frame, those of them marched with the strict arithmetic, pixels of the
 * frame}.  Synchronises.  BHR_ERR_STATE before the first frame rendered under bhr_set_adaptive_supersample(k > 1). */
BHR_API int32_t bhr_adaptive_info(bhr_ctx *ctx, int64_t out[3]);
/* A spinning (Kerr) hole.  a_over_m = A = a / M, |A| <= 0.998; 0 (the default) is the Schwarzschild hole every other entry
 * point describes.  The spin axis is the normal of the untilted disk (+z); A > 0 turns with the disk's orbital motion
 * (v_hat = r_hat x n), A < 0 against it.  With A != 0 -- or with force_kerr != 0 at any A, which tests use to run the Kerr
 * kernel at spin 0 -- the frames of bhr_render are marched by the Kerr object (csrc/march_kerr.hip): RK4 on the six-component
 * state (x, p) of the Hamiltonian H = (p.p - 1) / 2 - f (1 + l.p)^2 / 2 in Kerr-Schild coordinates, the reference's step rule
 * on the Kerr-Schild radius, capture at r < r_plus = (1 + sqrt(1 - A^2)) / 2, the disk crossing gated on the Boyer-Lindquist
 * radius sqrt(hx^2 + hy^2 - a^2) and shaded with the reference's g-factor model with Kerr's orbital frequency
 * sqrt(M) / (r^1.5 + a sqrt(M)) (DESIGN.md "Kerr" states the model; tests/kerr_ref.py is its CPU reference).  bhr_config.math_mode
 * then no longer selects the march (there is one Kerr arithmetic); the post-pass follows it as before.  Plain supersampling
 * (bhr_set_supersample), lens flare, grading, every output path and sink work as for any frame.  A = 0 with force_kerr = 0
 * launches exactly the kernels a context that never called this launches.  Ordered behind the frames in flight.
 * BHR_ERR_INVALID, each with a message that names the combination: |A| > 0.998 or NaN; with a spin set (A != 0 or forced), by
 * this call or by the call that meets it -- a tilted disk, anti_alias = 1, a Disk V2 source, adaptive supersampling, a
 * row-block context (bhr_group_render*, bhr_tile_export, bhr_tile_render), bhr_render with BHR_PERSISTENT or BHR_ROW_COSTS,
 * bhr_render_shutter, bhr_raymap_build and the three bhr_raymap_render* calls.
 * The camera of a frame marched with a spin set stands outside the static limit: with w = pos.pos - a^2,
 * S = sqrt(w^2 + 4 a^2 z^2) and the Kerr-Schild radius r = sqrt((w + S) / 2) of bhr_camera.pos, f = r / S < 1 (in the plane that is
 * r > r_s = 1 at every spin; on the axis the limit meets the horizon), and r >= r_plus.  Inside it no static observer exists and
 * the photon along a pixel direction d, p = s d + f Lam l with s = 1 / sqrt(1 - f (1 - (l.d)^2)), is not real for every d.
 * bhr_render evaluates f in binary64 and returns BHR_ERR_INVALID naming the static limit before anything is launched; the
 * context is untouched and renders the next camera as ever. */
BHR_API int32_t bhr_set_spin(bhr_ctx *ctx, float a_over_m, int32_t force_kerr);
/* out = {VGPRs per lane, LDS bytes per block, scratch (private segment) bytes per lane} of the Kerr march kernel
 * (supersampled != 0: of its supersampled twin), from hipFuncGetAttributes.  After a frame marched with a spin set,
 * bhr_counters.march_vgprs / march_lds_bytes are that kernel's too. */
BHR_API int32_t bhr_kerr_resources(int32_t supersampled, int32_t out[3]);
/* The redshift of the disk around a spinning hole.  BHR_REDSHIFT_MODEL (the default) is the reference's g-factor model with
 * Kerr's orbital frequency, as above.  BHR_REDSHIFT_EXACT is the g-factor of the Kerr metric, g = nu_obs / nu_em with both
 * frequencies -p.u on the traced photon: a static observer at the camera; gas on the circular geodesic of Kerr's Omega at
 * r >= r_isco of the disk's sense of rotation (frame dragging included, the Doppler term from the photon's own L_z); and
 * inside the ISCO gas that keeps the ISCO orbit's energy and angular momentum and falls inward, down to the horizon.  (Inside
 * the photon orbit of the disk's sense no circular orbit exists; the guard of the circular branch would make the gas dark
 * there, but that branch is taken at r >= r_isco only, which lies outside the photon orbit at every spin.)  The photon's momentum at a crossing is interpolated like the hit
 * point (second order in the step).  Everything behind g -- intensity, radial profile, Wien tint, the sampler and its roll -- is
 * the model's (DESIGN.md "Kerr"; tests/kerr_redshift_ref.py is the CPU reference).  The march is the same: BG, the step count
 * and the crossings do not change, two kernels of the Kerr object of their own shade the disk.
 * EXACT needs the Kerr march: BHR_ERR_INVALID naming the combination without a spin or force_kerr (bhr_set_spin), for an
 * unknown mode, and from a bhr_set_spin that would switch the Kerr march off while EXACT is set.  A context that never calls
 * this launches what it always launched.  Ordered behind the frames in flight.  EXACT is also refused (BHR_ERR_INVALID) while the
 * Kerr march's disk source is the Disk V2 volume (bhr_disk_v2.h: bhr_set_kerr_disk_source), whose gas off the plane has no
 * four-velocity in this model; the Disk V2 surface takes both modes. */
#define BHR_REDSHIFT_MODEL 0
#define BHR_REDSHIFT_EXACT 1
BHR_API int32_t bhr_set_redshift(bhr_ctx *ctx, int32_t mode);
/* bhr_kerr_resources for the kernels of a redshift mode (BHR_REDSHIFT_MODEL: the same numbers). */
BHR_API int32_t bhr_kerr_redshift_resources(int32_t mode, int32_t supersampled, int32_t out[3]);
/* Anti-aliasing of the disk around a spinning hole: ray differentials and mip LOD for the Kerr march (bhr_config.anti_alias
 * is the Schwarzschild march's and stays refused with a spin).  on != 0: beside (x, p) every Kerr ray carries two tangents
 * (xi, pi) = d(x, p) / d(pixel), one per pixel axis, integrated by the same RK4 step with the same h (a constant of the step)
 * through the variational equations of the Hamiltonian system -- the right-hand side differentiated line by line in forward
 * mode.  Seeds: xi = 0 and pi the differential of the camera's momentum p = s d + f Lam l under the pinhole's direction
 * differential (the direction through the next pixel less the pixel's own), f and l being constants of the camera.  A
 * crossing's hit differentials are the x and y components of the two xi at the end of the crossing step (the reference's
 * convention, not projected onto the plane); its level of the disk texture's mip chain is
 * min(int(clamp(lod * strength, 0, 3)), last level) with lod = log2(max(|d(u, v)/dx|^2, |d(u, v)/dy|^2, 1)) in the Kerr texture
 * coordinates phi = atan2(hy, hx), r = sqrt(hx^2 + hy^2 - a^2) and the reference's 1e-6 guards; the roll's own derivative is
 * ignored, as the reference ignores it.  The g-factor of both redshift modes and the compositing are unchanged, and so is the
 * primal march: BG and the step count are the frame's without the switch, and at strength 0 so is DISK, bit for bit.
 * (DESIGN.md "Kerr anti-aliasing"; tests/kerr_aa_ref.py is the CPU reference.)  Four kernels of the Kerr object of their own
 * (model / exact redshift, plain / supersampled).  Ordered behind the frames in flight.
 * BHR_ERR_STATE without the Kerr march (bhr_set_spin); BHR_ERR_INVALID for a negative or non-finite strength.  While the switch
 * is on, BHR_ERR_INVALID naming the combination from bhr_kerr_raymap_build (a record has no differential words),
 * bhr_render_kerr_view (the seeds would need the aberration's Jacobian) and from a bhr_set_spin that would switch the Kerr
 * march off; and from this call while a Kerr Disk V2 source is set (bhr_disk_v2.h: bhr_set_kerr_disk_source -- the analytic
 * source has no mip chain). */
BHR_API int32_t bhr_set_kerr_anti_alias(bhr_ctx *ctx, int32_t on, float strength);
/* bhr_kerr_resources for the anti-aliased kernel of a redshift mode. */
BHR_API int32_t bhr_kerr_anti_alias_resources(int32_t redshift, int32_t supersampled, int32_t out[3]);
/* The Kerr ray map: the ray map (bhr_raymap_build above) of a spinning hole, an object of its own beside it.  A Kerr ray's path
 * depends on the camera, the geometry of bhr_config and the spin, not on the skybox, the disk texture or t_offset.
 * bhr_kerr_raymap_build(ctx, cam, 0) marches the whole-frame view `cam` once with the Kerr march of the context's redshift
 * mode and keeps per pixel what bhr_raymap_build keeps: the executed steps, the status (0 captured, 1 escaped, 2 out of
 * iterations), the normalized escape direction (zeros unless escaped), the number of annulus crossings, and the first K of
 * them front to back as 5 floats each -- hit_x, hit_y, and to_cam xyz under BHR_REDSHIFT_MODEL or the photon's momentum
 * (p_x, p_y, 0) at the hit under BHR_REDSHIFT_EXACT.  K = option "raymap_slots" (1..8).  A pixel with more crossings is put on
 * an overflow list.  Synchronises; ordered behind the frames in flight; the planes are reused by later builds of the same K.
 * The build records the spin, the redshift mode and the camera.
 * bhr_kerr_raymap_render(ctx, t, flags) is a frame: BG, DISK, and with them FINAL and the u8 rows, are bit for bit those of
 * bhr_render(ctx, &cam_t, flags) with cam_t the build camera at t_offset = t, under the scene as it is at the call.  The
 * records are shaded by csrc/march_kerr_raymap.hip's shade kernel, the pixels of the overflow list are marched by its fix
 * kernel in the same frame.  flags: BHR_SKIP_BLOOM | BHR_LENS_FLARE.  The frame takes the next frame slot, has one
 * timing-ring entry whose march bracket spans the two launches, and goes through the post-pass, grade, sinks and reads like
 * any frame; its ray-step count is that of the overflow pixels (bhr_kerr_raymap_desc.ray_steps has the build's, equal to a
 * marched frame's).  It neither counts towards nor runs the stream calibration.
 * bhr_kerr_raymap_render_view(ctx, cam, flags): the frame seen from `cam`, which must be the build camera turned rigidly about
 * the z axis (the checks of bhr_raymap_render_view).  The spin axis is z and the disk of a spinning hole is not tilted, so the
 * turn is an exact symmetry of everything a Kerr ray's path depends on: the stored records are turned with the camera (two
 * products and a sum per component) and shaded; overflow pixels are marched from `cam`.  Such a frame is the Kerr march of the
 * build view's rays, not bit for bit bhr_render's frame of `cam`; with `cam` the build camera it is bhr_kerr_raymap_render's
 * bit for bit.
 * bhr_kerr_raymap_read hands out BHR_RAYMAP_STEPS / _STATUS / _ESCAPE_DIR / _CROSSINGS as (rows, W[, 3]) and _HITS as
 * (K, rows, W, 5); bhr_kerr_raymap_info never fails for want of a map (built = 0 then); bhr_kerr_raymap_free is ordered behind
 * the frames in flight, and bhr_destroy releases the map.  The Schwarzschild map of the context, its point stars (bhr_set_stars)
 * and its polarisation neither see nor are changed by any of these calls.
 * Supersampled Kerr maps.  Option "kerr_raymap_supersample" (1, 2, 4 or 8; default 1) is the Kerr map's OWN factor k, read by
 * bhr_kerr_raymap_build as "raymap_slots" is; the map in memory keeps the factor it was built with, and a build with another
 * one reallocates.  ("raymap_supersample" stays the Schwarzschild map's and is refused here unless 1.)  The context's
 * bhr_set_supersample / bhr_set_adaptive_supersample stay at 1 for every map call.  With k > 1 the map is the map of the fine
 * frame: built by the Kerr march of bhr_set_supersample's fine camera (pixel pitch / k) of `cam`, every plane k rows x k W, the
 * overflow list in fine pixel indices -- a k x k group with any ray over K is listed whole.  bhr_kerr_raymap_info: width and rows
 * stay the output frame's; crossings_stored, overflow_pixels (a multiple of k^2) and ray_steps count fine rays, ray_steps equal
 * to that of a marched Kerr frame of the view with bhr_set_supersample(k).  bhr_kerr_raymap_desc keeps its layout;
 * bhr_kerr_raymap_get_supersample(ctx, &k) reports the factor, never fails for want of a map and gives 1 when there is none.
 * bhr_kerr_raymap_read hands out the fine planes, (k rows, k W[, 3]) and (K, k rows, k W, 5).  Device memory: k^2 x (24 + K x 20)
 * bytes per output pixel.
 * The frame: BG, DISK, FINAL and the u8 rows of bhr_kerr_raymap_render(ctx, t, flags) are bit for bit those of
 * bhr_render(ctx', &cam_t, flags), ctx' a context of the same configuration, spin and redshift with bhr_set_supersample(ctx', k).
 * The shade kernel shades each fine record list and resolves the k x k groups in the wave with bhr_set_supersample's filter
 * (pairwise tree, times 1 / k^2); the groups of the overflow list are marched and resolved by the map's supersampled fix
 * kernel.  No march runs per frame.  bhr_kerr_raymap_render_view takes such a map with its checks and meaning unchanged (the
 * camera is compared with the build camera as passed, at the output pitch): its frame is the Kerr march of the build view's
 * fine rays turned about z, resolved the same way.  Flags, frame slot, timing-ring entry, post-pass, grade, sinks and reads are
 * those of a frame from a k = 1 map; no calibration.
 * bhr_kerr_raymap_render_shutter(ctx, cams, n, flags): motion blur from the Kerr map -- one frame as the mean of n frames from
 * the map, with no march at all; bhr_raymap_render_shutter's contract with the Kerr names.  cams[0 .. n - 1] (1 <= n <= 64) are
 * the samples' cameras, each with its own t_offset.  What differs between the samples of one exposure is what the Kerr map leaves
 * free: the disk's roll (t_offset enters the disk sampler alone) and the orbit camera's turn about z, the spin axis, an exact
 * symmetry (the turn bhr_kerr_raymap_render_view applies).  A sample is accepted
 *   - if its pose equals the build camera's field for field (everything but t_offset): the still camera, whose turn is (1, 0);
 *   - else if it passes bhr_raymap_turn_of_build's checks against the Kerr map's camera, exactly as bhr_kerr_raymap_render_view's
 *     camera does (binary64; cosine and sine computed as there).
 * For each layer L in {BG, DISK}:
 *   L_j  is, bit for bit, what bhr_kerr_raymap_render_view(ctx, &cams[j], BHR_SKIP_BLOOM) stores for a turned camera and what
 *        bhr_kerr_raymap_render(ctx, cams[j].t_offset, BHR_SKIP_BLOOM) stores for a camera with the build pose;
 *   acc  = L_0, then acc = acc + L_j for j = 1 .. n - 1 in that order, one f32 addition per channel;
 *   L    = acc * (1.0f / (float)n): the reciprocal rounded to f32 once, the product once, no FMA contraction anywhere
 * -- bhr_render_shutter's mean, word for word (tests/shutter_ref.py restates it).  For n = 1 this is L_0 itself.  The post-pass is
 * the one behind every shutter frame (the pack launch for a split-f16 frame, then the frame's post-pass): BLUR, FINAL and the
 * u8 / u16 rows are what bhr_bloom computes from the resolved layers in this context (BHR_SKIP_BLOOM suppresses them),
 * BHR_LENS_FLARE adds what bhr_lens_flare adds; dither, grade, HDR plane, the sinks and the y4m stream work on the frame as on any
 * other.
 * Two routes give these bits.  A k = 1 map without overflow pixels takes ONE launch when n > 1 (csrc/march_kerr_raymap.hip:
 * kerr_raymap_shade_shutter_kernel) that shades a pixel's records under all n (t_offset, cos, sin, camera position) and keeps the
 * running sums on the chip.  A supersampled map (each sample is resolved first, then the mean), a map with overflow pixels -- or
 * any map while option "kerr_raymap_shutter_fused" is 0 -- runs, per sample, the shade launch and the fix launch over the overflow
 * list as bhr_kerr_raymap_render[_view] issues them, then bhr_render_shutter's accumulation launch (csrc/shutter.hip).
 * The frame takes the next frame slot and runs under the context's Kerr variant; one timing-ring entry, its march bracket from the
 * first shade launch to behind the last launch that writes BG / DISK; it neither counts towards nor runs the stream calibration.
 * bhr_counters: rays = n k^2 W H, ray_steps the sum of the overflow re-marches' steps (0 for a map without overflow pixels).
 * Asynchronous.  Refusals, with nothing launched and the context as it was: everything bhr_kerr_raymap_render refuses; ctx or cams
 * NULL, n < 1 or n > 64, a non-finite t_offset in any sample, a sample that is neither the build pose nor an admissible turn (the
 * message names the sample index): BHR_ERR_INVALID; a Kerr polarisation being set (bhr_set_kerr_polarization: a mean of frames
 * has no Stokes planes): BHR_ERR_STATE.  bhr_render_shutter keeps refusing a spin and bhr_raymap_render_shutter a Kerr context:
 * this is the call for the combination.
 * Kerr point stars (csrc/march_kerr_raymap.hip, csrc/api_stars.hip; DESIGN 4 "Kerr point stars").  The model is "point stars"
 * above, word for word, read over the Kerr map: the cells and triangles T0 / T1 of the Kerr map's stored escape directions, the
 * span rule, the Van Oosterom-Strackee solid angles, the difference form of the determinants, the cap at max_magnification, the
 * bilinear deposit and the star plane S -- gathered by the same kernel (csrc/stars.hip) over the Kerr map's status and direction
 * planes, from the camera-side pixel directions both marches launch their rays along.
 * bhr_set_kerr_stars(ctx, stars, n, p) sets the Kerr map's OWN catalogue: bhr_set_stars' checks, binning, defaults, n = 0
 * removal, whole-frame requirement, synchronisation and error codes, with this call's name in the messages.  It needs no spin.
 * The two catalogues are independent: bhr_set_stars' is ignored by every Kerr frame, and this one by everything but
 * bhr_kerr_raymap_render, bhr_kerr_raymap_render_view and bhr_kerr_raymap_read -- the Kerr march, bhr_render_kerr_observer and
 * every Schwarzschild call neither read nor change it.  A context without a Kerr catalogue launches exactly what it launches
 * without this paragraph.
 * With one set, bhr_kerr_raymap_render and bhr_kerr_raymap_render_view launch the gather kernel and the Kerr STARS shade kernel:
 * BG = fl(fl(sky_sample + S) * (1 - alpha_total)) per channel, the sky sample with the bits it has without a catalogue and the
 * sum one f32 addition; DISK is untouched; a pixel on the map's overflow list is stored by the Kerr fix kernel as without a
 * catalogue and receives NO star light.  The build view's plane is gathered once per (Kerr map, Kerr catalogue) -- a build, a
 * free and a new catalogue invalidate it -- and a turned view's plane per frame into storage of the frame slot, on the frame's
 * stream ahead of its march bracket, from the escape directions turned exactly as the Kerr shade kernel turns them.  A view at
 * angle 0 takes the cached plane and the un-turned kernels: bhr_kerr_raymap_render's frame bit for bit.  A Kerr polarisation may
 * be set at the same time: the Stokes pass runs behind the STARS shade and its planes do not depend on the catalogue.
 * bhr_kerr_raymap_read(ctx, BHR_RAYMAP_STARS, out, rows * W * 12) returns the build view's plane, computing it if needed.
 * bhr_get_kerr_stars_info: bhr_get_stars_info of this catalogue and its last gather.  bhr_kerr_stars_resources(exact, rot, out):
 * VGPRs, LDS bytes and scratch bytes of the Kerr STARS shade kernel of the model (exact = 0) or exact redshift, plain or turned.
 * Refused with BHR_ERR_STATE naming the stars, nothing launched, map and catalogue kept: bhr_kerr_raymap_render_shutter while a
 * Kerr catalogue is set; a render, a view or a BHR_RAYMAP_STARS read from a map with "kerr_raymap_supersample" > 1 while one is
 * set; a BHR_RAYMAP_STARS read without a Kerr catalogue (or without a map).  bhr_destroy frees both catalogues.
 * Not available: point stars or a Kerr polarisation on a supersampled map, point stars in shutter frames, on overflow pixels, in
 * marched Kerr frames and under the Kerr camera, several devices.
 *   BHR_ERR_STATE:  build without the Kerr march (no spin, not forced, no exact redshift): bhr_raymap_build is the call for a
 *                    hole that does not spin; render or read before a build (or after bhr_kerr_raymap_free); render while the
 *                    context's spin or redshift mode is no longer the build's (the message names both).
 *   BHR_ERR_INVALID: a row-block context; everything the Kerr march refuses (a tilted disk, anti_alias = 1, a Disk V2 source,
 *                    adaptive supersampling); bhr_set_supersample(k > 1); "raymap_supersample" other than 1 or "raymap_slots"
 *                    outside 1..8 at a build; "kerr_raymap_supersample" not 1, 2, 4 or 8 (refused by bhr_set_option; a
 *                    BHR_KERR_RAYMAP_SUPERSAMPLE outside it by the build), a build with k^2 W H >= 2^31 (refused by arithmetic,
 *                    before any allocation), or k > 1 while a Kerr polarisation is set (bhr_set_kerr_polarization: the momentum
 *                    build and the Kerr Stokes kernel have no supersampled twin; the message names both);
 *                    a build camera inside the static limit; any build flag; any other render flag;
 *                    a non-finite t_offset; a view camera that is not a turn of the build's about z; an unknown plane or a
 *                    wrong byte count.  Nothing is launched and the context renders as before. */
typedef struct {
    int32_t built, slots, width, rows;
    int32_t redshift;                   /* BHR_REDSHIFT_* the map was built under */
    float spin;                         /* a / M the map was built for */
    int64_t crossings_stored;
    int64_t overflow_pixels;
    int64_t device_bytes;
    uint64_t ray_steps;                 /* of the build: a marched Kerr frame's */
    bhr_camera cam;                     /* the build camera */
} bhr_kerr_raymap_desc;
BHR_API int32_t bhr_kerr_raymap_build(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags);
BHR_API int32_t bhr_kerr_raymap_render(bhr_ctx *ctx, float t_offset, uint32_t flags);
BHR_API int32_t bhr_kerr_raymap_render_view(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags);
BHR_API int32_t bhr_kerr_raymap_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags);
BHR_API int32_t bhr_kerr_raymap_read(bhr_ctx *ctx, int32_t plane, void *out, int64_t bytes);
BHR_API int32_t bhr_kerr_raymap_info(bhr_ctx *ctx, bhr_kerr_raymap_desc *out);
BHR_API int32_t bhr_kerr_raymap_get_supersample(bhr_ctx *ctx, int32_t *k);
BHR_API int32_t bhr_kerr_raymap_free(bhr_ctx *ctx);
BHR_API int32_t bhr_set_kerr_stars(bhr_ctx *ctx, const bhr_star *stars, int32_t n, const bhr_star_params *p);
BHR_API int32_t bhr_get_kerr_stars_info(bhr_ctx *ctx, bhr_stars_info *out);
BHR_API int32_t bhr_kerr_stars_resources(int32_t exact, int32_t rot, int32_t out[3]);
/* ---- Kerr line profile: the disk's relativistically broadened emission line from the Kerr ray map
 * (csrc/march_kerr_line.hip, csrc/api_kerr_line.hip; DESIGN 4 "Kerr line profile") ----
 * A narrow line of rest energy E0 emitted by the gas with emissivity eps is observed at E = g E0 with the specific intensity
 * g^4 eps delta(E - g E0) (Cunningham's transfer with a delta line), so the line flux is
 *   F(g) dg = sum over the image of g^p eps dOmega, binned in g = E_obs / E_em,      p = `power`, 4 by default.
 * With a line set, every bhr_kerr_raymap_render launches one more pass behind the frame's shade, over the records of the k = 1
 * Kerr map, with the Kerr Stokes kernel's mapping (a lane per pixel, an 8 x 8 tile per wave).  Per pixel the records are walked
 * front to back; of each record (hx, hy, v) -- v words 2..4: to_cam under BHR_REDSHIFT_MODEL, the photon's momentum under
 * BHR_REDSHIFT_EXACT -- all in f32:
 *   r      = sqrt(hx^2 + hy^2 - a^2), the Boyer-Lindquist hit radius; the record COUNTS iff r_inner <= r <= r_outer (the line's
 *            annulus, inside the disk's) and, under BHR_LINE_FIRST, no earlier record of the pixel counted;
 *   g      the context's redshift mode's g of the record, its cap (1.5) included: kerr_g_exact under the exact redshift, the
 *            model's g as the frame's g-factor computes it under the model (csrc/ray_kerr.h: kerr_g_model);
 *   dOmega = cos^3 theta, cos theta = D . forward for the pixel's unit ray direction D: the pinhole pixel's solid angle relative
 *            to the central pixel's;
 *   eps    BHR_LINE_POWERLAW: (r / r_inner)^(-index), independent of time;
 *          BHR_LINE_TEXTURE:  that times the disk texture's opacity at the crossing under the frame's roll (t_offset),
 *            alpha = 1 - (1 - min(A, 0.999))^6 with A the texture's fourth channel there (the frame's own disk_alpha);
 *   T      the transmittance in front of the record, 1 - alpha_total, accumulated over every record of the pixel inside the
 *            DISK's annulus exactly as the frame composites (alpha_total' = 1 - (1 - alpha_total) (1 - alpha)) -- under
 *            BHR_LINE_TEXTURE with BHR_LINE_ALL only; 1 otherwise: BHR_LINE_FIRST is an opaque disk of which the first counted
 *            crossing is seen whole, BHR_LINE_POWERLAW with BHR_LINE_ALL a transparent one;
 *   w      = ((powf(g, p) eps) dOmega) T.
 * A pixel on the map's overflow list (more crossings than slots) contributes nothing; their number is reported.
 * The histogram: t = (g - g_min) * scale with scale = (float)(n_bins / (g_max - g_min)), computed once on the host (binary64,
 * rounded once); t < 0 (or NaN) goes to `under`, else bin = (int)floorf(t), and bin >= n_bins to `over`.  A sample adds the integer
 * Q = llrintf(w * unit), unit = (float)(2^32 / 1.5^p), to a 64-bit unsigned cell: w unit <= 2^32 (g <= 1.5, eps, dOmega, T <= 1),
 * so the sum over 8 records of a 7680 x 4320 frame stays under 2^3 2^25 2^32 = 2^60 < 2^61.  Integer adds commute: whatever the
 * order of the LDS and global atomics, the cells are a function of the samples alone, run after run.  Flux = Q / unit / bin width.
 * A device ROW is n_bins cells, then under, over (sums of Q like the bins), the number of samples and the number of overflow pixels
 * skipped.  The pass of a frame goes into the row option "kerr_line_row" names at the call (default 0), which is cleared on the
 * frame's stream first; a frame whose row another frame slot's frame in flight wrote is ordered behind that frame.
 * Option "kerr_line_samples" = 1 makes the pass also store, per record, g and w as (slots, rows, W) f32 planes of the frame slot,
 * 0 where a record does not count: bhr_kerr_raymap_read(ctx, BHR_RAYMAP_LINE_G / BHR_RAYMAP_LINE_W, out, slots rows W 4) reads
 * those of the last such frame (BHR_ERR_STATE without one).
 * The frame itself -- BG, DISK, FINAL, the u8 rows -- is bit for bit what it is without the line; the map is only read.
 * bhr_set_kerr_line(ctx, p): sets the line (NULL: off).  BHR_ERR_STATE without the Kerr march (bhr_set_spin); BHR_ERR_INVALID
 *   naming the field for n_bins outside 1..4096, a range that is not finite with g_min < g_max, power outside [0, 8], index outside
 *   [0, 16], an unknown emissivity or orders, an annulus that is not inside the disk's (r_inner = r_outer = 0: the disk's own),
 *   reserved words other than 0, a row-block context.  It synchronises, drops the device rows and reserves two anew, zeroed.
 * bhr_kerr_line_reserve(ctx, n_rows): n_rows (1 .. 65536) zeroed device rows, e.g. one per frame of a video; synchronises.
 * bhr_kerr_line_read(ctx, first_row, n_rows, bins, under_over): bins n_rows x n_bins, under_over n_rows x 2; synchronises.
 * bhr_kerr_line_info(ctx, row, out): out = {overflow pixels skipped, samples} of the row; synchronises.
 * bhr_kerr_line_resources(redshift, texture, out): VGPRs, LDS bytes (static; the histogram is dynamic LDS, (n_bins + 4) 8 bytes)
 *   and scratch bytes of the kernel of a redshift mode and emissivity.
 * While a line is set, with nothing launched and the context as it was: bhr_kerr_raymap_build with "kerr_raymap_supersample" > 1
 * is BHR_ERR_INVALID (and with a Kerr Disk V2 source or the Kerr anti-aliasing on, as ever); bhr_kerr_raymap_render from a
 * supersampled map or with "kerr_line_row" outside the reserved rows, bhr_kerr_raymap_render_view with a turned camera and
 * bhr_kerr_raymap_render_shutter are BHR_ERR_STATE.  A Kerr polarisation and Kerr point stars may be set beside it. */
#define BHR_LINE_POWERLAW 0
#define BHR_LINE_TEXTURE 1
#define BHR_LINE_FIRST 0
#define BHR_LINE_ALL 1
#define BHR_LINE_MAX_BINS 4096
#define BHR_RAYMAP_LINE_G 7
#define BHR_RAYMAP_LINE_W 8
typedef struct {
    int32_t n_bins;                     /* 1 .. BHR_LINE_MAX_BINS */
    float g_min, g_max;                 /* the histogram's range [g_min, g_max) */
    float power;                        /* p of g^p: 4 for a line's flux */
    float index;                        /* q of the power-law emissivity */
    int32_t emissivity;                 /* BHR_LINE_POWERLAW or BHR_LINE_TEXTURE */
    int32_t orders;                     /* BHR_LINE_FIRST or BHR_LINE_ALL */
    float r_inner, r_outer;             /* the line's annulus; 0, 0: the disk's */
    int32_t reserved[3];                /* 0 */
} bhr_kerr_line;
BHR_API int32_t bhr_set_kerr_line(bhr_ctx *ctx, const bhr_kerr_line *p);
BHR_API int32_t bhr_kerr_line_reserve(bhr_ctx *ctx, int32_t n_rows);
BHR_API int32_t bhr_kerr_line_read(bhr_ctx *ctx, int32_t first_row, int32_t n_rows, uint64_t *bins, uint64_t *under_over);
BHR_API int32_t bhr_kerr_line_info(bhr_ctx *ctx, int32_t row, int64_t out[2]);
BHR_API int32_t bhr_kerr_line_resources(int32_t redshift, int32_t texture, int32_t out[3]);
/* A moving observer: one frame as a camera sees it that moves through bhr_camera.pos with velocity beta (a 3-vector in units of
 * c, |beta| <= 0.995) as the static observer there measures it.  That observer's local frame is identified with the coordinate
 * axes, as the camera that stands still identifies it; the camera basis is the moving camera's own.  With n' the pixel's
 * direction in that basis, gamma = 1 / sqrt(1 - beta.beta) and D = 1 / (gamma (1 - beta.n')) = nu_observed / nu_static, the ray
 * is traced along n = (n' + (gamma^2 / (gamma + 1)) (beta.n') beta - gamma beta) D (aberration) by the strict Schwarzschild
 * march; the disk's g-factor is g_doppler g_grav D ahead of its cap (brightness law and Wien shift), and with sky_shift != 0
 * the sky sample c becomes c (r_s I, I, b_s I) with Ds = clamp(D, 0.1, 1.5), I = Ds^1.5, w = 1 - 1 / Ds,
 * r_s = min(e^(2.21 w) / e^(2.72 w), 3), b_s = min(e^(3.13 w) / e^(2.72 w), 3), ahead of the product with 1 - alpha: BG may
 * exceed 1, FINAL clips as ever, the HDR plane carries the headroom.  sky_shift = 0: the sky is aberrated only.  (DESIGN.md
 * "Observer" states the model; tests/observer_ref.py is its CPU reference.)
 * The frame is bhr_render's in every other respect -- next frame slot, one timing-ring entry, counters, post-pass, lens flare,
 * grade, HDR plane, rows, dither, sinks and streams; asynchronous -- and is marched by the observer object
 * (csrc/march_observer.hip) whatever bhr_config.math_mode is, beta = 0 included, where BG, DISK and ray_steps are the strict
 * march's bit for bit; the post-pass follows the context's arithmetic.  The velocity travels with the call: frames in flight
 * may differ in it.  Works with a tilted disk and bhr_set_supersample.  flags: BHR_SKIP_BLOOM, BHR_LENS_FLARE.
 * BHR_ERR_INVALID with a message that names the combination, nothing launched and the context untouched: a null argument, a NaN
 * in beta or |beta| > 0.995, any other flag bit, anti_alias = 1, a Disk V2 source, adaptive supersampling, a spin or the forced
 * Kerr march (bhr_set_spin) or the exact redshift, a row-block context. */
typedef struct {
    float beta[3];
    int32_t sky_shift;
} bhr_observer;
BHR_API int32_t bhr_render_observer(bhr_ctx *ctx, const bhr_camera *cam, const bhr_observer *obs, uint32_t flags);
/* out = {VGPRs per lane, LDS bytes per block, scratch bytes per lane} of the observer march kernel (supersampled != 0: of its
 * supersampled twin), from hipFuncGetAttributes.  No context. */
BHR_API int32_t bhr_observer_resources(int32_t supersampled, int32_t out[3]);
/* Projections: one frame through an equirectangular (360 degree panorama) or an equidistant fisheye (dome master) camera instead
 * of the pinhole.  The frame is bhr_render_observer's frame in every respect but the pixel's direction n' -- next frame slot,
 * one timing-ring entry, counters, post-pass following the context's arithmetic, lens flare, grade, HDR plane, u8 / u16 rows,
 * dither, sinks, streams; asynchronous; a tilted disk and bhr_set_supersample work; the texture source only, no ray
 * differentials -- and is marched by the projected object (csrc/march_projected.hip).  Of cam, pos, right, up, forward,
 * r_escape and t_offset are used; pixel_width and pixel_height are ignored.
 * F, R, U are cam's forward, right and up, Wf x Hf the grid the march walks (k W x k H under bhr_set_supersample(k)), (i, j) the
 * fine pixel; everything is f32, every operation rounded once, the two spans made in binary64 and rounded once:
 *   BHR_PROJ_EQUIRECT   fov_h_deg in (0, 360], fov_v_deg in (0, 180]; 360 x 180 is the full sphere
 *       lon = (((float)i + 0.5f) / (float)Wf - 0.5f) * span_h        span_h = (float)radians(fov_h_deg)
 *       lat = (0.5f - ((float)j + 0.5f) / (float)Hf) * span_v        span_v = (float)radians(fov_v_deg)
 *       a = cosf(lat) * cosf(lon);  b = cosf(lat) * sinf(lon);  c = sinf(lat)
 *       n'_k = (a * F_k + b * R_k) + c * U_k
 *     longitude grows towards right, row 0 is the top, the image centre looks along forward.
 *   BHR_PROJ_FISHEYE    equidistant; fov_h_deg in (0, 360] is the full angle of the image circle, which is inscribed in the
 *                       shorter side; fov_v_deg is ignored
 *       s = 2.0f / (float)min(Wf, Hf)
 *       x = (((float)i + 0.5f) - (float)Wf / 2) * s;   y = ((float)Hf / 2 - ((float)j + 0.5f)) * s
 *       rho = sqrtf(x * x + y * y);   inside = rho <= 1.0f
 *       theta = rho * half                                            half = (float)(radians(fov_h_deg) / 2)
 *       inv = rho > 0 ? 1.0f / rho : 0.0f
 *       a = cosf(theta);  b = sinf(theta) * (x * inv);  c = sinf(theta) * (y * inv);   n'_k as above
 *     a pixel that is not inside takes no step and its BG and DISK are exactly 0; under supersampling it enters the box filter
 *     as zeros, which anti-aliases the rim.  bhr_counters.rays is k^2 W H for either projection, ray_steps the steps taken.
 * sinf / cosf are the device library's accurate functions, evaluated once per ray (their bits are not pinned); n' is unit to a
 * few ulps and not renormalised.  With obs != NULL, n' is the n' of bhr_render_observer: aberration, D in the disk's g, the sky
 * under sky_shift exactly as stated there.  obs == NULL: the camera stands still, the frame bit for bit that of
 * obs = {{0, 0, 0}, 0}.  flags: BHR_SKIP_BLOOM, BHR_LENS_FLARE.  A star catalogue is ignored, as bhr_render ignores it.  The
 * bloom is an image-space pass and does not wrap at the +-180 degree seam.  (DESIGN.md "Projections"; tests/projection_ref.py is
 * the CPU reference.)
 * BHR_ERR_INVALID with a message that names the combination, nothing launched and the context untouched: a null ctx, cam or
 * proj, an unknown kind, a NaN or out-of-range field of view, any other flag bit, everything bhr_render_observer refuses for
 * its obs, anti_alias = 1, a Disk V2 source, adaptive supersampling, a spin or the forced Kerr march or the exact redshift, a
 * row-block context. */
#define BHR_PROJ_EQUIRECT 1
#define BHR_PROJ_FISHEYE  2
typedef struct {
    int32_t kind;
    float fov_h_deg, fov_v_deg;
    int32_t reserved;
} bhr_projection;
BHR_API int32_t bhr_render_projected(bhr_ctx *ctx, const bhr_camera *cam, const bhr_projection *proj,
                                     const bhr_observer *obs /* NULL: the camera stands still */, uint32_t flags);
/* out = {VGPRs per lane, LDS bytes per block, scratch bytes per lane} of the projected march kernel (supersampled != 0: of its
 * supersampled twin), from hipFuncGetAttributes.  No context. */
BHR_API int32_t bhr_projected_resources(int32_t supersampled, int32_t out[3]);
/* The Kerr camera: one frame of the spinning hole (bhr_set_spin, or the Kerr march forced at spin 0) through a camera that may
 * move and may be panoramic.  Units r_s = 1, M = 1/2, a = A / 2.  The Kerr march identifies the static observer's local frame at
 * the camera with the Kerr-Schild coordinate axes: a pixel's direction is the photon's coordinate direction d, from which the
 * march makes its momentum (s = 1 / sqrt(1 - f (1 - (l.d)^2)), Lam = (1 + s l.d) / (1 - f), p = s d + f Lam l).  This call keeps
 * that convention and puts the camera model of bhr_render_observer and bhr_render_projected ahead of it:
 *   n'   the pixel's direction in the camera's own frame: the pinhole's (proj == NULL: bhr_render's), or the equirectangular or
 *        fisheye direction exactly as stated for bhr_render_projected (same formulas and spans; here a product and the sum behind
 *        it may be one fused multiply-add); a fisheye pixel outside the image circle takes no step, its BG and DISK are exactly
 *        0 and enter the box filter of a supersampled frame as zeros; bhr_counters.rays is k^2 W H
 *   beta the velocity (units of c, |beta| <= 0.995) the static observer at bhr_camera.pos measures; obs == NULL: the camera
 *        hovers, the frame bit for bit that of obs = {{0, 0, 0}, 0}
 *   D  = 1 / (gamma (1 - beta.n'))                                       gamma = 1 / sqrt(1 - beta.beta)
 *   n  = (n' + (gamma^2 / (gamma + 1)) (beta.n') beta - gamma beta) D    f32; gamma, gamma^2 / (gamma + 1) binary64 rounded once
 * n is not renormalised and takes the place of d.  The RK4 loop, step rule, capture at r_plus, escape and crossings are the Kerr
 * march's.  D is a factor of the disk's g ahead of its cap in both redshift modes (bhr_set_redshift):
 *   model   g = min((g_doppler (grav_num / grav_den)) D, 1.5)
 *   exact   g = min((nu_obs D) / max(nu_em, 1e-3), 1.5)                   the static observer's nu_obs turned into the moving one's
 * and with sky_shift != 0 the sky sample is scaled as stated for bhr_render_observer (BG may exceed 1, FINAL clips).  With
 * beta = 0 and proj == NULL, under either sky setting, BG, DISK, FINAL and ray_steps are bhr_render's Kerr frame bit for bit.
 * The frame is bhr_render's in every other respect -- next frame slot, one timing-ring entry, counters, post-pass following
 * math_mode, lens flare, grade, HDR plane, sinks; asynchronous -- and is marched by the Kerr camera's object
 * (csrc/march_kerr_observer.hip) under the context's redshift mode.  The velocity and the projection travel with the call: frames
 * in flight may differ in them.  Works with bhr_set_supersample.  flags: BHR_SKIP_BLOOM, BHR_LENS_FLARE.  (DESIGN.md "Kerr
 * camera"; tests/kerr_observer_ref.py is the CPU reference; bhr_amd.observer.kerr_velocity has the circular orbit's and the
 * zero-angular-momentum observer's velocity.)
 * BHR_ERR_INVALID with a message that names the combination, nothing launched and the context untouched: a null ctx or cam; no
 * spin and no forced Kerr march; a NaN in beta or |beta| > 0.995; an unknown projection kind or a field of view
 * bhr_render_projected refuses; any other flag bit; everything bhr_set_spin refuses (a tilted disk, anti_alias = 1, a Disk V2
 * source, adaptive supersampling, a row-block context); a camera inside the static limit. */
BHR_API int32_t bhr_render_kerr_view(bhr_ctx *ctx, const bhr_camera *cam, const bhr_observer *obs /* NULL: at rest */,
                                     const bhr_projection *proj /* NULL: pinhole */, uint32_t flags);
/* out = {VGPRs per lane, LDS bytes per block, scratch bytes per lane} of the Kerr camera's march kernel of a redshift mode
 * (BHR_REDSHIFT_*; supersampled != 0: of its supersampled twin), from hipFuncGetAttributes.  No context. */
BHR_API int32_t bhr_kerr_view_resources(int32_t mode, int32_t supersampled, int32_t out[3]);
/* Light delay: one frame in which every disk crossing is shaded at the coordinate time its light LEFT the gas, not at the frame's
 * one instant.  Units r_s = 1, c = 1: t_offset is coordinate time in r_s / c.  The strict Schwarzschild march integrates
 * x'' = -1.5 L^2 x / r^5 with |d| = 1 at the camera; along that parameter l a null geodesic has energy
 * E = sqrt(1 - L^2 / r_cam^3) (L^2 = |d x p|^2 at launch) and dt/dl = E w(r), w(r) = r / (r - 1) with r clamped to
 * max(r, 1 + 1e-3) as the march clamps it.  The march accumulates, f32, every operation rounded once, no contraction, sqrt and
 * quotients correctly rounded:
 *   launch     E = sqrt(1 - L2 / (r2p * r)),  w = wr(r),  T = 0                  wr(r): rs = max(r, 1 + 1e-3); rs / (rs - 1)
 *   step       from (p, d, r) to (np, nd, rn) under the step's own h:
 *              m_k = 0.5 * (p_k + np_k) + (0.125 * h) * (d_k - nd_k)             the Hermite midpoint
 *              rm = sqrt((m.x m.x + m.y m.y) + m.z m.z)
 *              dT = (E * (h / 6)) * ((w + 4 * wr(rm)) + wr(rn))                  Simpson's rule, fourth order like the RK4
 *   crossing   T_hit = T + t_frac * dT, t_frac the step's own hit fraction f_old / (f_old - f_new + 1e-8)
 *   commit     T = T + dT,  w = wr(rn)
 *   shade      the crossing is shaded exactly as bhr_render shades it, but under t_eff = t_offset - scale * T_hit
 *              (one product, one difference): the texture's Keplerian roll is phi + t_eff Omega(r).
 * Redshift, brightness, alpha, the sky, step counts and termination do not see T.  scale = 1 is physical, larger values
 * exaggerate the delay for teaching, and scale = 0 gives BG, DISK and ray_steps of the strict march bit for bit (T_hit is finite
 * for every crossing).  The texture stays the frame's: its population and noise do not evolve within the delay.  (DESIGN.md
 * "Light delay"; tests/delay_ref.py is the CPU reference.)
 * The frame is bhr_render's in every other respect -- next frame slot, one timing-ring entry, counters, post-pass following the
 * context's arithmetic, lens flare, grade, HDR plane, u8 / u16 rows, dither, sinks and streams; asynchronous -- and is marched
 * by the delay object (csrc/march_delay.hip) whatever bhr_config.math_mode is.  The scale travels with the call: frames in flight
 * may differ in it.  Works with a tilted disk and bhr_set_supersample.  flags: BHR_SKIP_BLOOM, BHR_LENS_FLARE.
 * BHR_ERR_INVALID with a message that names the combination, nothing launched and the context untouched: a null argument, a NaN,
 * negative or > 16 scale, reserved != 0, any other flag bit, anti_alias = 1, a Disk V2 source, adaptive supersampling, a spin or
 * the forced Kerr march (bhr_set_spin) or the exact redshift, a row-block context. */
typedef struct {
    float scale;
    int32_t reserved;
} bhr_light_delay;
BHR_API int32_t bhr_render_delayed(bhr_ctx *ctx, const bhr_camera *cam, const bhr_light_delay *d, uint32_t flags);
/* out = {VGPRs per lane, LDS bytes per block, scratch bytes per lane} of the delayed march kernel (supersampled != 0: of its
 * supersampled twin), from hipFuncGetAttributes.  No context. */
BHR_API int32_t bhr_delayed_resources(int32_t supersampled, int32_t out[3]);
/* The library's switches.  Each has an environment variable that bhr_create reads ONCE (no entry point calls getenv
 * afterwards) and can be changed per context later with this call -- what tests and A/B tools use:
 *   "bloom_split"     BHR_BLOOM_SPLIT     -1 post-pass by arithmetic (exact f32 under strict, split f16 under fast / hybrid), 0 / 1 force
 *   "bloom_tiles"     BHR_BLOOM_TILES     0 output tiles per wave of the split post-pass by launch size, 1..8 force (A/B runs)
 *   "hybrid_repair"   BHR_HYBRID_REPAIR   -1 guards + strict fix list by view (anti-aliased or tilted), 0 / 1 force
 *   "hybrid_band_lo" / "hybrid_band_hi" / "hybrid_band_default"   BHR_HYBRID_BAND="lo,hi"   strict band around b_c, in r_s
 *   "hybrid_pad"      BHR_HYBRID_PAD      share of its own span of b a tile spanning <= 0.1 r_s is padded by in the strict-band test (default 0.5; larger tiles: up to all of it)
 *   "hybrid_streams"  BHR_HYBRID_STREAMS  -1 (default) the two lists of a hybrid march on one stream where two frame slots overlap
 *                                         frames and on two where a frame runs alone; 1 / 2 force
 *   "calibrate_streams" BHR_CALIBRATE_STREAMS 1 (default) a context with two frame slots times six candidate streams for slot 1 on
 *                                         its ninth frame and keeps the fastest (~0.15 s once; csrc/calibrate.hip)
 *   "hybrid_classify" BHR_HYBRID_CLASSIFY 1 (default) a view change classifies the tiles and partitions the launch order on the
 *                                         device (~0.05 ms whatever the size), 0 on the submitting thread (the same lists)
 *   "mip_lds"         BHR_MIP_LDS         1 anti-aliased fast frames stage the coarse mip levels in LDS
 *   "group_threads"   BHR_GROUP_THREADS   -1 one submitting thread per tile where the tiles sit on distinct devices, 0 / 1 force
 *   "group_schedule"  BHR_GROUP_SCHEDULE  -1 by flags, else pipelined where a halo copy can hide (exact-f32 post-pass on distinct
 *                                         devices) and serial otherwise; 0 serial, 1 pipelined (explicit flags still win)
 *   "png16_menu"      BHR_PNG16_MENU      1 (default) the 16-bit device PNG encoder codes from its own menu, 0 from the 8-bit one (A/B runs)
 *   "shutter_timing"  BHR_SHUTTER_TIMING  1 a shutter frame brackets each of its accumulation launches with a pair of HIP events
 *                                         (bhr_debug_read, which = 5; ~5 us per event in the frame's stream); default 0
 *   "grade_timing"    BHR_GRADE_TIMING    1 a graded frame (bhr_set_grade) brackets each launch of its grade stage with a pair of HIP
 *                                         events (bhr_debug_read, which = 6); default 0
 *   "raymap_slots"    BHR_RAYMAP_SLOTS    crossings a ray map keeps per pixel (1..8, default 4); read by bhr_raymap_build
 *   "raymap_supersample" BHR_RAYMAP_SUPERSAMPLE the next ray map's own supersampling factor (1, 2, 4 or 8, default 1): k x k records per
 *                                         pixel, resolved in the shade; read by bhr_raymap_build; anything else: BHR_ERR_INVALID
 *   "kerr_raymap_supersample" BHR_KERR_RAYMAP_SUPERSAMPLE the next Kerr ray map's own supersampling factor (1, 2, 4 or 8, default 1): k x k
 *                                         records per pixel, resolved in the shade; read by bhr_kerr_raymap_build; anything else: BHR_ERR_INVALID
 *   "raymap_shutter_fused" BHR_RAYMAP_SHUTTER_FUSED 1 (default) bhr_raymap_render_shutter shades all samples of a map without overflow
 *                                         pixels in one launch, 0 sample by sample with the accumulation launches (the same bits; A/B runs)
 *   "kerr_raymap_shutter_fused" BHR_KERR_RAYMAP_SHUTTER_FUSED 1 (default) bhr_kerr_raymap_render_shutter shades all samples of a k = 1 Kerr
 *                                         map without overflow pixels in one launch, 0 sample by sample likewise (the same bits; A/B runs)
 *   "kerr_line_row"   (no variable)       the device row the Kerr line pass of the next bhr_kerr_raymap_render fills (bhr_set_kerr_line;
 *                                         0 .. 65535, default 0; the render refuses a row that is not reserved)
 *   "kerr_line_samples" (no variable)     1 the Kerr line pass also stores the per-record g and w planes (BHR_RAYMAP_LINE_G / _W); default 0
 * (bhr_create only: BHR_FRAME_SLOTS.) */
BHR_API int32_t bhr_set_option(bhr_ctx *ctx, const char *name, double value);
/* Diagnostics (tests): the split-f16 post-pass's packed intermediates of the last frame as raw bytes -- which = 0 the H pass's
 * input (csrc/bloom.hip: pa), 1 its output / the V pass's input (pb) -- and the layout's geometry: geom[10] = {NT, n_tx, WP, YB,
 * GP, g0, t_first, n_ty, pbr, GR}; which = 2 the launch order of the last math-hybrid march as int32 tile indices, strict tiles
 * first (geom[0] = tiles in it; bhr_hybrid_info tells how many are strict).  out == NULL or bytes == 0: geometry only.
 * which = 5 (option "shutter_timing"): geom[0] = accumulation launches of the last shutter frame, geom[1] = their summed
 * HIP-event time in nanoseconds (bhr_render_shutter: n for n > 1; bhr_raymap_render_shutter: n on its sample-by-sample route,
 * 0 on its fused route, which has no accumulation launch).  which = 6 (option "grade_timing"): the same for the launches of the last graded frame's
 * grade stage (csrc/grade.hip: one, or two for a flared frame).
 * Synchronises. */
BHR_API int32_t bhr_debug_read(bhr_ctx *ctx, int32_t which, void *out, int64_t bytes, int32_t *geom);
/* TaichiRenderer._apply_lens_flare(final, disk) (render.py:3925-4028) on the device, standalone:
 * FINAL <- clip(FINAL + flare(DISK), 0, 1) for a whole-frame context.  bhr_render / bhr_group_render
 * with BHR_LENS_FLARE run the same kernels after the combine.  Asynchronous. */
BHR_API int32_t bhr_lens_flare(bhr_ctx *ctx);
/* The three frame sums the flare is built from, as the reference computes them (render.py:3931-3939):
 * out3 = { np.sum(glow) (f32 value), np.sum(x * glow), np.sum(y * glow) } with glow = max(DISK, axis=2),
 * accumulated in NumPy's own summation order, hence bit-identical to it.  Synchronises. */
BHR_API int32_t bhr_lens_flare_sums(bhr_ctx *ctx, double *out3);
/* save_image()'s quantisation (clip*255 truncated to u8, render.py:423) done
 * on the device: (row1-row0, width, 3) u8.  Synchronises. */
BHR_API int32_t bhr_read_final_u8(bhr_ctx *ctx, uint8_t *out);
/* The frame at 16 bits per sample: q16 = (uint16)(int)(clip(x, 0, 1) * 65535.0f), the truncation of the 8-bit path with
 * 65536 levels (the product rounded to f32; NaN -> 0).  (row1-row0, width, 3) u16, native endian.  A kernel of its own
 * quantises the f32 FINAL frame on demand (a frame that kept only its u8 rows gets the f32 frame from its V pass first) into
 * a buffer of the frame slot that exists from the first use on; nothing changes for a context that never asks.  Row-block
 * contexts and two frame slots work as for bhr_read_final_u8.  Synchronises.  The 16-bit PNG encoders (bhr_output.h) read
 * the same rows. */
BHR_API int32_t bhr_read_final_u16(bhr_ctx *ctx, uint16_t *out);
/* Dithered 8-bit quantisation.  mode BHR_DITHER_NONE (default): the u8 rows are save_image's truncation, as ever.
 * BHR_DITHER_BLUE: q8 = (uint8)floorf(clip(x, 0, 1) * 255.0f + t(c, X, Y)) with
 *   t(c, X, Y) = (M[(Y + oy_c) & 63][(X + ox_c) & 63] + 0.5f) / 4096.0f,
 * M the 64 x 64 blue-noise rank matrix of bhr_dither_matrix, (X, Y) the pixel's coordinates in the FULL image (a row block
 * dithers exactly as the whole frame does) and (ox, oy) = (0, 0) for R, (21, 37) for G, (43, 11) for B.  f32 arithmetic, the
 * product and then the sum rounded once each; the largest value is 255 + 4095.5 / 4096 < 256.  A flat value v thus rounds up
 * in exactly the share frac(255 v) of the pixels (to 1 / 4096), and the pattern that decides which has no energy at low
 * spatial frequencies: bands become fine noise.  The pattern does not depend on the frame.
 * While dither is on EVERY consumer of the context's u8 rows sees the dithered rows: bhr_read_final_u8, the device and host
 * PNG paths, the sinks, the JPEG encoder and the y4m stream.  The frame takes the route of a flared frame: its V pass keeps
 * f32 and a kernel of its own quantises afterwards.  bhr_group_render* with BHR_GATHER_U8 and bhr_tile_render store their u8
 * rows from inside the V pass into peer memory: with dither on they return BHR_ERR_INVALID.  Changing the mode drains the
 * frames in flight and invalidates the u8 rows in memory (the next reader gets them under the new mode, bit for bit what a
 * context that never changed mode gives).  bhr_read_final_u16 is not dithered. */
#define BHR_DITHER_NONE 0
#define BHR_DITHER_BLUE 1
BHR_API int32_t bhr_set_dither(bhr_ctx *ctx, int32_t mode);
/* The rank matrix M, row-major (out[64 y + x] = M[y][x]): every value of 0 .. 4095 once; void-and-cluster on a torus with a
 * Gaussian energy, generated by tools/make_blue_noise.py and compiled in.  Host only, needs no GPU. */
BHR_API int32_t bhr_dither_matrix(uint16_t out[4096]);
/* Grading: exposure, a highlight roll-off and a display transfer function in place of the combine's hard clip, between the
 * combine and the quantisers.  Per value, all in f32, every operation rounded once:
 *   x = (bg + disk) + blur                  the combine's own order; blur = 0 for a BHR_SKIP_BLOOM frame
 *   h = fminf(fmaxf(x, 0), 65504)           the HDR value: NaN -> 0 as in the quantisers, +inf -> 65504
 *   v = h * gain                            gain = (float)exp2((double)exposure_stops)
 *   BHR_GRADE_CLIP      y = fminf(v, 1)
 *   BHR_GRADE_REINHARD  y = fminf((v * (1 + v * iw2)) / (1 + v), 1)          iw2 = (float)(1 / ((double)white * white)): v = white -> 1
 *   BHR_GRADE_ACES      y = fminf(fmaxf((v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f), 0), 1)
 *   BHR_TRANSFER_LINEAR FINAL = y
 *   BHR_TRANSFER_SRGB   FINAL = y <= 0.0031308f ? 12.92f * y : 1.055f * powf(y, 1.0f / 2.4f) - 0.055f
 * bhr_set_grade(ctx, NULL) switches the stage off (the default): an ungraded frame launches the kernels it always has.
 * {BHR_GRADE_CLIP, 0 stops, BHR_TRANSFER_LINEAR} is not a synonym for off: it runs the stage, and gives the ungraded frame bit
 * for bit.  While a grade is set a frame of bhr_render / bhr_render_shutter takes the route of a flared or dithered frame: its
 * V pass stores BLUR only, one kernel (csrc/grade.hip) writes FINAL -- and the frame's u8 rows where bhr_set_outputs asked for
 * them and dither is off -- and FINAL is the authority for everything made on demand: bhr_read_final_u8 / _u16, the dither,
 * the PNG and JPEG paths, the sinks and the y4m stream.  With BHR_LENS_FLARE the flare sits in front of the sensor response:
 * x is fmaxf(((bg + disk) + blur) + flare, 0), the flare's term added without the upper clip.  keep_hdr != 0: the frame keeps
 * its plane h (scene-linear, before exposure, with the flare if it had one), one more (rows, W, 3) f32 buffer of the frame slot
 * from the first use on, read with bhr_read_layer(BHR_LAYER_HDR) -- BHR_ERR_STATE for a frame that did not keep it;
 * bhr_write_layer refuses the layer.  The plane is also what the HDR video stream converts (bhr_output.h: bhr_y4m_open_hdr).
 * bhr_set_grade drains the frames in flight and applies to the frames rendered afterwards; frames in memory keep the outputs
 * they were rendered with.  BHR_ERR_INVALID, with the context as it was: op not in {0, 1, 2}, transfer not in {0, 1},
 * exposure_stops non-finite or outside [-16, 16], white non-finite or outside (0, 65504].  The stand-alone bhr_bloom and
 * bhr_lens_flare stay the reference's functions and ignore the grade.  bhr_group_render*, bhr_tile_export and bhr_tile_render
 * store rows from inside their V passes into peer memory: while a grade is set they return BHR_ERR_INVALID.  bhr_render on a
 * row-block context works (without flare, as ever). */
#define BHR_GRADE_CLIP 0
#define BHR_GRADE_REINHARD 1
#define BHR_GRADE_ACES 2
#define BHR_TRANSFER_LINEAR 0
#define BHR_TRANSFER_SRGB 1
typedef struct { int32_t op, transfer; float exposure_stops, white; int32_t keep_hdr; } bhr_grade;
BHR_API int32_t bhr_set_grade(bhr_ctx *ctx, const bhr_grade *g);   /* NULL: off (the default) */
/* Stand-alone, like bhr_bloom: FINAL <- grade((BG + DISK) + BLUR) of the layers in the active frame slot, without flare; the
 * plane h is kept if keep_hdr is set.  Invalidates the u8 and u16 rows.  Asynchronous.  BHR_ERR_STATE while no grade is set.
 * Works on row-block contexts too: the stage is per value. */
BHR_API int32_t bhr_grade_frame(bhr_ctx *ctx);
BHR_API int32_t bhr_get_counters(bhr_ctx *ctx, bhr_counters *out);
/* Last BHR_MATH_HYBRID march of this context: out_tiles = {tiles marched strict, tiles of the row block},
 * out_band = {lo, hi}: the strict band [b_c - lo, b_c + hi] of impact parameters, in r_s. */
BHR_API int32_t bhr_hybrid_info(bhr_ctx *ctx, int32_t out_tiles[2], double out_band[2]);
/* Guards of the last BHR_MATH_HYBRID frame: out = {pixels its fast list handed over to the strict fix kernel, capacity of that
 * list}.  The count runs past the capacity -- pixels beyond it keep their fast value -- so out[0] > out[1] says that a view
 * needs a larger list than an eighth of the block's pixels.  {0, 0}: the frame ran without guards.  Synchronises. */
BHR_API int32_t bhr_hybrid_repairs(bhr_ctx *ctx, int32_t out[2]);
/* Device self-test of the strict march's hand-written exact sqrt / divide / divide-by-6 against the
 * compiler's IEEE sequences: out[0..2] = mismatches (sqrt over every f32 in [2^-80, 2^80); 1/x over
 * the same range plus a/b over 2^30 random pairs; x/6 over the same range), out[3] = comparisons made. */
BHR_API int32_t bhr_selftest(bhr_ctx *ctx, uint64_t out[4]);
/* forget the per-frame timing ring (call before a timed region) */
BHR_API int32_t bhr_timing_reset(bhr_ctx *ctx);
/* The last n timed bhr_render calls, oldest first: out[3 k .. 3 k + 2] = march start, march end, frame end of frame k in
 * milliseconds after the oldest frame's march start (HIP events on the frame slots' streams).  Synchronises. */
BHR_API int32_t bhr_timing_dump(bhr_ctx *ctx, float *out, int32_t n);
/* BHR_MIP_LDS=1 (environment of bhr_create): anti-aliased frames of the fast arithmetic stage the coarse levels of the disk
 * texture's mip stack in LDS -- as many of levels 3, 2, 1 as fit 44 KB -- and sample them from there (BASELINE.json's "mipmap
 * levels staged through LDS"; not the default: DESIGN.md section 4).  Returns the first staged level of the last such march,
 * -1 if it staged none (switch off, another arithmetic, or a texture whose level 3 alone exceeds the budget). */
BHR_API int32_t bhr_mip_lds_level(bhr_ctx *ctx);
/* Cost of each band of 8 rows in the last bhr_render(..., BHR_ROW_COSTS), in ray-step units: the ray-steps marched
 * plus 320 per wave-wide shading pass.  n = ceil(rows / 8) values.
 * The step count of a ray depends on the camera, the step size and the escape radius only -- not on the
 * textures -- so a small probe frame gives the cost profile of a large one (multigpu.balanced_row_blocks). */
BHR_API int32_t bhr_get_row_costs(bhr_ctx *ctx, uint64_t *out, int32_t n);
/* The same profile split by the arithmetic that took the steps: a math_mode 2 (hybrid) frame marches its tiles near the
 * photon ring with the strict kernel, ~2.2x the cost per step of the fast one -- row blocks of hybrid frames are balanced
 * on fast + 2.2 strict (multigpu.probe_row_costs).  A strict frame has everything in strict_out, a fast one in fast_out. */
BHR_API int32_t bhr_get_row_costs_split(bhr_ctx *ctx, uint64_t *fast_out, uint64_t *strict_out, int32_t n);

/* ---- multi-GPU row-block tiling (one process driving N devices) -----------
 * ctxs[k] renders rows [row0_k,row1_k) of the same image; blocks must be
 * contiguous, ordered and cover [0,height).  Marches all tiles concurrently,
 * exchanges the R = int(0.02*W) H-blurred halo rows between neighbours with
 * hipMemcpyPeerAsync, runs the V pass per tile and gathers the final tiles:
 * with BHR_GATHER_PEER into a full-frame f32 buffer on ctxs[0]'s device, with BHR_GATHER_U8 into a quantised u8 one
 * (peer copies over xGMI, no collective), and, if out_host != NULL, into out_host (H, W, 3) through per-device pinned
 * buffers.  Two schedules (csrc/group.hip), same bytes: pipelined -- the halo pull runs under the V pass of the rows
 * that need no halo, finished row chunks are pushed while the next chunk's V pass runs -- and serial; see
 * BHR_GROUP_SERIAL / BHR_GROUP_PIPELINED.  Synchronises. */
BHR_API int32_t bhr_group_render(bhr_ctx **ctxs, int32_t n, const bhr_camera *cam, uint32_t flags, float *out_host);
/* The same with only the tiles k with live[k] != 0 rendering; the others keep the buffers (halo rows, gathered rows,
 * glow rows) of the last call in which they were live.  live == NULL: all.  Times one tile of N end to end on one
 * device (bench.py tile_scaling): its counters' frame_ms then spans first march launch .. its rows landed on tile 0. */
BHR_API int32_t bhr_group_render_subset(bhr_ctx **ctxs, int32_t n, const bhr_camera *cam, uint32_t flags, float *out_host,
                                        const int32_t *live);
/* Waits for every frame the tiles have in flight (BHR_GROUP_ASYNC). */
BHR_API int32_t bhr_group_sync(bhr_ctx **ctxs, int32_t n);
/* The quantised frame the last bhr_group_render(..., BHR_GATHER_U8) gathered on this context's device: (H, W, 3) u8. */
BHR_API int32_t bhr_read_gathered_u8(bhr_ctx *ctx, uint8_t *out);

/* ---- multi-GPU row-block tiling, one PROCESS per tile ------------------------------------------------------------
 * The same frame and the same pipelined schedule with every tile in its own process (one rank per GPU under
 * torch.distributed.run, each seeing only its device).  Device buffers cross the process boundary as HIP IPC memory
 * handles, ordering as two counters per rank in host shared memory; no collective, no inter-process event.
 *   1. every rank: bhr_tile_export(ctx, BHR_GATHER_U8 and / or BHR_GATHER_PEER, &mine) -- rank 0 (the tile with row0 = 0)
 *      allocates the frame buffers and exports them with its H-blur planes;
 *   2. the ranks exchange the bhr_tile_handles records (any host channel: gloo all_gather, a file ...) and agree on a
 *      zero-initialised shared-memory area of world * BHR_TILE_SHM_WORDS uint64 words;
 *   3. every rank: bhr_tile_connect(ctx, rank, world, all, shm) -- opens the neighbours' planes and rank 0's buffers;
 *   4. per frame, every rank: bhr_tile_render(ctx, cam, flags) -- returns when EVERY rank's rows have landed;
 *      rank 0 then reads the frame with bhr_read_gathered / bhr_read_gathered_u8.
 * Tiles must be at least R = int(0.02 W) rows high; the lens flare (frame sums) needs bhr_group_render. */
#define BHR_TILE_SHM_WORDS 8
typedef struct {
    uint8_t hblur[64];          /* hipIpcMemHandle_t of the tile's H-blur planes (3, rows + 2R, W) */
    uint8_t gather_f32[64];     /* rank 0: the (H, W, 3) f32 frame buffer */
    uint8_t gather_u8[64];      /* rank 0: the (H, W, 3) u8 frame buffer */
    int32_t row0, rows, device;
    int32_t has_gather_f32, has_gather_u8;
    int32_t reserved[3];
} bhr_tile_handles;
BHR_API int32_t bhr_tile_export(bhr_ctx *ctx, uint32_t gather_flags, bhr_tile_handles *out);
BHR_API int32_t bhr_tile_connect(bhr_ctx *ctx, int32_t rank, int32_t world, const bhr_tile_handles *all, uint64_t *shm);
BHR_API int32_t bhr_tile_render(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags);
/* The frame the last bhr_group_render(..., BHR_GATHER_PEER) gathered on this context's device: (H, W, 3) f32. */
BHR_API int32_t bhr_read_gathered(bhr_ctx *ctx, float *out);

#ifdef __cplusplus
}
#endif
#endif /* BHR_H */
