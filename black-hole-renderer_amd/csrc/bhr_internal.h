// bhr_internal.h -- shared declarations of libbhr_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/bhr.h"
#include "../../include/bhr_disk_v2.h"
#include "../../include/bhr_lifecycle.h"

#define BHR_NUM_MIP_LEVELS 5  // generate_disk_mipmaps(levels=4) => 5 stored levels (render.py:2239-2240)
#define BHR_WAVE 64

// ---- constants of the reference (render.py:37-59) ---------------------------
#define BHR_RS 1.0f
#define BHR_G_FACTOR_CAP 1.5f
#define BHR_G_LUMINOSITY_POWER 1.5f
#define BHR_G_BRIGHTNESS_GAIN 0.38f
#define BHR_DISK_COLOR_TEMPERATURE 6000.0f
#define BHR_DISK_ALPHA_GAIN 6.0f
#define BHR_DISK_RADIAL_BRIGHTNESS_POWER 1.2f
#define BHR_DISK_RADIAL_BRIGHTNESS_MIN 0.2f
#define BHR_DISK_RADIAL_BRIGHTNESS_MAX 8.0f

// Ray-step counters: every wave adds its count with one atomic.  32 400 atomics to ONE address serialise in
// the memory system and put a floor of 0.45 ms under an fhd launch (measured; the fast march spends 0.36 ms);
// a counter is therefore a cell of 128 lanes, 256 bytes apart, indexed by block, summed when read.
// rows of zeros in front of and behind the (3, rows + 2R, W) H-blur planes of the exact-f32 post-pass (the IPC handles of
// csrc/group.hip name the allocation: the planes start this many rows in)
#define BHR_HBLUR_PAD_ROWS 16
// the largest disk value the split-f16 post-pass carries: two f16 halves of x 2^14 (bloom.hip); a written DISK layer with a
// larger one goes through the exact f32 kernels (bhr_write_layer, bhr_bloom)
#define BHR_SPLIT_DISK_MAX 3.99f
#define BHR_SHUTTER_MAX_SAMPLES 64   // samples of a shutter frame (bhr_render_shutter)
#define BHR_STEP_LANES 128
#define BHR_STEP_STRIDE 32          // in u64 words
#define BHR_STEP_CELL (BHR_STEP_LANES * BHR_STEP_STRIDE)

// hybrid march: guard bands around the algorithm's switches; a lane inside one is re-marched strict (march.hip: march_tile_guard_kernel; march_strict_ilp.hip: march_fix_kernel)
#ifndef BHR_LOD_GUARD
#define BHR_LOD_GUARD 1e-2f         // |lod - level boundary|: the fast differentials are good to ~1e-5 in lod at the BASELINE views, but a camera
                                    // 15-50 r_s away behind a long lens carries them through hundreds of steps -- fuzzed 512x320 views flipped
                                    // levels with 2e-3 (3 of 6 gone at 5e-3, all at 1e-2; no measurable cost at 4k: tools/dbg_flipviews.sh)
#endif
#ifndef BHR_R2_GUARD
#define BHR_R2_GUARD 4e-5f          // |r^2 - r_term^2| / r_term^2 of a plane-crossing step (fast positions are good to ~1e-6 relative)
#endif
#ifndef BHR_EDGE_GUARD
#define BHR_EDGE_GUARD 2e-5f        // |hit_r - r_edge| / r_edge at the disk's edges
#endif
#ifndef BHR_F_GUARD
#define BHR_F_GUARD 2e-6f           // |plane function at new_pos| / |new_pos|: a step that ends on the disk plane
#endif
#define BHR_FLUSH_COST 5u            // cost of one wave-wide shading pass in wave-steps (row-cost profile)
#define BHR_VOLUME_OPAQUE 0.9999f   // finite-thickness disk: accumulated opacity at which a ray stops sampling

#define BHR_PI_F 3.14159274101257324f      // (float)pi
#define BHR_TWO_PI_F 6.28318548202514648f  // (float)(2*pi)

// Scene textures as the march kernel sees them.
struct BhrScene {
    const float *skybox;   // (sky_h, sky_w, 3)
    int32_t sky_h, sky_w;
    const float4 *mips;    // packed levels 0..4, level l at mip_off[l], dims (mip_h[l], mip_w[l]); (0, 0) beyond mip_last
    int32_t mip_off[BHR_NUM_MIP_LEVELS];
    int32_t mip_h[BHR_NUM_MIP_LEVELS];
    int32_t mip_w[BHR_NUM_MIP_LEVELS];
    int32_t n_r, n_phi;
    // the last level the texture's mip chain really has (alloc_mips: a chain stops at a side below 2): what _sample_disk_mip
    // clamps the level to (num_mip_levels - 1, render.py:2613).  Read by the anti-aliased kernels only; it sits in what was the
    // struct's tail padding, so every other kernel argument keeps its offset
    int32_t mip_last;
};

// Kernel argument block of the march (passed by value -> SGPRs).
struct BhrMarchArgs {
    float cp[3], cr[3], cu[3], cf[3];
    float pw, ph, r_esc, r_esc2;
    float e1[3], r0, A;      // fast build: e1 = cam/|cam|, r0 = |cam|, A = n.e1 with n = (0, -tan_t, 1)
    float h_base, r_inner, r_outer, t_offset;
    float tilt_rad, tan_t, sin_t, cos_t;
    float aa_strength;
    float max_affine, max_affine_u;   // max_affine_u = max_affine / h_base (fast build)
    int32_t max_iter;
    int32_t width, height;   // full image -- the FINE frame under supersampling (ss > 1), as are row0, rows and the tile grid
    int32_t row0, rows;      // this context's row block
    BhrScene sc;
    float *bg;               // (rows, width, 3)
    float *disk;             // (rows, width, 3)
    _Float16 *diskp;         // non-null: the disk layer once more, cut into f16 halves in the bloom H pass's operand order (bloom.hip: pa)
    int32_t dp_yb, dp_gp, dp_g0;
    float *sum;              // with diskp: bg + disk per value (the V pass's combine reads one plane instead of two)
    unsigned long long *ray_steps;
    unsigned int *queue;     // persistent-wave work counter (zeroed before launch)
    const bhr_disk_v2_params *dv2;   // non-null: analytic Disk V2 source instead of the texture
    double dv2_norm_shear, dv2_norm_hotspot, dv2_t_peak;
    double vol_absorption, vol_grazing_gain, vol_h_max, vol_r_max;   // finite-thickness Disk V2
    int32_t vol_substeps;
    const int32_t *tile_order;   // launch slot -> tile (nullptr: row-major)
    unsigned long long *row_steps;   // BHR_ROW_COSTS: ray-steps per 8-row band (nullptr: not collected)
    unsigned long long *wave_stamps; // diagnostic (env BHR_WAVE_STAMPS): per wave s_memrealtime at start / end, steps, XCC|CU id
    int32_t n_tiles;         // 8x8 pixel tiles in the row block
    int32_t tiles_x;
    int32_t n_list;          // launch slots of this launch (= n_tiles, or the length of a hybrid / row-band sub-list)
    int32_t mip_lds_from;    // BHR_MIP_LDS: mip levels mip_lds_from .. BHR_NUM_MIP_LEVELS - 1 are staged in LDS (march_tile_mipstaged_kernel); -1: none
    unsigned int *fix_count; // hybrid march: pixels the guard kernel handed over to the strict fix kernel
    int32_t *fix_list;
    int32_t fix_cap;
    // supersampling (bhr_set_supersample): k = ss rays per output pixel along x and y, 2^ss_log2; 1 outside the ss kernels
    int32_t ss, ss_log2;
    float ss_inv;            // 1 / k^2
    int32_t out_width, out_rows;   // the output frame's row block: the store pitch and rows of bg / disk / sum
};
// The argument blocks of the march variants' kernels (bhr_march_variant): each the march's block with the variant's own words
// behind it, binary64 on the host rounded once, filled for a launch of that variant alone (march_launch.hip: variant_args).  Blocks
// of their own, because BhrMarchArgs is the whole explicit argument of every other march kernel: one more field in it moves
// their hidden arguments, and with them the code of all of them (tools/code_object_diff.py).
struct BhrKerrMarchArgs : BhrMarchArgs {          // march_kerr.hip
    float kerr_a, kerr_rplus;                     // a = A M in r_s; the horizon radius r_plus = (1 + sqrt(1 - A^2)) / 2 a ray is captured at
};
struct BhrKerrExactMarchArgs : BhrKerrMarchArgs { // ... its exact-redshift kernels (the model ones keep the block above)
    float isco_r, isco_e, isco_l;                 // the ISCO of the disk's sense of rotation: its radius, and the energy -u_t and angular
};                                                // momentum u_phi of its orbit, which the gas inside it keeps (ray_kerr.h: kerr_g_exact)
struct BhrKerrViewMarchArgs : BhrKerrExactMarchArgs {   // march_kerr_observer.hip: the Kerr camera (bhr_render_kerr_view), both redshifts
    float obs_beta[3];                            // the moving camera's velocity,
    float obs_gamma, obs_g2;                      // gamma and gamma^2 / (gamma + 1),
    int32_t obs_sky_shift;                        // whether the sky sample takes the Doppler factor,
    int32_t proj_kind;                            // 0: the pinhole, else BHR_PROJ_*
    float span_h, span_v;                         // and the projection's spans as in BhrProjectedMarchArgs
};
struct BhrObserverMarchArgs : BhrMarchArgs {      // march_observer.hip
    float obs_beta[3];                            // the moving camera's velocity,
    float obs_gamma, obs_g2;                      // gamma and gamma^2 / (gamma + 1),
    int32_t obs_sky_shift;                        // and whether the sky sample takes the Doppler factor
};
struct BhrProjectedMarchArgs : BhrObserverMarchArgs {   // march_projected.hip
    int32_t proj_kind;                            // BHR_PROJ_*
    float span_h, span_v;                         // radians: the equirectangular frame's spans; the fisheye's HALF angle in span_h (ray_projected.h)
};
struct BhrDelayMarchArgs : BhrMarchArgs {         // march_delay.hip
    float delay_scale;                            // ray_delay.h: t_eff = t_offset - delay_scale * T_hit
};

// A partial march launch: the tiles of `d_list` only.  bhr_launch_march_hybrid builds one for each of its launches (strict
// list, fast list, fix list and the empty parts that bracket them) and passes it to bhr_launch_march (null: the whole block).
struct bhr_march_part {
    const int32_t *d_list;   // device list of this launch
    int32_t n;
    int32_t first, last;     // the first part records the start event and clears an untimed counter, the last one records the end event
    int32_t math;            // the arithmetic of this launch: BHR_MATH_FAST or BHR_MATH_STRICT
    int32_t repair;          // 1: the fast object's guard kernel (marks lanes on a discontinuity, appends them to the fix list); 2: the strict fix kernel over that list
    unsigned int *fix_count; // the frame slot's fix list (owned by hybrid.hip), null / 0 without guards
    int32_t *fix_list;
    int32_t fix_cap;
};

// The marches that are not the Schwarzschild pinhole march of a camera at rest: each one object over a ray_*.h (march_device.h)
// with the tile schedule, the texture source, no differentials, and a row of what the host knows of it (bhr_variant_row).
enum bhr_march_variant { BHR_MV_NONE, BHR_MV_KERR, BHR_MV_KERR_EXACT, BHR_MV_OBSERVER, BHR_MV_PROJECTED, BHR_MV_DELAYED, BHR_MV_KERR_VIEW, BHR_MV_KERR_VIEW_EXACT,
                         BHR_MV_COUNT };

// What a frame's entry point (render.hip) asks of the march: the variant and its payload -- a projection comes with an observer
// (at rest if the caller gave none), light delay with neither, none of them with a spin (bhr_variant_frame_check refuses it).
// The Kerr camera's two (BHR_MV_KERR_VIEW, _EXACT: bhr_render_kerr_view) need the spin or the forced Kerr march, come with an
// observer (at rest if the caller gave none) and may come with a projection (null: the pinhole).
struct bhr_variant_request {
    bhr_march_variant variant = BHR_MV_NONE;
    const bhr_observer *observer = nullptr;       // BHR_MV_OBSERVER, BHR_MV_PROJECTED, BHR_MV_KERR_VIEW*: the camera's velocity
    const bhr_projection *projection = nullptr;   // BHR_MV_PROJECTED; BHR_MV_KERR_VIEW*: or null
    const bhr_light_delay *delay = nullptr;       // BHR_MV_DELAYED: the scale
};

// One march call, built by the caller: what bhr_launch_march, bhr_launch_march_hybrid and bhr_launch_adaptive work from.
struct bhr_march_call {
    const bhr_camera *cam;
    uint32_t flags;
    hipStream_t stream;      // the stream of the launch
    int32_t slot;            // timing-ring slot of a bhr_render (its events and counter cell), -1: untimed (the context's scalar ones)
    bool time_untimed;       // an untimed launch records its march-end event too (BHR_GROUP_TIME_MARCH); off, the tile's stream carries no event between march and H pass
    bool defer_end;          // the caller records the march-end event (adaptive frames: the refinement follows the base march)
    int32_t ss;              // supersampling factor of the frame being marched
    bool keep_start;         // a later sample of a shutter frame (bhr_render_shutter): the march-start event stays the first sample's
    bhr_variant_request req;    // the variant whose object marches the frame, resolved by the frame's entry point (none: the rest of this file's marches)
};

// The march kernels by what they do; each march object returns its own instantiation of a name (or null) from
// bhr_march_kernel_fast / _strict / _strict_ilp / _raymap (march.hip, march_strict.hip, march_strict_ilp.hip,
// march_raymap.hip).  diff: the instantiation that integrates the ray differentials.
enum bhr_march_kernel {
    BHR_MK_VOLUME,        // march_tile_kernel<false, 2>: finite-thickness Disk V2 (never differentials)          fast, strict
    BHR_MK_DV2,           // march_tile_kernel<diff, 1>: analytic Disk V2                                        fast, strict
    BHR_MK_PERSISTENT,    // march_persistent_kernel<diff>: waves pull tiles from a queue (BHR_PERSISTENT)       fast, strict
    BHR_MK_TILE,          // strict march_tile_kernel<diff, 0>; fast march_tile_kernel<true, 0> / march_tile_plain_fast
    BHR_MK_TILE_COSTS,    // march_tile_kernel<diff, 0, true>: fills the row-cost profile (BHR_ROW_COSTS)          fast
    BHR_MK_GUARD,         // march_tile_guard_kernel<diff>: the fast list of a hybrid march with guards           fast
    BHR_MK_GUARD_COSTS,   // march_tile_guard_kernel<diff, true>: the same with row costs                         fast
    BHR_MK_MIPSTAGED,     // march_tile_mipstaged_kernel: coarse mip levels in LDS (BHR_MIP_LDS, diff only)       fast
    BHR_MK_TILE_ILP,      // march_tile_aa_ilp / march_tile_plain_ilp: the strict texture march                   strict_ilp
    BHR_MK_FIX,           // march_fix_kernel<diff>: the fix list of a hybrid march                              strict_ilp
    // adaptive supersampling (bhr_set_adaptive_supersample): the kernels of the refinement, whatever the `ss` argument
    BHR_MK_LIST,          // march_list_kernel<diff, 0>: the refined groups of a list of fine tiles, texture       fast, strict_ilp
    BHR_MK_LIST_DV2,      // march_list_kernel<diff, 1>: analytic Disk V2                                        fast, strict
    BHR_MK_LIST_VOLUME,   // march_list_kernel<false, 2>: finite-thickness Disk V2                               fast, strict
    BHR_MK_DETECT,        // adaptive_detect_kernel: lists the output pixels whose neighbours differ             strict
    // the ray map (march_raymap.hip)
    BHR_MK_RAYMAP_BUILD,  // raymap_build_kernel<diff>: marches a view and records what the march finds          raymap
    BHR_MK_RAYMAP_SHADE,  // raymap_shade_kernel<diff, false>: a frame from the records and the current scene    raymap
    BHR_MK_RAYMAP_SHADE_ROT,  // raymap_shade_kernel<diff, true>: the same with the records turned about z       raymap
    BHR_MK_RAYMAP_SHUTTER,      // raymap_shade_shutter_kernel<diff, false>: the mean of n such frames, one launch   raymap
    BHR_MK_RAYMAP_SHUTTER_ROT,  // raymap_shade_shutter_kernel<diff, true>: each sample turned about z by its own angle  raymap
    // the Kerr object's exact-redshift kernels (march_kerr.hip; the model ones are its BHR_MK_TILE)
    BHR_MK_KERR_EXACT,    // march_kerr_exact_kernel / march_kerr_exact_ss_kernel                                   kerr
    // point stars (bhr_set_stars): the shade kernels that add the star plane to the sky sample; no supersampled twins
    BHR_MK_RAYMAP_SHADE_STARS,      // raymap_shade_kernel<diff, false, true>                                     raymap
    BHR_MK_RAYMAP_SHADE_STARS_ROT,  // raymap_shade_kernel<diff, true, true>                                      raymap
    // (ss: BUILD, SHADE and SHADE_ROT have twins for a supersampled map, raymap_build_kernel<DIFF, true> / raymap_shade_ss_kernel; the shutter kernels have none)
    // the Kerr ray map (march_kerr_raymap.hip), each with the model and with the exact redshift; no differentials
    // (ss: BUILD, SHADE, SHADE_ROT and FIX have twins for a supersampled map -- kerr_raymap_build_kernel<RS, KERR_BUILD_SS>,
    // kerr_raymap_shade_ss_kernel<RS, ROT>, kerr_raymap_fix_kernel<RS, true>; the momentum build and the shutter kernels have none)
    BHR_MK_KERR_RAYMAP_BUILD,      // kerr_raymap_build_kernel<RS, KERR_BUILD_PLAIN>: marches a view with the Kerr Ray and records what it finds  kerr_raymap
    BHR_MK_KERR_RAYMAP_SHADE,      // kerr_raymap_shade_kernel<RS, false>: a frame from the records and the current scene          kerr_raymap
    BHR_MK_KERR_RAYMAP_SHADE_ROT,  // kerr_raymap_shade_kernel<RS, true>: the same with the records turned about z                 kerr_raymap
    BHR_MK_KERR_RAYMAP_FIX,        // kerr_raymap_fix_kernel<RS, false>: the map's overflow list, marched with the Kerr Ray        kerr_raymap
    BHR_MK_KERR_RAYMAP_BUILD_MOM,  // kerr_raymap_build_kernel<RS, KERR_BUILD_MOM>: the build that also keeps each crossing's photon momentum  kerr_raymap
    BHR_MK_KERR_RAYMAP_SHUTTER,      // kerr_raymap_shade_shutter_kernel<RS, false>: the mean of n frames from the Kerr map, one launch  kerr_raymap
    BHR_MK_KERR_RAYMAP_SHUTTER_ROT,  // kerr_raymap_shade_shutter_kernel<RS, true>: each sample turned about z by its own angle          kerr_raymap
    // Kerr point stars (bhr_set_kerr_stars): the Kerr shade kernels that add the star plane to the sky sample; no supersampled twins
    BHR_MK_KERR_RAYMAP_SHADE_STARS,      // kerr_raymap_shade_kernel<RS, false, true>                                                    kerr_raymap
    BHR_MK_KERR_RAYMAP_SHADE_STARS_ROT,  // kerr_raymap_shade_kernel<RS, true, true>                                                     kerr_raymap
};

// The row of a march variant (settings.hip: bhr_variant_row_of): its kernels, and the terms and words of its refusals.
struct bhr_variant_row {
    const void *(*kernels)(bhr_march_kernel, int32_t diff, int32_t ss);   // the object's kernel table (diff 0 only) ...
    bhr_march_kernel name;       // ... and the name its frame kernel is asked for under
    const char *noun;            // what a refusal calls the request (a format of the spin: the Kerr rows print it)
    const char *march;           // "the <march> march shades the disk texture", "... has no refinement kernels", "... is Schwarzschild's"
    const char *no_diff;         // why it takes no anti-aliasing
    const char *no_exact;        // why it takes no exact redshift (the Kerr rows: null)
    const char *no_rows;         // why it takes no row-block context
    uint32_t flags_ok;           // the flags of a call it accepts
    bool kerr;                   // the spinning hole's: refuses a tilted disk; the others refuse a spin and the exact redshift
};

// The ray map as its two kernels see it (march_raymap.hip): second kernel argument, behind the march's own block.  Planar: every
// plane is (rows, W) with the pixel index j W + i, so a wave's 8x8 tile reads and writes 32-byte runs of each.  A supersampled
// map (factor k) is the map of the fine frame: (k rows, k W), fine pixel indices; the kernels take k from the march's block.
struct BhrRayMapArgs {
    int32_t *steps;              // executed steps of the pixel's ray
    int32_t *status;             // 0 captured, 1 escaped (samples the sky), 2 ran out of iterations
    float *dir;                  // 3 planes: normalized(escape direction), zeros unless status 1
    int32_t *crossings;          // annulus crossings of the ray, counting past the slots
    float *hits;                 // slots x comps planes, [slot][component]: hit_x, hit_y, to_cam xyz (, dxx, dxy, dyx, dyy)
    unsigned int *over_count;    // pixels with more crossings than slots ...
    int32_t *over_list;          // ... and their indices (the fix kernel's list format)
    unsigned long long *stats;   // [0] crossings stored
    int32_t slots, comps;
    int64_t plane;               // rows W
    float rot_c, rot_s;          // the rotated shade kernel only: cosine and sine of the turn about z (bhr_raymap_render_view)
};

// The map as the STARS shade kernels see it: the map's block with the frame's star plane behind it.  A block of its own for the
// Kerr block's reason: BhrRayMapArgs is an argument of every other map kernel and does not grow.
struct BhrRayMapStarArgs : BhrRayMapArgs {
    const float *stars;          // (rows, W, 3): the star plane S of the frame's view (stars.hip)
};

// The Kerr map as its build under a Kerr polarisation and the Kerr Stokes kernel see it (bhr_set_kerr_polarization): the map's
// block with the momentum planes behind it, for the star block's reason.
struct BhrRayMapMomArgs : BhrRayMapArgs {
    float *mom;                  // slots x 3 planes, [slot][component]: the photon's covariant momentum (p_x, p_y, p_z) at each stored crossing
};

// Third argument of raymap_stokes_kernel (march_polar.hip), behind the march's block of the map's view and the map: the frame's
// polarisation -- wave-uniform, so scalars -- and the three planes it fills.  Also the argument of stokes_cells_kernel.
struct BhrStokesArgs {
    float b[3];                  // the field in the gas frame (b_r, b_phi, b_z), normalized on the host in binary64 and rounded once
    float frac;                  // Pi_0
    float *out;                  // I | Q | U: three planes of rows W floats
    float *cells;                // (gh, gw, 3): the means over cell x cell pixels
    int32_t cell, gw, gh;
    int32_t width, rows;
};

// Third argument of kerr_line_kernel (march_kerr_line.hip), behind the Kerr block of the map's view and the map: the line of the
// frame (bhr_set_kerr_line; include/bhr.h states the model) -- wave-uniform, so scalars -- the device row the histogram goes into
// and, where the frame keeps them, the sample planes.
struct BhrKerrLineArgs {
    unsigned long long *row;     // n_bins sums of Q, then under, over (sums of Q), samples, overflow pixels skipped
    float *g_out, *w_out;        // null, or (slots, rows, W) each: g and w per record, 0 where a record does not count
    float g_min, scale, unit;    // t = (g - g_min) * scale; Q = llrintf(w * unit): both factors rounded once on the host
    float power, index;          // p of g^p, q of (r / r_in)^-q
    float r_in, r_out;           // the line's annulus
    int32_t n_bins;
    int32_t all;                 // BHR_LINE_ALL: every counted record contributes; else the first one of the pixel
};

// Second argument of stars_gather_kernel (stars.hip), behind the march's block of the view (its camera fields and frame shape):
// the map's two planes it reads, the turn of the view, the binned catalogue and the plane it fills.
struct BhrStarsArgs {
    const int32_t *status;       // the map's STATUS plane
    const float *dir;            // ... and its three direction planes
    int64_t plane;               // rows W
    float rot_c, rot_s;          // the turned kernel only: cosine and sine of the view's turn about z
    const float *rec;            // n star records of 6 floats (direction, flux), sorted by bin
    const int32_t *off;          // bins_theta bins_phi + 1 offsets into them
    int32_t bins_theta, bins_phi;
    float cos_span, max_mag;     // cos(max_span) (binary64, rounded once), max_magnification
    float *out;                  // S: (rows, W, 3)
    unsigned int *counts;        // images, capped, skipped_span (cleared ahead of the launch)
};

// The samples of a shutter frame from the map (bhr_raymap_render_shutter): third argument of raymap_shade_shutter_kernel, behind
// the map.  By value: the kernel indexes the table with its wave-uniform loop counter, so t, c and s come out of scalar loads.
struct BhrShutterSample {
    float t, c, s;               // the sample's t_offset; cosine and sine of its turn about z from the build camera (1, 0: none)
    float cp[3];                 // its camera position: the g-factor takes the observer's radius from it (march_device.h: apply_g_factor)
};
struct BhrShutterArgs {
    BhrShutterSample smp[BHR_SHUTTER_MAX_SAMPLES];
    int32_t n;                   // samples, 1 .. BHR_SHUTTER_MAX_SAMPLES
    float inv;                   // 1.0f / (float)n, rounded once on the host
};
static_assert(sizeof(BhrMarchArgs) + sizeof(BhrRayMapArgs) + sizeof(BhrShutterArgs) + 256 < 4096,
              "raymap_shade_shutter_kernel: explicit and hidden kernel arguments stay under 4096 bytes");
static_assert(sizeof(BhrKerrExactMarchArgs) + sizeof(BhrRayMapArgs) + sizeof(BhrShutterArgs) + 256 < 4096,
              "kerr_raymap_shade_shutter_kernel: explicit and hidden kernel arguments stay under 4096 bytes");

// Kernel argument block of adaptive_detect_kernel (march_strict.hip).
struct BhrDetectArgs {
    const float *bg, *disk;      // the k = 1 frame: (height, width, 3)
    int32_t width, height;
    float threshold;             // T: a pixel is refined iff c(p) > T
    int32_t k_log2;
    const uint8_t *flags;        // hybrid: strict flag per 8x8 tile of the FINE frame (null: every tile goes to the first list)
    int32_t fine_tiles_x;
    unsigned char *mask;         // (height, width): 1 = refined
    int32_t *list;               // 2 cap entries: fine tiles that hold a refined pixel; [0, cap) strict (or all), [cap, 2 cap) fast
    int32_t cap;                 // = tiles of the fine frame
    unsigned int *counts;        // [0], [1] tiles in the two lists; [2], [3] refined pixels in them
};

// what a frame's V pass stores (bhr_launch_bloom_v_rows); bhr_ensure_outputs re-runs it for layers nobody asked for up front
#define BHR_OUT_F32 1u    // clip(bg + disk + blur) as f32: what TaichiRenderer.render() returns
#define BHR_OUT_BLUR 2u   // blur_field
#define BHR_OUT_U8 4u     // the frame quantised as save_image does (render.py:423); blue-noise dithered while bhr_set_dither(1)
// internal only (no bhr_set_outputs bit): the 16-bit rows, always made on demand from the f32 frame (quantize.hip)
#define BHR_OUT_U16 8u
// internal only: the HDR plane h of a graded frame that keeps it (grade.hip; bhr_read_layer(BHR_LAYER_HDR)); never asked of bhr_ensure_outputs
#define BHR_OUT_HDR 16u

// The library's environment switches, read ONCE by bhr_create (nothing on the bhr_render path calls getenv).
struct bhr_options {
    int32_t frame_slots;        // BHR_FRAME_SLOTS: frames in flight per context (1 or 2, default 2)
    int32_t bloom_split;        // BHR_BLOOM_SPLIT: -1 by arithmetic (default), 0 exact f32 kernels always, 1 split-f16 always
    int32_t bloom_tiles;        // BHR_BLOOM_TILES: output tiles per wave of the split-f16 post-pass (1..8; 0 = by launch size), A/B runs
    int32_t hybrid_repair;      // BHR_HYBRID_REPAIR: -1 by view (default), 0 / 1 guards + strict fix list off / on
    double hybrid_band[2];      // BHR_HYBRID_BAND="lo,hi": strict band around b_c in r_s (default 0.085, 0.36)
    int32_t hybrid_band_set;
    double hybrid_pad;          // share of its own span of b a small tile is padded by in the strict-band test (BHR_HYBRID_PAD, default 0.5; hybrid.hip: tile_pad)
    int32_t hybrid_streams;     // BHR_HYBRID_STREAMS: 1 both lists of a hybrid march on one stream, 2 on two, -1 (default) 1 where two frame slots overlap frames, else 2
    int32_t calibrate_streams;  // BHR_CALIBRATE_STREAMS: 1 (default) a two-slot context picks slot 1's stream by timing candidates (calibrate.hip)
    int32_t hybrid_classify;    // BHR_HYBRID_CLASSIFY: 1 (default) the tiles are classified and the launch order partitioned on the device, 0 on the host
    int32_t mip_lds;            // BHR_MIP_LDS=1: anti-aliased fast frames stage the coarse mip levels in LDS
    int32_t group_threads;      // BHR_GROUP_THREADS: -1 by device layout (default), 0 / 1 one submitting thread / one per tile
    int32_t group_schedule;     // BHR_GROUP_SCHEDULE: -1 by flags (default), 0 serial, 1 pipelined
    int32_t png16_menu;         // BHR_PNG16_MENU: 1 (default) the 16-bit device PNG codes from its own menu, 0 from the 8-bit one (A/B runs)
    int32_t grade_timing;       // BHR_GRADE_TIMING: 1 a graded frame brackets each launch of its grade stage with HIP events (bhr_debug_read, which = 6); default 0
    int32_t raymap_shutter_fused;   // BHR_RAYMAP_SHUTTER_FUSED: 1 (default) a shutter frame from a map without overflow pixels is one launch, 0 sample by sample (A/B runs, tests)
    int32_t kerr_raymap_shutter_fused;   // BHR_KERR_RAYMAP_SHUTTER_FUSED: the same for a shutter frame from the Kerr map (k = 1, no overflow pixels); default 1
    int32_t shutter_timing;     // BHR_SHUTTER_TIMING: 1 a shutter frame brackets each accumulation launch with HIP events (bhr_debug_read, which = 5); default 0
    int32_t raymap_slots;       // BHR_RAYMAP_SLOTS / option "raymap_slots": crossings a map keeps per pixel (1..8, default 4), read by bhr_raymap_build, which refuses anything else
    int32_t raymap_ss;          // BHR_RAYMAP_SUPERSAMPLE / option "raymap_supersample": the next map's own factor (1, 2, 4, 8; default 1), read by bhr_raymap_build likewise
    int32_t kerr_line_row;      // option "kerr_line_row": the device row the Kerr line pass of the next frame from the Kerr map fills (api_kerr_line.hip); default 0
    int32_t kerr_line_samples;  // option "kerr_line_samples": 1 that pass also stores the per-record g and w planes; default 0
    int32_t kerr_raymap_ss;     // BHR_KERR_RAYMAP_SUPERSAMPLE / option "kerr_raymap_supersample": the next Kerr map's own factor (1, 2, 4, 8; default 1), read by bhr_kerr_raymap_build
};

// The context's ray map (api_raymap.hip): what the strict march of one whole-frame view finds before it shades anything.
// Read-only shared state while frames are in flight, like the scene; allocated at the first build, reused by builds of the
// same shape, released by bhr_raymap_free / bhr_destroy.  A context owns up to two, ctx->raymap and ctx->kerr_raymap, one of each
// kind; everything that builds, reads, shades and frees a map takes the map and asks it what it is.
enum bhr_raymap_kind { BHR_RAYMAP_SCHWARZSCHILD, BHR_RAYMAP_KERR };
struct bhr_raymap {
    BhrRayMapArgs a;             // the device planes
    int32_t kind;                // bhr_raymap_kind: whose rays the records hold; each kind has a star catalogue and a polarisation of its own
    float kerr_spin;             // a Kerr map: the spin and the redshift mode of its build, which a frame from it needs the
    int32_t kerr_redshift;       // context to have still
    int32_t built, diff, slots;
    int32_t ss;                  // the map's own supersampling factor (option "raymap_supersample", a Kerr map's "kerr_raymap_supersample", at the build): planes of the fine frame
    int32_t alloc_slots, alloc_comps, alloc_ss;   // shape of the allocation
    int32_t over_cap;            // capacity of the overflow list: the (fine) pixel count rounded up to whole blocks of the fix kernel
    int64_t device_bytes;
    bhr_camera cam;              // the view it was built for
    uint64_t ray_steps, crossings_stored, overflow_pixels;
    // a Kerr map built while a Kerr polarisation was set: the photon's momentum at each stored crossing, slots x 3 planes of the
    // map's own beside the hits (BhrRayMapMomArgs); has_mom: the last build filled them
    float *mom;
    int32_t has_mom;
};

// A star catalogue of the context (api_stars.hip): read-only shared state while frames are in flight, like the map.  A context
// owns up to two, ctx->stars (bhr_set_stars) and ctx->kerr_stars (bhr_set_kerr_stars), one for each kind of map; everything that
// sets, gathers and frees a catalogue takes the kind (bhr_raymap_kind) and serves that kind's map with that kind's catalogue.
struct bhr_stars {
    int32_t n, bins_theta, bins_phi;
    bhr_star_params params;
    float cos_span;              // cos(max_span_deg), binary64 rounded once
    float *d_rec;                // n x 6
    int32_t *d_off;              // bins + 1
    float *d_plane;              // the build view's plane (rows, W, 3) and, behind it, its gather's three counts
    int32_t plane_valid;         // ... holds the plane of the map and catalogue as they are
    const unsigned int *last_counts;   // the counts of the last gather launched (in d_plane's tail or a frame slot's)
    int64_t device_bytes;
};

// geometry of a context's split-f16 bloom buffers (bloom.hip)
struct bhr_split_geom {
    int32_t NT;            // 16-tap chunks either side of a tile: ceil(R / 16) + 1
    int32_t n_tx, WP;      // 32-pixel tiles along x, W rounded up to them
    int32_t YB, GP, g0;    // pa: 32-row blocks, 8-pixel groups per block (padded), zero groups in front
    int32_t t_first, n_ty; // global 32-row tile of the block's first row, tiles it touches
    int32_t pbr, GR;       // pb: global row of plane row 0 (multiple of 16, may be negative), 8-row groups
    size_t pa_halfs, pb_halfs;
    int32_t table_bytes;
};

// Frame slot: everything one frame in flight owns -- its buffers, its streams and events, how its post-pass ran.  The
// slot is the only home of that state: the launchers reach the active one through bhr_slot(ctx).  bhr_render alternates
// between two slots, each with its own stream, so that the tail and the bloom of frame n run under the march of frame
// n + 1; the scene (skybox, mip stack, comp planes ...) is shared and read-only while frames are in flight (bhr_enter
// orders every other entry point behind them).  Slot 1 is allocated at the second bhr_render; BHR_FRAME_SLOTS=1 keeps one
// slot on the context's own stream (round 1 behaviour, isolated per-kernel timing).
// two is the measured optimum (fhd strict: 1291 fps with one frame in flight, 1452 with two, 1389 / 1400 with three / four)
#define BHR_MAX_FRAME_SLOTS 2
struct bhr_frame_slot {
    hipStream_t stream;
    float *d_bg, *d_disk, *d_blur, *d_final;   // (rows, W, 3) each: rows [row0, row1)
    float *d_hblur;            // planar (3, rows + 2R, W): rows [row0 - R, row1 + R)
    float *d_hblur_base;       // the allocation d_hblur points BHR_HBLUR_PAD_ROWS rows into (zero rows in front of plane 0 and behind plane 2); exact-f32 bloom, on first use
    void *d_pa, *d_pb;         // split-f16 bloom (bloom.hip): the march's packed copy of the disk layer, the packed H-blur planes; on first use
    float *d_sum;              // ... and bg + disk of the frame (rows, W, 3); sum_valid: written by this frame's march / pack kernel
    int32_t sum_valid;
    int32_t disk_wide;         // the DISK layer is a caller's (bhr_write_layer) with a value above BHR_SPLIT_DISK_MAX; a march clears it
    uint8_t *d_final_u8;       // (rows, W, 3)
    uint16_t *d_final_u16;     // (rows, W, 3) 16-bit rows, native endian (bhr_read_final_u16, the 16-bit PNG paths); on first use
    float *d_hdr;              // (rows, W, 3) the HDR plane of a graded frame (grade.hip): h where the frame keeps it, the flare's target; on first use
    uint32_t have;             // BHR_OUT_* layers of the slot's last frame that are in memory (the V pass stores what was asked for; the rest on demand)
    // the post-pass of the slot's frame, set by bhr_frame_begin: frame_split 0 exact f32 kernels (strict), 1 split-f16
    // matrix-core kernels (fast / hybrid); bhr_ensure_outputs re-runs its V pass
    int32_t frame_split, frame_with_bloom;
    unsigned int *d_queue;
    // lens flare scratch of the frame (flare.hip), on first use
    float *d_glow_hw;          // glow rows (rows, W); (H, W) on the context that sums the frame
    int64_t flare_glow_rows;
    float *d_glow_wh;          // (W, H): the reference's memory order, summed the way NumPy sums it
    float *d_flare_c0;         // per 8192-element chunk: sum glow (f32)
    double *d_flare_c12;       // per chunk: sum x glow | sum y glow
    double *d_flare_sums;      // S0, S1, S2
    // adaptive supersampling (march_launch.hip: bhr_launch_adaptive), on first use: two lists of fine tiles, the mask, four counts
    int32_t *d_ada_list;
    unsigned char *d_ada_mask;
    unsigned int *d_ada_counts;
    // shutter frames (shutter.hip), on first use: the running sums of the samples' BG and DISK layers, (rows, W, 3) f32 each
    float *d_acc_bg, *d_acc_disk;
    // point stars (api_stars.hip), on first use: the star plane of a turned view's frame, (rows, W, 3) f32, and behind it its gather's counts
    float *d_star_plane;
    // polarisation (api_polar.hip), on first use: the Stokes planes I | Q | U of the slot's last map frame, rows W floats each, and
    // the grid of their cell means (sized for the smallest cell); stokes_cell: the cell size of that frame, 0: the slot has none
    float *d_stokes, *d_stokes_cells;
    int32_t stokes_cell;
    // second march stream: the strict tiles of a two-stream hybrid march run on it beside the fast ones instead of ahead of
    // them (bhr_aux_fork / _join, which creates the streams of all slots on first use)
    hipStream_t aux_stream;
    hipEvent_t aux_fork, aux_done;
    hipEvent_t done;        // end of the slot's last bhr_render (and of frame work queued behind it: bhr_leave_frame)
    // the last reader of the scene in the slot's last frame (bhr_enter_scene_write): the end of its last march, borrowed from the
    // timing ring -- or, for a map frame with a polarisation set, stokes_done: its Stokes pass samples the disk texture behind the march
    hipEvent_t march_done;
    // the Kerr line pass of the slot's last map frame (api_kerr_line.hip): its sample planes g | w, (slots, rows, W) each, on first
    // use; line_keep: the slots of the frame that filled them (0: the slot has none); line_row: the device row that frame's pass
    // wrote (-1 after a change of the line); line_done: the slot's own event behind the pass, which reads the scene like the Stokes pass
    float *d_line_samples;
    int32_t line_keep, line_alloc, line_row;
    hipEvent_t line_done;
    hipEvent_t stokes_done; // the slot's own, on first use (api_polar.hip): behind the Stokes pass of its last map frame
    int32_t allocated;
    int32_t in_flight;      // rendered since the last join
};

// What bhr_get_counters and bhr_get_row_costs* report about "the last frame": the last frame call that launched everything it
// meant to.  Written whole, in two kinds of place: frame_on_next_slot (render.hip) once a frame's body has returned BHR_OK, and
// the group / tile renders (group.hip: record_tile_frame).  No launcher writes it; a frame that fails leaves the one before.
struct bhr_last_frame {
    int32_t valid;         // a frame has been launched since bhr_create
    int32_t ring;          // its timing-ring slot (events, counter cell: bhr_steps_cell); -1: the context's scalar ones (group / tile renders)
    int32_t march_timed;   // its march-end event was recorded (a group render without BHR_GROUP_TIME_MARCH: not)
    uint32_t flags;
    uint64_t rays;         // launched by the frame's marches: the fine frame's pixels times its shutter samples (an adaptive frame's refinement is added when read)
    int32_t adaptive;      // an adaptively supersampled frame: its refinement's counts are in slot ada_info_slot
};

struct bhr_ctx {
    bhr_config cfg;
    int32_t rows;
    hipStream_t stream;                 // the stream launchers use: the scene stream, or a slot's during bhr_render
    hipStream_t scene_stream;           // scene updates, read-backs, group renders
    bhr_frame_slot slots[BHR_MAX_FRAME_SLOTS];   // the per-frame state; the context keeps no copy of it
    int32_t n_slots, next_slot;
    int32_t active_slot;                // the slot the launchers work on (bhr_slot): always a valid, allocated one (bhr_activate_slot)
    int32_t two_slot_frames, streams_calibrated, calibrating;   // bhr_calibrate_slot_streams (calibrate.hip)
    int32_t calib_choice, calib_fps[8];
    hipStream_t calib_idle[8];
    int32_t n_calib_idle;
    hipEvent_t scene_ev;                // scene stream -> slot stream ordering, recorded at every bhr_render
    hipEvent_t ev[8];
    hipEvent_t sync_ev;                 // bhr_sync polls it (no timing)
    // per-frame timing ring: 3 events per bhr_render (march start, march end, frame end)
    hipEvent_t ring_ev[BHR_TIMING_RING * 3];
    unsigned long long *d_steps_ring;   // one ray-step counter cell (BHR_STEP_CELL words) per ring slot
    unsigned long long *d_steps_fold;   // folded cells (BHR_TIMING_RING words)
    int64_t ring_head;                  // frames recorded since reset

    // scene
    float *d_skybox;
    int32_t sky_h, sky_w;
    float4 *d_mips;
    int32_t n_r, n_phi;
    int32_t mip_off[BHR_NUM_MIP_LEVELS], mip_h[BHR_NUM_MIP_LEVELS], mip_w[BHR_NUM_MIP_LEVELS];
    int64_t mip_texels;

    // texture pipeline
    int32_t bg_ready, bg_n_r, bg_n_phi, az_freq;
    float az_shear;
    float *d_comp;       // (13, n_r, n_phi)
    float *d_edge, *d_omega, *d_row_stats;
    float stats[2];
    float *d_noise_in, *d_noise_out;
    int64_t noise_cap;
    // device lifecycle (lifecycle.hip)
    float *d_pool;             // entity profile pool (bump allocated)
    int64_t pool_used, pool_cap;
    void *d_pairs;             // per-call pair tables
    size_t pairs_cap;
    float *d_stats_scratch;    // density | temp_struct | histogram | row results
    size_t stats_scratch_elems;
    int32_t stats_prepared;
    // analytic disk source
    int32_t disk_source;
    bhr_disk_v2_params *d_dv2_params;
    double dv2_norm[3];        // max|raw shear|, max|raw hotspot| on the reference grid, peak T_mid
    double vol_opts[4];        // absorption Ca, grazing gain kg, max half thickness, max spherical radius of the volume
    int32_t vol_substeps;

    // bloom tables (bloom.hip: bhr_bloom_prepare)
    float *d_wtab;             // bloom weights (3, R + pad)
    float *d_wext;             // unfolded weights (3, 2 R4 + 8)
    unsigned short *d_w16;     // split-f16 weight table: 3 channels x 2 halves x 8 shifted copies (bloom.hip: bloom_tables_kernel)
    int32_t mip_lds_from;      // first mip level the last anti-aliased fast march staged in LDS (BHR_MIP_LDS), -1: none
    int32_t split_ok;          // the context's radius fits the split kernels' table (R <= 176)
    // bhr_set_dither: 1 = the u8 rows are the blue-noise dithered quantisation of the f32 frame (quantize.hip); the frame then
    // takes the route of a flared frame: the V pass keeps f32, the rows are quantised afterwards
    int32_t dither;
    uint16_t *d_dither;        // the 64 x 64 rank matrix on the device, on first use
    // bhr_set_grade: grade_on = 1 while a grade is set; the frames rendered then get FINAL (and their undithered u8 rows) from
    // the grade kernel behind a V pass that stores BLUR only (grade.hip).  gain and iw2 are the host's two derived factors
    int32_t grade_on;
    bhr_grade grade;
    float grade_gain, grade_iw2;
    // option "grade_timing": a start / end event per launch of the last graded frame's grade stage (grade.hip: at most the sum
    // kernel of a flared frame and the grade kernel), on first use
    hipEvent_t grade_ev[4];
    int32_t grade_ev_n;
    uint32_t out_want;         // BHR_OUT_* the frames of this context store (bhr_set_outputs; default: the f32 frame)
    bhr_options opt;           // the BHR_* environment switches, read once by bhr_create
    float *d_wsum_h;           // (3, W) in-bounds weight sums, then (3, W) the split H pass's multiplier 2^-10 / sum
    float *d_wsum_v;           // (3, H), then (3, H) the split V pass's multiplier 2^-24 / sum
    int32_t bloom_R, bloom_ready;
    unsigned long long *d_ray_steps;
    unsigned long long *d_row_steps;   // ray-steps per 8-row band of the last BHR_ROW_COSTS launch
    int32_t *d_tile_order;     // march launch order of the 8x8 tiles
    int32_t *h_tile_order;     // host copy (malloc)
    int32_t tile_order_n, tile_order_ss;   // ... built for this many tiles of the frame marched with this supersampling factor
    int32_t ss;                // bhr_set_supersample: k x k rays per pixel (1, 2, 4, 8)
    // bhr_set_adaptive_supersample: the frame is marched with ss = 1, then the pixels whose neighbours differ by more than
    // ada_threshold are marched again with ada_k x ada_k rays (march_launch.hip: bhr_launch_adaptive).  ada_k = 0: off.
    int32_t ada_k;
    float ada_threshold;
    // bhr_adaptive_info's subject, beside the last-frame record because it outlives it: written with the record of an adaptive
    // frame, kept across frames of other kinds, reset only by a change of the sampling (settings.hip: set_sampling).  (Today
    // every frame of a context with ada_k > 1 is adaptive and the other kinds are refused there, so "kept across" cannot be
    // observed: the two fields behave like fields of the record that set_sampling clears.)
    int32_t ada_info_slot;     // frame slot of the last adaptive frame (-1: none since the setting changed), and
    int32_t ada_info_math;     // the arithmetic bhr_resolve_math gave it
    void *hybrid;              // hybrid.hip: tile classification cache
    void *pipe;                // group.hip: streams, events and band lists of the pipelined row-block path
    uint8_t *d_gather_u8;      // (H, W, 3) u8: quantised frame gathered from the tiles (BHR_GATHER_U8), on tile 0
    int32_t *d_flare_prog;     // lens flare (flare.hip): pairwise tree of the ragged last chunk; shared by the slots, read-only
    float *d_gather;           // (H, W, 3): full frame gathered from the tiles of a group render (BHR_GATHER_PEER), on tile 0
    void *png_dev;             // device PNG encoder state (png_device.hip), created on first use
    void *jpeg_dev;            // device JPEG encoder state (jpeg_device.hip), created on first use
    // option "shutter_timing": a start / end event per accumulation launch of the last shutter frame (shutter.hip), on first use
    hipEvent_t shutter_ev[2 * BHR_SHUTTER_MAX_SAMPLES];
    int32_t shutter_ev_n;      // accumulation launches of the last shutter frame that were bracketed
    void *pop_host;            // pinned staging of bhr_accumulate_population (lifecycle.hip)
    float *h_pinned;           // staging for readbacks
    size_t h_pinned_bytes;

    bhr_counters counters;
    bhr_last_frame last;       // the last frame launched whole; counters.rays / ray_steps / *_ms are filled from it when read

    // the ray map (api_raymap.hip), behind everything the frames of bhr_render touch
    bhr_raymap *raymap;        // null until the first bhr_raymap_build

    // bhr_set_spin: kerr_on = the march is the Kerr object's (a spin other than 0, or force_kerr); kerr_spin = A = a / M
    int32_t kerr_on;
    float kerr_spin;
    int32_t kerr_redshift;     // bhr_set_redshift: BHR_REDSHIFT_MODEL (0) or BHR_REDSHIFT_EXACT, which needs kerr_on
    int32_t kerr_aa;           // bhr_set_kerr_anti_alias: the Kerr march carries ray differentials (needs kerr_on); its strength
    float kerr_aa_strength;

    // the Kerr ray map (api_kerr_raymap.hip): a map object of its own -- nothing of `raymap` above is shared, its stars and polarisation
    // never see it; it carries the spin and the redshift mode it was built under
    bhr_raymap *kerr_raymap;   // null until the first bhr_kerr_raymap_build

    // point stars (api_stars.hip)
    bhr_stars *stars;          // null until a catalogue is set (bhr_set_stars): the Schwarzschild map's
    bhr_stars *kerr_stars;     // null until a catalogue is set (bhr_set_kerr_stars): the Kerr map's

    // polarisation (api_polar.hip): polar_on = a polarisation is set (bhr_set_polarization); stokes_slot = the frame slot that holds
    // the Stokes planes of the last map frame rendered since (-1: none)
    int32_t polar_on;
    bhr_polarization polar;
    int32_t stokes_slot;
    // ... and the Kerr polarisation (bhr_set_kerr_polarization), a setting of its own beside it: the Stokes pass of the frames from
    // the Kerr ray map, into the same slot planes
    int32_t kerr_polar_on;
    bhr_polarization kerr_polar;

    // the Kerr line profile (api_kerr_line.hip): kerr_line_on = a line is set (bhr_set_kerr_line), kerr_line = it with the annulus
    // resolved; d_line_rows = line_rows_n device rows of kerr_line.n_bins + 4 cells; line_slot = the frame slot that holds the
    // sample planes of the last frame that kept them (-1: none)
    int32_t kerr_line_on;
    bhr_kerr_line kerr_line;
    unsigned long long *d_line_rows;
    int32_t line_rows_n;
    int32_t line_slot;

    // the Kerr march's own disk source (bhr_set_kerr_disk_source; api_disk_v2.hip): BHR_DISK_TEXTURE, or a Disk V2 source with a
    // parameter block, norms and bounding slab of its own beside disk_source's above (which stays refused with a spin); absorption,
    // grazing gain and substeps are vol_opts[0], [1] and vol_substeps for both
    int32_t kerr_disk_source;
    bhr_disk_v2_params *d_kerr_dv2_params;
    double kerr_dv2_norm[3];   // max|raw shear|, max|raw hotspot|, peak T_mid
    double kerr_vol_bound[2];  // max half thickness H_max; sqrt(r_out^2 + H_max^2), the largest Kerr-Schild radius of the volume
};

// The active frame slot: the one bhr_activate_slot / bhr_render last pointed the launchers at.
inline bhr_frame_slot &bhr_slot(bhr_ctx *ctx) { return ctx->slots[ctx->active_slot]; }
inline const bhr_frame_slot &bhr_slot(const bhr_ctx *ctx) { return ctx->slots[ctx->active_slot]; }

// The frame the march marches: the context's own, or under supersampling (factor k > 1) the one k times finer along
// both axes, at pixel pitch / k.  The tile grid, the tile order, the hybrid classification and the fix lists live on it.
struct bhr_fine_frame {
    int32_t width, height, row0, rows;
};
inline bhr_fine_frame bhr_fine(const bhr_ctx *ctx, int32_t k) {
    return {ctx->cfg.width * k, ctx->cfg.height * k, ctx->cfg.row0 * k, ctx->rows * k};
}
// k is a power of two: the fine pitch is exact, and the pitch of build_camera(k W, k H) bit for bit
inline bhr_camera bhr_fine_camera(const bhr_camera *cam, int32_t k) {
    bhr_camera c = *cam;
    c.pixel_width /= (float)k;
    c.pixel_height /= (float)k;
    return c;
}
inline int32_t bhr_log2(int32_t k) { return k == 8 ? 3 : k == 4 ? 2 : k == 2 ? 1 : 0; }   // of a supersampling factor (1, 2, 4, 8)

// The march events of a call: timed launches (bhr_render) use their ring slot's, the others the context's scalar ones.
inline hipEvent_t bhr_march_start_event(const bhr_ctx *ctx, int32_t slot) { return slot >= 0 ? ctx->ring_ev[slot * 3 + 0] : ctx->ev[0]; }
inline hipEvent_t bhr_march_end_event(const bhr_ctx *ctx, int32_t slot) { return slot >= 0 ? ctx->ring_ev[slot * 3 + 1] : ctx->ev[1]; }
// ... and the ray-step counter cell they count into: the ring slot's, or the context's scalar one
inline unsigned long long *bhr_steps_cell(const bhr_ctx *ctx, int32_t slot) { return slot >= 0 ? ctx->d_steps_ring + (size_t)slot * BHR_STEP_CELL : ctx->d_ray_steps; }
// anti_alias "disabled": the reference still integrates the differentials (skip_diff = 0 on
// the CLI path) but never reads them (render.py:2957-2959) => skipping them is pixel-identical.
inline bool bhr_want_diff(const bhr_ctx *ctx, uint32_t flags) { return ctx->cfg.anti_alias != 0 && !(flags & BHR_SKIP_DIFFERENTIALS); }
// ... of a march of variant v: the Kerr march's own switch (bhr_set_kerr_anti_alias) for its two variants, else the above
inline bool bhr_want_diff(const bhr_ctx *ctx, uint32_t flags, bhr_march_variant v) {
    return v == BHR_MV_KERR || v == BHR_MV_KERR_EXACT ? ctx->kerr_aa != 0 : bhr_want_diff(ctx, flags);
}

// A row block's packed H-blur planes as a neighbour's split-f16 H pass stores its halo rows into them (bhr_launch_bloom_h;
// group.hip fills the array for the duration of one group / tile render)
#define BHR_MAX_MIRRORS 6
struct bhr_mirror {
    void *pb;
    int32_t pbr, gr;
};

// ================ internal functions, by the source that defines them ================================================================

// ---- context.hip: error plumbing, the context's synchronisation and copies --------------------------------------------------------
int32_t bhr_fail(int32_t code, const char *fmt, ...);
#define BHR_HIP(call)                                                                       \
    do {                                                                                    \
        hipError_t e__ = (call);                                                            \
        if (e__ != hipSuccess)                                                              \
            return bhr_fail(BHR_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                            __FILE__, __LINE__);                                            \
    } while (0)

#define BHR_TRY(expr)                    \
    do {                                 \
        int32_t rc__ = (expr);           \
        if (rc__ != BHR_OK) return rc__; \
    } while (0)

// `count` elements of device memory at *p (null for none, and on failure: BHR_ERR_NOMEM)
template <typename T>
int32_t bhr_dev_alloc(T **p, size_t count) {
    *p = nullptr;
    if (count == 0) return BHR_OK;
    hipError_t e = hipMalloc((void **)p, count * sizeof(T));
    if (e != hipSuccess) {
        *p = nullptr;
        return bhr_fail(BHR_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    }
    return BHR_OK;
}
int32_t bhr_ensure_pinned(bhr_ctx *ctx, size_t bytes);                     // the pinned staging buffer holds at least `bytes`
// caller memory <-> device memory on ctx->stream, which both synchronise (the download through the pinned staging buffer)
int32_t bhr_download(bhr_ctx *ctx, void *dst, const void *d_src, size_t bytes);
int32_t bhr_upload(bhr_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int32_t bhr_poll_sync(bhr_ctx *ctx, hipStream_t stream);                   // waits for `stream`, polling an event for the first 200 ms

// ---- frame_slot.hip: the frame slots, their streams and post-pass -----------------------------------------------------------------
int32_t bhr_alloc_slot(bhr_ctx *ctx, int k);                               // slot k's stream, event and layers, once
void bhr_free_slot(bhr_ctx *ctx, int k);
int32_t bhr_activate_slot(bhr_ctx *ctx, int32_t k);                        // points the launchers at frame slot k (allocating it)
// Every API entry point except bhr_render: selects the device and orders the scene stream behind the frames in
// flight, so that scene writes, read-backs and stand-alone passes see (and never race with) a finished frame.
int32_t bhr_enter(bhr_ctx *ctx);
// Entry points that touch only the component planes / entity pool (comp, d_pool: read by no frame kernel) -- the
// per-frame background and entity-layer passes -- select the scene stream WITHOUT joining the frames in flight, so that
// the next frame's texture work runs beside the current march; bhr_compose_texture (full bhr_enter) is the join.
int32_t bhr_enter_components(bhr_ctx *ctx);
// Work that only reads the last rendered frame (quantise, PNG encode, copy out) rides the stream that rendered it:
// bhr_enter_frame points ctx->stream at that slot's stream (ordered behind the scene stream), bhr_leave_frame
// re-records the slot's completion event and restores the scene stream.  The scene stream stays free meanwhile.
// bhr_compose_texture rewrites the disk texture and its mips, which only the MARCH of a frame in flight reads: the scene
// stream waits for the marches, not for the bloom / flare / PNG work behind them.
int32_t bhr_enter_scene_write(bhr_ctx *ctx);
int32_t bhr_enter_frame(bhr_ctx *ctx);
int32_t bhr_leave_frame(bhr_ctx *ctx);
// fork: the aux stream waits for everything ctx->stream has been given so far; join: ctx->stream waits for the aux stream
int32_t bhr_aux_fork(bhr_ctx *ctx);
int32_t bhr_aux_join(bhr_ctx *ctx);
// decides the frame's arithmetic / post-pass kernels (exact: the exact f32 ones whatever the arithmetic) and makes sure their
// buffers exist (before the march is launched)
int32_t bhr_frame_begin(bhr_ctx *ctx, uint32_t flags, bool exact = false);
// the whole-block V pass of a frame into the context's own buffers, recording what it stored
int32_t bhr_frame_post(bhr_ctx *ctx, int32_t with_bloom, uint32_t want, unsigned long long *zero_cell);
// the lens flare of the active slot's frame from device-resident sums: glow -> sums -> apply (hdr: as bhr_launch_flare_apply)
int32_t bhr_frame_flare(bhr_ctx *ctx, bool hdr);
// makes the BHR_OUT_* layers in `need` of the active slot's last frame exist (re-runs its V pass for what is missing)
int32_t bhr_ensure_outputs(bhr_ctx *ctx, uint32_t need);

// ---- scene.hip ------------------------------------------------------------------------------------------------------------------------
void bhr_free_scene(bhr_ctx *ctx);                                         // the mip stack
void bhr_free_bg(bhr_ctx *ctx);                                            // the background layer's planes

// ---- calibrate.hip ----------------------------------------------------------------------------------------------------------------------
int32_t bhr_streams_share_queue(hipStream_t a, hipStream_t b, int32_t *share);   // probe (two one-lane kernels, <= 4 ms)
// picks slot 1's stream by timing candidates on frames of (cam, flags) through bhr_render; once per two-slot context
int32_t bhr_calibrate_slot_streams(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags);

// ---- settings.hip: the march variants' table and their refusals -----------------------------------------------------------------------
const bhr_variant_row &bhr_variant_row_of(bhr_march_variant v);   // the table
// the variant of a frame: what its entry point asks for, else what the context is set to (a spin, the exact redshift) -- the
// one place that reads kerr_on for it; everything else switches on the result
bhr_march_variant bhr_variant_of(const bhr_ctx *ctx, bhr_march_variant asked = BHR_MV_NONE);
int32_t bhr_note_frame_kernel(bhr_ctx *ctx);                               // its registers / LDS into the counters (bhr_create, bhr_set_spin, bhr_set_redshift, bhr_set_kerr_anti_alias)
// what a frame of variant v does not combine with: BHR_ERR_INVALID naming it -- `flags` of the call, the context's state (tilt,
// anti-aliasing, Disk V2, adaptive supersampling, spin and redshift, row block).  spin: a / M as printed (bhr_set_spin: the candidate)
int32_t bhr_variant_frame_check(const bhr_ctx *ctx, bhr_march_variant v, uint32_t flags, const char *who, double spin);
// a call that has no Kerr form at all (ray maps, shutter frames, group and tile renders): BHR_ERR_INVALID with a spin set
int32_t bhr_kerr_refuse(const bhr_ctx *ctx, const char *who, const char *what);
// a camera inside the static limit: BHR_ERR_INVALID, before anything is launched
int32_t bhr_kerr_camera_check(const bhr_ctx *ctx, const bhr_camera *cam, const char *who);
// a call that has no form over the Kerr march's Disk V2 source (bhr_set_kerr_disk_source): BHR_ERR_INVALID while one is set
int32_t bhr_kerr_disk_refuse(const bhr_ctx *ctx, const char *who, const char *what);

// ---- counters.hip -------------------------------------------------------------------------------------------------------------------
float bhr_ev_ms(hipEvent_t a, hipEvent_t b);                               // milliseconds between two recorded events, -1 where there are none
// sum of the lanes of each of `n` counter cells -> host_out[n], on ctx->stream (synchronises)
int32_t bhr_fold_cells(bhr_ctx *ctx, const unsigned long long *cells, int n, unsigned long long *host_out);

// ---- march_launch.hip and the march objects (each table lives next to its kernels) ----------------------------------------------------
int32_t bhr_resolve_math(const bhr_ctx *ctx, uint32_t flags);                          // BHR_MATH_* of a frame
int32_t bhr_launch_march(bhr_ctx *ctx, const bhr_march_call &call, const bhr_march_part *part = nullptr);   // every march launch
// {VGPRs, LDS, scratch bytes} of the kernel that marches a whole texture frame: variant v's, or without one the arithmetic's
int32_t bhr_march_resources(const char *who, bhr_march_variant v, int32_t math, int32_t diff, int32_t ss, int32_t out[3]);
int32_t bhr_ensure_tile_order(bhr_ctx *ctx, int32_t ss);                               // builds d_/h_tile_order of the frame marched with factor ss
// detect + refinement (ctx->ada_k) of an adaptively supersampled frame, behind its base march `call` on the same stream; records the march-end event
int32_t bhr_launch_adaptive(bhr_ctx *ctx, const bhr_march_call &call);
// the ray map's launches on ctx->stream.  build: marches `cam` and fills the map (counting its steps into a cell of the map's
// own); shade: the map's pixels under the scene as it is and cam's t_offset into the active slot's
// layers -- the pixels on the overflow list are left to the fix kernel (bhr_launch_march with a repair == 2 part over that list)
// ss: the map's factor -- the build marches the fine frame bhr_fine(ctx, ss) of `cam`
// v, call.req.variant: none takes march_raymap.hip's kernels under the march's block, BHR_MV_KERR / BHR_MV_KERR_EXACT
// march_kerr_raymap.hip's under the Kerr block (one ray per pixel, 5 components)
// mom: a Kerr build's momentum planes (kerr_raymap_build_kernel<RS, KERR_BUILD_MOM> fills them beside the records); null: the plain build
int32_t bhr_launch_raymap_build(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags, const BhrRayMapArgs &m, int32_t ss, bhr_march_variant v = BHR_MV_NONE,
                                float *mom = nullptr);
// rot_c, rot_s: the stored records turned about z by that cosine and sine before they are shaded (1, 0: the kernel without a turn)
// stars: the star plane of the frame's view (bhr_set_stars, a Kerr map's bhr_set_kerr_stars), added to the sky sample by the STARS kernels; null: the kernels without
int32_t bhr_launch_raymap_shade(bhr_ctx *ctx, const bhr_march_call &call, const BhrRayMapArgs &m, bool diff, float rot_c = 1.0f, float rot_s = 0.0f,
                                const float *stars = nullptr);
// the star plane of the map `m` under the catalogue `st`, seen from `cam`, the build camera turned by (rot_c, rot_s), into `out`
// (rows W 3 floats and three counts behind them, which the launch clears first) on `stream` (stars.hip: stars_gather_kernel).
// The kernel reads the view's camera and the frame's shape out of the march's block -- the part a Kerr block begins with -- and
// the map's status and direction planes, which both kinds of map store alike: either kind's map, with either catalogue.
int32_t bhr_launch_stars_gather(bhr_ctx *ctx, const bhr_stars *st, const bhr_camera *cam, const BhrRayMapArgs &m, float rot_c, float rot_s, float *out, hipStream_t stream);
const void *bhr_stars_kernel(int32_t rot);                                             // stars.hip -> stars.o
// all samples of a shutter frame from the map in one launch (raymap_shade_shutter_kernel): the mean of the n frames the launch
// above would store for (smp[j].t, smp[j].c, smp[j].s), into the active slot's BG / DISK; no packed bloom operands.  Opens the
// frame's march bracket; the caller closes it.  turned: some sample has a turn other than (1, 0).  Under call's Kerr variant the
// map is the Kerr map and the kernel kerr_raymap_shade_shutter_kernel<RS, turned> under the Kerr block (diff: false).
int32_t bhr_launch_raymap_shade_shutter(bhr_ctx *ctx, const bhr_march_call &call, const BhrRayMapArgs &m, bool diff, const BhrShutterArgs &smp, bool turned);
const void *bhr_march_kernel_fast(bhr_march_kernel k, int32_t diff, int32_t ss);       // march.hip -> march.o (ss: the supersampled twin)
const void *bhr_march_kernel_strict(bhr_march_kernel k, int32_t diff, int32_t ss);     // march_strict.hip -> march_strict.o
const void *bhr_march_kernel_strict_ilp(bhr_march_kernel k, int32_t diff, int32_t ss); // march_strict_ilp.hip -> march_strict_ilp.o
const void *bhr_march_kernel_raymap(bhr_march_kernel k, int32_t diff, int32_t ss);     // march_raymap.hip -> march_raymap.o
const void *bhr_march_kernel_observer(bhr_march_kernel k, int32_t diff, int32_t ss);   // march_observer.hip -> march_observer.o (BHR_MK_TILE, diff 0 only)
const void *bhr_march_kernel_projected(bhr_march_kernel k, int32_t diff, int32_t ss);  // march_projected.hip -> march_projected.o (BHR_MK_TILE, diff 0 only)
const void *bhr_march_kernel_delay(bhr_march_kernel k, int32_t diff, int32_t ss);      // march_delay.hip -> march_delay.o (BHR_MK_TILE, diff 0 only)
const void *bhr_march_kernel_kerr(bhr_march_kernel k, int32_t diff, int32_t ss);       // march_kerr.hip -> march_kerr.o (BHR_MK_TILE or BHR_MK_KERR_EXACT; diff: the Ray with differentials, bhr_set_kerr_anti_alias)
const void *bhr_march_kernel_kerr_dv2(bhr_march_kernel k, int32_t diff, int32_t ss);   // march_kerr_dv2.hip -> march_kerr_dv2.o (BHR_MK_DV2, BHR_MK_KERR_EXACT: the Disk V2 surface, model / exact; BHR_MK_VOLUME; diff 0 only)
// the kernel that marches a Kerr frame over the Kerr disk source `source` (not the texture) under redshift `mode`; null: none
const void *bhr_kerr_dv2_kernel(int32_t source, int32_t mode, int32_t ss);
const void *bhr_march_kernel_kerr_view(bhr_march_kernel k, int32_t diff, int32_t ss);  // march_kerr_observer.hip -> march_kerr_observer.o (as bhr_march_kernel_kerr)
const void *bhr_march_kernel_kerr_raymap(bhr_march_kernel k, int32_t exact, int32_t ss);   // march_kerr_raymap.hip -> march_kerr_raymap.o (exact: the exact redshift's; ss: a supersampled map's)
int32_t bhr_selftest_strict(bhr_ctx *ctx, unsigned long long *d_out4);                 // march_strict.hip -> march_strict.o

// ---- hybrid.hip -------------------------------------------------------------------------------------------------------------------------
int32_t bhr_launch_march_hybrid(bhr_ctx *ctx, const bhr_march_call &call);
// strict flag per 8x8 tile of the frame k times finer than the context's (the rule a bhr_set_supersample(k) hybrid
// frame classifies its tiles by), in a buffer of the active frame slot, made on ctx->stream and cached on the view key
int32_t bhr_hybrid_fine_flags(bhr_ctx *ctx, const bhr_camera *cam, int32_t k, const uint8_t **d_flags, int32_t *tiles_x);
void bhr_hybrid_free(bhr_ctx *ctx);
int32_t bhr_hybrid_active_list(bhr_ctx *ctx, const int32_t **list, int32_t *n);   // the active slot's partitioned launch order (tests)

// ---- bloom.hip ------------------------------------------------------------------------------------------------------------------------
int32_t bhr_bloom_prepare(bhr_ctx *ctx);
int32_t bhr_split_nt(int32_t R);
void bhr_split_geometry(const bhr_ctx *ctx, bhr_split_geom *g);
int32_t bhr_launch_bloom_pack(bhr_ctx *ctx);                               // d_disk -> d_pa
// H pass; split frames: also into the n_mirrors planes of neighbouring row blocks that need rows of this one for their V pass
int32_t bhr_launch_bloom_h(bhr_ctx *ctx, const bhr_mirror *mirrors, int32_t n_mirrors);
// V pass + combine over local rows [r0, r1) storing the BHR_OUT_* layers in `want`; gather_u8 / gather_f32 non-null: the
// u8 / f32 rows go into that (H, W, 3) frame buffer (a row-block gather, possibly on a peer device) instead of the context's own;
// zero_cell non-null: the ray-step counter cell the launch clears (bhr_render: a ring slot ahead)
int32_t bhr_launch_bloom_v_rows(bhr_ctx *ctx, int32_t with_bloom, int32_t r0, int32_t r1, uint32_t want, uint8_t *gather_u8, float *gather_f32,
                                unsigned long long *zero_cell);
int32_t bhr_bloom_v_tile_rows(bhr_ctx *ctx);                               // output rows per V-pass block

// ---- group.hip --------------------------------------------------------------------------------------------------------------------------
void bhr_pipe_free(bhr_ctx *ctx);

// ---- flare.hip ------------------------------------------------------------------------------------------------------------------------
int32_t bhr_launch_flare_glow(bhr_ctx *ctx, bool whole_frame);
int32_t bhr_launch_flare_sums(bhr_ctx *ctx);
// sums == nullptr: device-resident totals; hdr: onto the slot's HDR plane without the upper clip (a graded frame) instead of FINAL
int32_t bhr_launch_flare_apply(bhr_ctx *ctx, const double *sums, bool hdr = false);

// ---- png_device.hip, jpeg_device.hip ------------------------------------------------------------------------------------------------------
// (rows, W, 3) u8 at d_rgb -> PNG file bytes at d_out on ctx->stream; d_meta (4 words) = {length, error, ..}
int32_t bhr_launch_png_encode(bhr_ctx *ctx, const uint8_t *d_rgb, uint8_t *d_out, int64_t cap, uint32_t *d_meta);
// the same for the (rows, W, 3) u16 rows at d_rgb16 (native endian): a 16-bit PNG, samples big-endian in the file
int32_t bhr_launch_png16_encode(bhr_ctx *ctx, const uint16_t *d_rgb16, uint8_t *d_out, int64_t cap, uint32_t *d_meta);
void bhr_png_dev_free(bhr_ctx *ctx);
// (rows, W, 3) u8 at d_rgb -> JFIF file bytes at d_out on ctx->stream; d_meta (4 words) = {length, error, ..}
int32_t bhr_launch_jpeg_encode(bhr_ctx *ctx, int32_t quality, const uint8_t *d_rgb, uint8_t *d_out, int64_t cap, uint32_t *d_meta);
void bhr_jpeg_dev_free(bhr_ctx *ctx);

// ---- quantize.hip: the two quantisers that read the f32 FINAL frame, on ctx->stream (bhr_ensure_outputs calls them) ------------------
int32_t bhr_launch_quantize_u16(bhr_ctx *ctx);      // d_final -> d_final_u16 (allocated here on first use)
int32_t bhr_launch_quantize_dither(bhr_ctx *ctx);   // d_final -> d_final_u8, blue-noise dithered

// ---- grade.hip, on ctx->stream ------------------------------------------------------------------------------------------------------------
// FINAL of the active slot under the context's grade, from its BG / DISK / BLUR layers or (from_hdr)
// from its HDR plane, which is then clamped in place; store_hdr: also the plane h; store_u8: also the undithered u8 rows
int32_t bhr_launch_grade(bhr_ctx *ctx, bool from_hdr, bool store_hdr, bool store_u8);
int32_t bhr_launch_grade_sum(bhr_ctx *ctx);         // (d_bg + d_disk) + d_blur -> d_hdr (allocated here on first use)
void bhr_grade_free(bhr_ctx *ctx);                  // the timing events

// ---- hdr_stream.hip, on ctx->stream ---------------------------------------------------------------------------------------------------
// the active slot's HDR plane -> planar u16 Y | Cb | Cr (3 W rows bytes) at d_out under
// `transfer` (BHR_HDR_PQ / _HLG), and the frame's light levels into d_levels = {u32 bits of the largest f32 nits, u32 0, f64 sum
// of nits}, 16 bytes on an 8-byte boundary that the launch clears first (HLG leaves them 0).  scale: white_nits / 10000 (PQ)
int32_t bhr_launch_hdr_yuv420p10(bhr_ctx *ctx, int32_t transfer, float gain, float scale, float white_nits, uint16_t *d_out, void *d_levels);

// ---- shutter.hip ----------------------------------------------------------------------------------------------------------------------
// sample j of the n > 1 samples of a shutter frame has been marched into the active slot's d_bg / d_disk; on
// ctx->stream: j = 0 starts the slot's running sums with it, 0 < j < n - 1 adds it, j = n - 1 adds it and stores the mean
// (sum * (1.0f / n)) back into d_bg / d_disk.  The sums are allocated here on first use.
int32_t bhr_launch_shutter_accumulate(bhr_ctx *ctx, int32_t j, int32_t n);
void bhr_shutter_free(bhr_ctx *ctx);                                 // the timing events

// ---- api_raymap.hip -------------------------------------------------------------------------------------------------------------------
// the refusals of bhr_raymap_render (nothing launched)
int32_t bhr_raymap_check_render(bhr_ctx *ctx, float t_offset, uint32_t flags);
// ... and of bhr_raymap_render_view, which also gives the cosine and sine of cam's turn from the build camera (binary64, rounded once)
int32_t bhr_raymap_check_render_view(bhr_ctx *ctx, const bhr_camera *cam, uint32_t flags, float *rot_c, float *rot_s);
// ... and of bhr_raymap_render_shutter, which fills smp (t, c, s per sample, n, 1 / n) and tells whether any sample is turned
int32_t bhr_raymap_check_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags, BhrShutterArgs *smp, bool *turned);
// What both maps of a context share, each taking the map or the context's pointer to it (&ctx->raymap or &ctx->kerr_raymap) and
// the public call `who` that a refusal names.
// The tail of a build, behind the entry point's own refusals: enters behind the frames in flight, creates the map or re-allocates
// it on a shape change, clears it, marches `cam` into it (bhr_launch_raymap_build under `flags` and variant `v`, which also says
// the map's kind) and fills its fields.  K: slots per pixel; ss: the map's own factor.
int32_t bhr_raymap_build_into(bhr_ctx *ctx, bhr_raymap **map, const char *who, const bhr_camera *cam, uint32_t flags, bhr_march_variant v, int32_t K, int32_t ss);
// one plane of a built map (BHR_RAYMAP_STEPS .. _HITS) to the host, [pixel][component]
int32_t bhr_raymap_read_plane(bhr_ctx *ctx, const bhr_raymap *rm, const char *who, int32_t which, void *out, int64_t bytes);
int32_t bhr_raymap_free_map(bhr_ctx *ctx, bhr_raymap **map);                    // behind every stream that may still read it
void bhr_raymap_release(bhr_ctx *ctx, bhr_raymap **map);                        // ... without waiting (bhr_destroy)
// the fields the two info structs of include/bhr.h share, `out` zeroed first; false: no built map, nothing more to say
template <class Info>
bool bhr_raymap_fill_info(const bhr_ctx *ctx, const bhr_raymap *rm, Info *out) {
    memset(out, 0, sizeof(*out));
    if (!rm) return false;
    out->built = rm->built;
    out->device_bytes = rm->device_bytes;
    if (!rm->built) return false;
    out->slots = rm->slots;
    out->width = ctx->cfg.width;
    out->rows = ctx->rows;
    out->crossings_stored = (int64_t)rm->crossings_stored;
    out->overflow_pixels = (int64_t)rm->overflow_pixels;
    out->ray_steps = rm->ray_steps;
    out->cam = rm->cam;
    return true;
}
// is `cam` the build camera `b` turned rigidly about z?  Gives the turn's cosine and sine (binary64, rounded once)
int32_t bhr_raymap_turn_of_build(const bhr_camera &b, const bhr_camera *cam, const char *who, float *rot_c, float *rot_s);

// ---- api_kerr_raymap.hip ------------------------------------------------------------------------------------------------------------------
// the refusals of bhr_kerr_raymap_render and bhr_kerr_raymap_render_view (nothing launched); cam null: the build camera, no turn
int32_t bhr_kerr_raymap_check_render(bhr_ctx *ctx, const char *who, const bhr_camera *cam, float t_offset, uint32_t flags, float *rot_c, float *rot_s);
// ... and of bhr_kerr_raymap_render_shutter, which fills smp and tells whether any sample is turned (as bhr_raymap_check_render_shutter)
int32_t bhr_kerr_raymap_check_render_shutter(bhr_ctx *ctx, const bhr_camera *cams, int32_t n, uint32_t flags, BhrShutterArgs *smp, bool *turned);

// ---- api_stars.hip ----------------------------------------------------------------------------------------------------------------------
// kind (bhr_raymap_kind): whose catalogue -- the Schwarzschild map's (bhr_set_stars) or the Kerr map's (bhr_set_kerr_stars); a
// catalogue serves the map of its own kind and no other
inline bhr_stars *&bhr_stars_of(bhr_ctx *ctx, int32_t kind) { return kind == BHR_RAYMAP_KERR ? ctx->kerr_stars : ctx->stars; }
inline const bhr_stars *bhr_stars_of(const bhr_ctx *ctx, int32_t kind) { return kind == BHR_RAYMAP_KERR ? ctx->kerr_stars : ctx->stars; }
inline const bhr_raymap *bhr_stars_map(const bhr_ctx *ctx, int32_t kind) { return kind == BHR_RAYMAP_KERR ? ctx->kerr_raymap : ctx->raymap; }
inline bool bhr_have_stars(const bhr_ctx *ctx, int32_t kind = BHR_RAYMAP_SCHWARZSCHILD) {
    const bhr_stars *st = bhr_stars_of(ctx, kind);
    return st && st->n > 0;
}
size_t bhr_star_plane_floats(const bhr_ctx *ctx);                          // rows W 3 and the counts' words behind them
// the build view's plane exists and is current (gathers it on the scene stream, behind the frames in flight, if not)
int32_t bhr_stars_ensure_plane(bhr_ctx *ctx, int32_t kind = BHR_RAYMAP_SCHWARZSCHILD);
// the star plane of the active slot's frame from the map turned by (c, s) on ctx->stream: the cached one for no turn, else gathered into the slot's own
int32_t bhr_stars_frame_plane(bhr_ctx *ctx, int32_t kind, const bhr_camera *cam, float c, float s, const float **plane);
void bhr_stars_invalidate(bhr_ctx *ctx, int32_t kind);                     // the kind's map changed: the cached plane is stale
// what the entry points of the kind's (built) map refuse while its catalogue is set, BHR_ERR_STATE naming the stars: a render or a
// plane read from a supersampled map; a shutter frame
int32_t bhr_stars_check_map(const bhr_ctx *ctx, int32_t kind, const char *who);
int32_t bhr_stars_check_shutter(const bhr_ctx *ctx, int32_t kind, const char *who);
// BHR_RAYMAP_STARS of the kind's (built) map for `who` (bhr_raymap_read, bhr_kerr_raymap_read): the build view's plane, gathered now if stale
int32_t bhr_stars_read_plane(bhr_ctx *ctx, int32_t kind, const char *who, void *out, int64_t bytes);
void bhr_stars_release(bhr_ctx *ctx, int32_t kind);

// ---- api_polar.hip, march_polar.hip -----------------------------------------------------------------------------------------------------
inline bool bhr_have_polar(const bhr_ctx *ctx) { return ctx->polar_on != 0; }
// the Stokes pass of the active slot's map frame on ctx->stream, behind its shade launch: the planes and the cell grid into the
// slot's own storage (allocated here on first use); records the slot's stokes_done behind it and makes it the slot's march_done
int32_t bhr_polar_frame(bhr_ctx *ctx, const bhr_march_call &call, const bhr_raymap &rm);
void bhr_polar_invalidate(bhr_ctx *ctx);                                   // the map or the setting changed: no frame's planes to read
// march_launch.hip: the two launches of that pass under the march's block of call's view -- or, under call's Kerr variant, the
// Kerr Stokes kernel under the Kerr block over the Kerr map's momentum planes `mom` (diff: false), and the same cell means
int32_t bhr_launch_stokes(bhr_ctx *ctx, const bhr_march_call &call, const BhrRayMapArgs &m, bool diff, float *mom, const BhrStokesArgs &s);
const void *bhr_stokes_kernel(int32_t diff);                               // march_polar.hip -> march_polar.o
const void *bhr_stokes_cells_kernel(void);
// the Kerr polarisation (bhr_set_kerr_polarization): the same pass for a frame from the Kerr ray map `rm`, which has to hold the
// momentum planes; the kernel is march_kerr_polar.hip's under the Kerr block of call's variant, the cell means the kernel above
inline bool bhr_have_kerr_polar(const bhr_ctx *ctx) { return ctx->kerr_polar_on != 0; }
int32_t bhr_kerr_polar_frame(bhr_ctx *ctx, const bhr_march_call &call, const bhr_raymap &rm);
const void *bhr_kerr_stokes_kernel(int32_t exact);                         // march_kerr_polar.hip -> march_kerr_polar.o
// the Kerr line profile (bhr_set_kerr_line; api_kerr_line.hip): the pass of a frame from the k = 1 Kerr map `rm` on frame slot k
// into the row of option "kerr_line_row", behind the frame's shade and Stokes pass; what a render and a build are refused for
// while a line is set; the sample planes of the last frame that kept them; the state's release
inline bool bhr_have_kerr_line(const bhr_ctx *ctx) { return ctx->kerr_line_on != 0; }
inline int32_t bhr_kerr_line_cells(const bhr_ctx *ctx) { return ctx->kerr_line.n_bins + 4; }
int32_t bhr_kerr_line_frame(bhr_ctx *ctx, const bhr_march_call &call, const bhr_raymap &rm, int k);
int32_t bhr_kerr_line_check_render(const bhr_ctx *ctx, const bhr_raymap *rm, const char *who, bool turned, bool shutter);
int32_t bhr_kerr_line_read_samples(bhr_ctx *ctx, const char *who, int32_t which, void *out, int64_t bytes);
void bhr_kerr_line_invalidate(bhr_ctx *ctx);
void bhr_kerr_line_release(bhr_ctx *ctx);
// its launch (march_launch.hip): the kernel of call's Kerr variant and of the emissivity over the shade kernel's tiles, a
// capped grid of workgroups that stride over them, (n_bins + 4) cells of dynamic LDS
int32_t bhr_launch_kerr_line(bhr_ctx *ctx, const bhr_march_call &call, const BhrRayMapArgs &m, const BhrKerrLineArgs &s, bool texture);
const void *bhr_kerr_line_kernel(int32_t exact, int32_t texture);           // march_kerr_line.hip -> march_kerr_line.o

// ---- lifecycle.hip, texture.hip, disk_v2.hip ------------------------------------------------------------------------------------------
void bhr_population_free(bhr_ctx *ctx);
int32_t bhr_launch_build_mips(bhr_ctx *ctx);
int32_t bhr_launch_background(bhr_ctx *ctx, float t);
int32_t bhr_launch_compose(bhr_ctx *ctx, float t_offset, int32_t enable_rt, float color_temp);
int32_t bhr_launch_fill(bhr_ctx *ctx, float *dst, int64_t n, float v);
int32_t bhr_launch_noise(bhr_ctx *ctx, int64_t n, int32_t mode, int32_t octaves, float pers, float lac);
int32_t bhr_launch_disk_v2(bhr_ctx *ctx, const bhr_disk_v2_params *p, const double *d_r, const double *d_z,
                           const double *d_phi, int64_t n, int32_t field, double *d_out, double *d_aux,
                           double *d_maxabs, double norm0, double norm1);
