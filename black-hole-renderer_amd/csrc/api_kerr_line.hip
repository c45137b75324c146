// api_kerr_line.hip -- the Kerr line profile's entry points (include/bhr.h): bhr_set_kerr_line, bhr_kerr_line_reserve,
// bhr_kerr_line_read, bhr_kerr_line_info, bhr_kerr_line_resources, and what a frame from the Kerr ray map asks of it (the pass into
// a device row, its refusals, the sample planes).  The kernel is march_kerr_line.hip's, its launcher march_launch.hip's; the frame
// itself is launched from render.hip.  The device rows are the context's (a video fills one per frame and reads them once at
// the end); the sample planes are the frame slot's own, like the Stokes planes.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "bhr_internal.h"

namespace {

const int32_t kMaxRows = 65536;
const int32_t kDefaultRows = BHR_MAX_FRAME_SLOTS;

// every stream that may still write a row or a slot's planes
int32_t drain(bhr_ctx *ctx) {
    for (auto &f : ctx->slots) {
        if (f.stream) BHR_HIP(hipStreamSynchronize(f.stream));
        if (f.aux_stream) BHR_HIP(hipStreamSynchronize(f.aux_stream));
    }
    BHR_HIP(hipStreamSynchronize(ctx->scene_stream));
    return BHR_OK;
}

size_t plane_floats(const bhr_ctx *ctx) { return (size_t)ctx->rows * ctx->cfg.width; }

void free_rows(bhr_ctx *ctx) {
    if (ctx->d_line_rows) (void)hipFree(ctx->d_line_rows);
    ctx->d_line_rows = nullptr;
    ctx->line_rows_n = 0;
}

// n zeroed rows of the line as it is set; the caller has drained the streams
int32_t alloc_rows(bhr_ctx *ctx, int32_t n) {
    free_rows(ctx);
    const size_t cells = (size_t)n * bhr_kerr_line_cells(ctx);
    BHR_TRY(bhr_dev_alloc(&ctx->d_line_rows, cells));
    BHR_HIP(hipMemsetAsync(ctx->d_line_rows, 0, cells * sizeof(unsigned long long), ctx->scene_stream));
    BHR_HIP(hipStreamSynchronize(ctx->scene_stream));
    ctx->line_rows_n = n;
    return BHR_OK;
}

int32_t check_struct(const bhr_ctx *ctx, const char *who, const bhr_kerr_line *p, bhr_kerr_line *out) {
    if (p->n_bins < 1 || p->n_bins > BHR_LINE_MAX_BINS) return bhr_fail(BHR_ERR_INVALID, "%s: n_bins %d (1 .. %d)", who, p->n_bins, BHR_LINE_MAX_BINS);
    if (!(isfinite(p->g_min) && isfinite(p->g_max) && p->g_min < p->g_max))
        return bhr_fail(BHR_ERR_INVALID, "%s: range g_min %g, g_max %g: finite, g_min < g_max", who, (double)p->g_min, (double)p->g_max);
    const double scale = (double)p->n_bins / ((double)p->g_max - (double)p->g_min);
    if (!isfinite((float)scale)) return bhr_fail(BHR_ERR_INVALID, "%s: range g_min %g, g_max %g: too narrow for %d bins in f32", who, (double)p->g_min, (double)p->g_max, p->n_bins);
    if (!(p->power >= 0.0f && p->power <= 8.0f)) return bhr_fail(BHR_ERR_INVALID, "%s: power %g: in [0, 8] and no NaN", who, (double)p->power);
    if (!(p->index >= 0.0f && p->index <= 16.0f)) return bhr_fail(BHR_ERR_INVALID, "%s: index %g: in [0, 16] and no NaN", who, (double)p->index);
    if (p->emissivity != BHR_LINE_POWERLAW && p->emissivity != BHR_LINE_TEXTURE)
        return bhr_fail(BHR_ERR_INVALID, "%s: emissivity %d (BHR_LINE_POWERLAW = 0, BHR_LINE_TEXTURE = 1)", who, p->emissivity);
    if (p->orders != BHR_LINE_FIRST && p->orders != BHR_LINE_ALL) return bhr_fail(BHR_ERR_INVALID, "%s: orders %d (BHR_LINE_FIRST = 0, BHR_LINE_ALL = 1)", who, p->orders);
    *out = *p;
    if (p->r_inner == 0.0f && p->r_outer == 0.0f) {
        out->r_inner = ctx->cfg.r_disk_inner;
        out->r_outer = ctx->cfg.r_disk_outer;
    }
    if (!(out->r_inner >= ctx->cfg.r_disk_inner && out->r_inner < out->r_outer && out->r_outer <= ctx->cfg.r_disk_outer))
        return bhr_fail(BHR_ERR_INVALID, "%s: annulus r_inner %g, r_outer %g: inside the disk's [%g, %g] with r_inner < r_outer (0, 0: the disk's own)", who, (double)p->r_inner,
                        (double)p->r_outer, (double)ctx->cfg.r_disk_inner, (double)ctx->cfg.r_disk_outer);
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return bhr_fail(BHR_ERR_INVALID, "%s: reserved words other than 0", who);
    if (ctx->rows != ctx->cfg.height)
        return bhr_fail(BHR_ERR_INVALID, "%s: needs a whole-frame context (rows %d of %d): group and tile contexts have no ray map", who, ctx->rows, ctx->cfg.height);
    return BHR_OK;
}

int32_t need_line(const bhr_ctx *ctx, const char *who) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "%s: null ctx", who);
    if (!bhr_have_kerr_line(ctx) || !ctx->d_line_rows) return bhr_fail(BHR_ERR_STATE, "%s: no Kerr line is set (bhr_set_kerr_line)", who);
    return BHR_OK;
}

int32_t check_rows(const bhr_ctx *ctx, const char *who, int32_t first, int32_t n) {
    if (first < 0 || n < 1 || (int64_t)first + n > ctx->line_rows_n)
        return bhr_fail(BHR_ERR_INVALID, "%s: rows [%d, %lld) of %d reserved (bhr_kerr_line_reserve)", who, first, (long long)first + n, ctx->line_rows_n);
    return BHR_OK;
}

// rows [first, first + n) on the host, behind every frame in flight
int32_t fetch_rows(bhr_ctx *ctx, int32_t first, int32_t n, std::vector<unsigned long long> &host) {
    const size_t cells = (size_t)bhr_kerr_line_cells(ctx);
    host.resize((size_t)n * cells);
    BHR_TRY(bhr_enter(ctx));
    BHR_HIP(hipMemcpyAsync(host.data(), ctx->d_line_rows + (size_t)first * cells, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    return BHR_OK;
}

}  // namespace

void bhr_kerr_line_invalidate(bhr_ctx *ctx) {
    ctx->line_slot = -1;
    for (auto &f : ctx->slots) {
        f.line_keep = 0;
        f.line_row = -1;
    }
}

void bhr_kerr_line_release(bhr_ctx *ctx) {
    free_rows(ctx);
    ctx->kerr_line_on = 0;
}

// What a frame from the Kerr map `rm` (bhr_kerr_raymap_render, _view: turned, _shutter) is refused for while a line is set; nothing
// has been launched.
int32_t bhr_kerr_line_check_render(const bhr_ctx *ctx, const bhr_raymap *rm, const char *who, bool turned, bool shutter) {
    if (!bhr_have_kerr_line(ctx)) return BHR_OK;
    if (shutter)
        return bhr_fail(BHR_ERR_STATE, "%s: a Kerr line is set (bhr_set_kerr_line) and a mean of frames has no line profile -- switch it off (NULL) first", who);
    if (turned)
        return bhr_fail(BHR_ERR_STATE, "%s: a Kerr line is set (bhr_set_kerr_line) and the line pass walks the build view's records; turned views have none -- switch it off (NULL) first", who);
    if (rm->ss != 1)
        return bhr_fail(BHR_ERR_STATE, "%s: a Kerr line is set (bhr_set_kerr_line) and the map was built with kerr_raymap_supersample %d; the line pass needs a map with one ray per pixel", who, rm->ss);
    if (ctx->opt.kerr_line_row < 0 || ctx->opt.kerr_line_row >= ctx->line_rows_n)
        return bhr_fail(BHR_ERR_STATE, "%s: kerr_line_row %d of %d reserved rows (bhr_kerr_line_reserve)", who, ctx->opt.kerr_line_row, ctx->line_rows_n);
    return BHR_OK;
}

// The pass of the frame on slot k under `call` into the row of option "kerr_line_row" (bhr_kerr_line_check_render has seen it).
int32_t bhr_kerr_line_frame(bhr_ctx *ctx, const bhr_march_call &call, const bhr_raymap &rm, int k) {
    bhr_frame_slot &f = ctx->slots[k];
    const bhr_kerr_line &ln = ctx->kerr_line;
    const int32_t row = ctx->opt.kerr_line_row;
    const size_t cells = (size_t)bhr_kerr_line_cells(ctx);
    // two frame slots never share a row: a frame in flight on another slot that wrote this row ends first
    for (int j = 0; j < BHR_MAX_FRAME_SLOTS; ++j) {
        const bhr_frame_slot &o = ctx->slots[j];
        if (j != k && o.in_flight && o.line_row == row && o.done && o.stream != call.stream) BHR_HIP(hipStreamWaitEvent(call.stream, o.done, 0));
    }
    BhrKerrLineArgs s;
    memset(&s, 0, sizeof(s));
    s.row = ctx->d_line_rows + (size_t)row * cells;
    f.line_keep = 0;                   // until the launch is in the stream
    if (ctx->opt.kerr_line_samples) {
        const size_t want = 2 * (size_t)rm.a.slots * plane_floats(ctx);
        if (!f.d_line_samples || f.line_alloc != rm.a.slots) {
            if (f.d_line_samples) {
                BHR_HIP(hipStreamSynchronize(f.stream));   // the slot's last frame may still be writing the planes this replaces
                (void)hipFree(f.d_line_samples);
                f.d_line_samples = nullptr;
            }
            BHR_TRY(bhr_dev_alloc(&f.d_line_samples, want));
            f.line_alloc = rm.a.slots;
        }
        s.g_out = f.d_line_samples;
        s.w_out = f.d_line_samples + want / 2;
    }
    // both factors in binary64, rounded once
    s.g_min = ln.g_min;
    s.scale = (float)((double)ln.n_bins / ((double)ln.g_max - (double)ln.g_min));
    s.unit = (float)(4294967296.0 / pow((double)BHR_G_FACTOR_CAP, (double)ln.power));
    s.power = ln.power;
    s.index = ln.index;
    s.r_in = ln.r_inner;
    s.r_out = ln.r_outer;
    s.n_bins = ln.n_bins;
    s.all = ln.orders == BHR_LINE_ALL;
    BHR_HIP(hipMemsetAsync(s.row, 0, cells * sizeof(unsigned long long), call.stream));
    f.line_row = row;
    BHR_TRY(bhr_launch_kerr_line(ctx, call, rm.a, s, ln.emissivity == BHR_LINE_TEXTURE));
    if (s.g_out) {
        f.line_keep = rm.a.slots;
        ctx->line_slot = k;
    }
    // under the texture emissivity the pass samples the disk texture behind the frame's march bracket: it is then the frame's last
    // reader of the scene, and a scene write has to wait for it (api_polar.hip: the Stokes pass likewise)
    if (!f.line_done) BHR_HIP(hipEventCreateWithFlags(&f.line_done, hipEventDisableTiming));
    BHR_HIP(hipEventRecord(f.line_done, call.stream));
    f.march_done = f.line_done;
    return BHR_OK;
}

int32_t bhr_kerr_line_read_samples(bhr_ctx *ctx, const char *who, int32_t which, void *out, int64_t bytes) {
    if (!bhr_have_kerr_line(ctx)) return bhr_fail(BHR_ERR_STATE, "%s: no Kerr line is set (bhr_set_kerr_line)", who);
    if (ctx->line_slot < 0 || !ctx->slots[ctx->line_slot].d_line_samples || ctx->slots[ctx->line_slot].line_keep == 0)
        return bhr_fail(BHR_ERR_STATE, "%s: no frame from the Kerr ray map has been rendered with the line set and option \"kerr_line_samples\" on (bhr_kerr_raymap_render)", who);
    const bhr_frame_slot &f = ctx->slots[ctx->line_slot];
    const size_t n = (size_t)f.line_keep * plane_floats(ctx);
    if (bytes != (int64_t)(n * sizeof(float))) return bhr_fail(BHR_ERR_INVALID, "%s: plane %d has %zu bytes, caller gave %lld", who, which, n * sizeof(float), (long long)bytes);
    BHR_TRY(bhr_enter(ctx));
    return bhr_download(ctx, out, f.d_line_samples + (which == BHR_RAYMAP_LINE_W ? n : 0), n * sizeof(float));
}

extern "C" {

int32_t bhr_set_kerr_line(bhr_ctx *ctx, const bhr_kerr_line *p) {
    const char *who = "bhr_set_kerr_line";
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "%s: null ctx", who);
    bhr_kerr_line ln;
    memset(&ln, 0, sizeof(ln));
    if (p) {
        BHR_TRY(check_struct(ctx, who, p, &ln));
        if (!ctx->kerr_on)
            return bhr_fail(BHR_ERR_STATE, "%s: no spin is set and the Kerr march is not forced (bhr_set_spin): the line profile is a pass over the Kerr ray map", who);
    }
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(drain(ctx));               // a frame in flight may be writing the rows and planes this drops
    bhr_kerr_line_invalidate(ctx);
    free_rows(ctx);
    ctx->kerr_line = ln;
    ctx->kerr_line_on = 0;
    if (!p) return BHR_OK;
    BHR_TRY(alloc_rows(ctx, kDefaultRows));
    ctx->kerr_line_on = 1;
    return BHR_OK;
}

int32_t bhr_kerr_line_reserve(bhr_ctx *ctx, int32_t n_rows) {
    const char *who = "bhr_kerr_line_reserve";
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "%s: null ctx", who);
    if (!bhr_have_kerr_line(ctx)) return bhr_fail(BHR_ERR_STATE, "%s: no Kerr line is set (bhr_set_kerr_line)", who);
    if (n_rows < 1 || n_rows > kMaxRows) return bhr_fail(BHR_ERR_INVALID, "%s: %d rows (1 .. %d)", who, n_rows, kMaxRows);
    BHR_TRY(bhr_enter(ctx));
    BHR_TRY(drain(ctx));
    for (auto &f : ctx->slots) f.line_row = -1;
    return alloc_rows(ctx, n_rows);
}

int32_t bhr_kerr_line_read(bhr_ctx *ctx, int32_t first_row, int32_t n_rows, uint64_t *bins, uint64_t *under_over) {
    const char *who = "bhr_kerr_line_read";
    BHR_TRY(need_line(ctx, who));
    if (!bins || !under_over) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    BHR_TRY(check_rows(ctx, who, first_row, n_rows));
    std::vector<unsigned long long> host;
    BHR_TRY(fetch_rows(ctx, first_row, n_rows, host));
    const size_t nb = (size_t)ctx->kerr_line.n_bins, cells = nb + 4;
    for (size_t r = 0; r < (size_t)n_rows; ++r) {
        for (size_t b = 0; b < nb; ++b) bins[r * nb + b] = host[r * cells + b];
        under_over[2 * r] = host[r * cells + nb];
        under_over[2 * r + 1] = host[r * cells + nb + 1];
    }
    return BHR_OK;
}

int32_t bhr_kerr_line_info(bhr_ctx *ctx, int32_t row, int64_t out[2]) {
    const char *who = "bhr_kerr_line_info";
    BHR_TRY(need_line(ctx, who));
    if (!out) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    BHR_TRY(check_rows(ctx, who, row, 1));
    std::vector<unsigned long long> host;
    BHR_TRY(fetch_rows(ctx, row, 1, host));
    const size_t nb = (size_t)ctx->kerr_line.n_bins;
    out[0] = (int64_t)host[nb + 3];
    out[1] = (int64_t)host[nb + 2];
    return BHR_OK;
}

int32_t bhr_kerr_line_resources(int32_t redshift, int32_t texture, int32_t out[3]) {
    if (!out) return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_line_resources: null argument");
    if (redshift != BHR_REDSHIFT_MODEL && redshift != BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "bhr_kerr_line_resources: unknown mode %d (BHR_REDSHIFT_MODEL = 0, BHR_REDSHIFT_EXACT = 1)", redshift);
    const void *f = bhr_kerr_line_kernel(redshift == BHR_REDSHIFT_EXACT ? 1 : 0, texture ? 1 : 0);
    if (!f) return bhr_fail(BHR_ERR_STATE, "bhr_kerr_line_resources: no line kernel in this library");
    hipFuncAttributes at;
    BHR_HIP(hipFuncGetAttributes(&at, f));
    out[0] = at.numRegs;
    out[1] = (int32_t)at.sharedSizeBytes;
    out[2] = (int32_t)at.localSizeBytes;
    return BHR_OK;
}

}  // extern "C"
