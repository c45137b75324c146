// api_disk_v2.hip -- extern "C" entry point of include/bhr_disk_v2.h
#include "bhr_internal.h"

namespace {
struct DevBuf {
    double *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int32_t alloc(size_t n) {
        hipError_t e = hipMalloc((void **)&p, n * sizeof(double));
        if (e != hipSuccess) { p = nullptr; return bhr_fail(BHR_ERR_NOMEM, "hipMalloc failed: %s", hipGetErrorString(e)); }
        return BHR_OK;
    }
};
}  // namespace

extern "C" int32_t bhr_disk_v2_eval(bhr_ctx *ctx, const bhr_disk_v2_params *p, int32_t field, const double *r,
                                    const double *z, const double *phi, int64_t n, double norm_shear,
                                    double norm_hotspot, double *out, double *max_out) {
    if (!ctx || !p || !r || !out || n < 0) return bhr_fail(BHR_ERR_INVALID, "bhr_disk_v2_eval: bad argument");
    if (field < BHR_DV2_H || field > BHR_DV2_F_TOTAL) return bhr_fail(BHR_ERR_INVALID, "bhr_disk_v2_eval: field %d", field);
    if (p->shear_components < 0 || p->shear_components > BHR_DV2_MAX_TERMS || p->hotspot_count < 0 ||
        p->hotspot_count > BHR_DV2_MAX_TERMS)
        return bhr_fail(BHR_ERR_INVALID, "bhr_disk_v2_eval: at most %d shear components / hotspots", BHR_DV2_MAX_TERMS);
    const bool needs_z = field == BHR_DV2_W_Z || field == BHR_DV2_MASK_VOL || field == BHR_DV2_RHO || field == BHR_DV2_T;
    const bool needs_phi = field >= BHR_DV2_F_MODE;
    if ((needs_z && !z) || (needs_phi && !phi)) return bhr_fail(BHR_ERR_INVALID, "bhr_disk_v2_eval: field %d needs %s", field, needs_z ? "z" : "phi");
    if (n == 0) return BHR_OK;
    BHR_TRY(bhr_enter(ctx));
    DevBuf dr, dz, dphi, dout, daux, dmax;
    const size_t bytes = (size_t)n * sizeof(double);
    int32_t rc;
    if ((rc = dr.alloc(n)) || (rc = dout.alloc(n)) || (rc = dmax.alloc(2))) return rc;
    BHR_HIP(hipMemcpyAsync(dr.p, r, bytes, hipMemcpyHostToDevice, ctx->stream));
    if (needs_z) {
        if ((rc = dz.alloc(n))) return rc;
        BHR_HIP(hipMemcpyAsync(dz.p, z, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    if (needs_phi) {
        if ((rc = dphi.alloc(n))) return rc;
        BHR_HIP(hipMemcpyAsync(dphi.p, phi, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    if (field == BHR_DV2_F_TOTAL && (rc = daux.alloc(n))) return rc;
    if ((rc = bhr_launch_disk_v2(ctx, p, dr.p, dz.p, dphi.p, n, field, dout.p, daux.p, dmax.p, norm_shear, norm_hotspot))) return rc;
    BHR_HIP(hipMemcpyAsync(out, dout.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    double mx[2] = {0, 0};
    BHR_HIP(hipMemcpyAsync(mx, dmax.p, sizeof(mx), hipMemcpyDeviceToHost, ctx->stream));
    BHR_HIP(hipStreamSynchronize(ctx->stream));
    if (max_out) { max_out[0] = mx[0]; max_out[1] = mx[1]; }
    return BHR_OK;
}

// The disk source of one of the context's two slots -- kerr false: the Schwarzschild marches' (bhr_set_disk_source), true: the Kerr
// march's (bhr_set_kerr_disk_source) -- behind the entry point's own refusals: the argument checks, then behind the frames in
// flight the parameter block's upload, the norms and the volume's bounding slab into the slot's own fields.
static int32_t set_source(bhr_ctx *ctx, const char *who, bool kerr, int32_t source, const bhr_disk_v2_params *p, double norm_shear, double norm_hotspot,
                          double t_peak) {
    if (source != BHR_DISK_TEXTURE && source != BHR_DISK_V2 && source != BHR_DISK_V2_VOLUME) return bhr_fail(BHR_ERR_INVALID, "%s: bad argument", who);
    BHR_TRY(bhr_enter(ctx));
    if (source != BHR_DISK_TEXTURE) {
        if (!p || !(norm_shear > 0.0) || !(norm_hotspot > 0.0) || !(t_peak > 0.0))
            return bhr_fail(BHR_ERR_INVALID, "%s: Disk V2 needs parameters and positive normalisation constants", who);
        if (!(p->r_out > p->r_in) || !(p->r_in > 0.0) || !(p->h0 > 0.0) || p->shear_components < 0 ||
            p->shear_components > BHR_DV2_MAX_TERMS || p->hotspot_count < 0 || p->hotspot_count > BHR_DV2_MAX_TERMS)
            return bhr_fail(BHR_ERR_INVALID, "%s: inconsistent Disk V2 parameters", who);
        bhr_disk_v2_params *&d_params = kerr ? ctx->d_kerr_dv2_params : ctx->d_dv2_params;
        double *norm = kerr ? ctx->kerr_dv2_norm : ctx->dv2_norm, *bound = kerr ? ctx->kerr_vol_bound : ctx->vol_opts + 2;
        if (!d_params) BHR_HIP(hipMalloc((void **)&d_params, sizeof(bhr_disk_v2_params)));
        BHR_HIP(hipMemcpyAsync(d_params, p, sizeof(*p), hipMemcpyHostToDevice, ctx->stream));
        BHR_HIP(hipStreamSynchronize(ctx->stream));
        norm[0] = norm_shear;
        norm[1] = norm_hotspot;
        norm[2] = t_peak;
        // bounding slab of the volume: H(r) = h0 r (r / r_in)^beta is monotonic, its maximum sits at an end
        const double h_in = p->h0 * p->r_in, h_out = p->h0 * p->r_out * pow(p->r_out / p->r_in, p->beta_h);
        bound[0] = h_in > h_out ? h_in : h_out;
        bound[1] = sqrt(p->r_out * p->r_out + bound[0] * bound[0]);
        if (ctx->vol_substeps == 0) {   // options never set: defaults
            ctx->vol_opts[0] = 4.0;
            ctx->vol_opts[1] = 1.0;
            ctx->vol_substeps = 2;
        }
    }
    (kerr ? ctx->kerr_disk_source : ctx->disk_source) = source;
    return BHR_OK;
}

extern "C" int32_t bhr_set_disk_source(bhr_ctx *ctx, int32_t source, const bhr_disk_v2_params *p, double norm_shear,
                                       double norm_hotspot, double t_peak) {
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "bhr_set_disk_source: bad argument");
    return set_source(ctx, "bhr_set_disk_source", false, source, p, norm_shear, norm_hotspot, t_peak);
}

// The Kerr march's own disk source (include/bhr_disk_v2.h).  Everything it does not combine with is refused here or where the
// other side is set, each naming the combination; then set_source, and the counters name the kernel that marches the frames.
extern "C" int32_t bhr_set_kerr_disk_source(bhr_ctx *ctx, int32_t source, const bhr_disk_v2_params *p, double norm_shear,
                                            double norm_hotspot, double t_peak) {
    const char *who = "bhr_set_kerr_disk_source";
    if (!ctx) return bhr_fail(BHR_ERR_INVALID, "%s: null ctx", who);
    if (source != BHR_DISK_TEXTURE && source != BHR_DISK_V2 && source != BHR_DISK_V2_VOLUME)
        return bhr_fail(BHR_ERR_INVALID, "%s: unknown source %d (BHR_DISK_TEXTURE = 0, BHR_DISK_V2 = 1, BHR_DISK_V2_VOLUME = 2)", who, source);
    if (source != BHR_DISK_TEXTURE) {
        if (!ctx->kerr_on)
            return bhr_fail(BHR_ERR_STATE, "%s: a Kerr Disk V2 source without the Kerr march: set a spin, or force_kerr at spin 0, first (bhr_set_spin)", who);
        if (source == BHR_DISK_V2_VOLUME && ctx->kerr_redshift == BHR_REDSHIFT_EXACT)
            return bhr_fail(BHR_ERR_INVALID, "%s: the Disk V2 volume with the exact redshift (bhr_set_redshift): gas off the equatorial plane has no four-velocity in this model; "
                            "set BHR_REDSHIFT_MODEL first", who);
        if (ctx->kerr_aa)
            return bhr_fail(BHR_ERR_INVALID, "%s: a Kerr Disk V2 source with the Kerr anti-aliasing on (bhr_set_kerr_anti_alias): the analytic source has no mip chain; switch it off first", who);
        if (ctx->kerr_raymap && ctx->kerr_raymap->built)
            return bhr_fail(BHR_ERR_INVALID, "%s: a Kerr Disk V2 source while a Kerr ray map is built (bhr_kerr_raymap_build): a frame from the map shades the disk texture; free it first (bhr_kerr_raymap_free)", who);
    }
    BHR_TRY(set_source(ctx, who, true, source, p, norm_shear, norm_hotspot, t_peak));
    return bhr_note_frame_kernel(ctx);
}

extern "C" int32_t bhr_kerr_disk_resources(int32_t source, int32_t mode, int32_t ss, int32_t out[3]) {
    const char *who = "bhr_kerr_disk_resources";
    if (!out) return bhr_fail(BHR_ERR_INVALID, "%s: null argument", who);
    if (source != BHR_DISK_V2 && source != BHR_DISK_V2_VOLUME) return bhr_fail(BHR_ERR_INVALID, "%s: source %d (BHR_DISK_V2 = 1 or BHR_DISK_V2_VOLUME = 2)", who, source);
    if (mode != BHR_REDSHIFT_MODEL && mode != BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "%s: unknown mode %d (BHR_REDSHIFT_MODEL = 0, BHR_REDSHIFT_EXACT = 1)", who, mode);
    if (source == BHR_DISK_V2_VOLUME && mode == BHR_REDSHIFT_EXACT)
        return bhr_fail(BHR_ERR_INVALID, "%s: the Disk V2 volume with the exact redshift: there is no such kernel", who);
    const void *f = bhr_kerr_dv2_kernel(source, mode, ss ? 1 : 0);
    if (!f) return bhr_fail(BHR_ERR_STATE, "%s: no such march kernel in this library", who);
    hipFuncAttributes at;
    BHR_HIP(hipFuncGetAttributes(&at, f));
    out[0] = at.numRegs;
    out[1] = (int32_t)at.sharedSizeBytes;
    out[2] = (int32_t)at.localSizeBytes;
    return BHR_OK;
}

extern "C" int32_t bhr_set_disk_volume_options(bhr_ctx *ctx, double absorption, double grazing_gain, int32_t substeps) {
    if (!ctx || !(absorption >= 0.0) || !(grazing_gain >= 0.0) || substeps < 1 || substeps > 16)
        return bhr_fail(BHR_ERR_INVALID, "bhr_set_disk_volume_options: absorption/grazing_gain must be >= 0, substeps in 1..16");
    ctx->vol_opts[0] = absorption;
    ctx->vol_opts[1] = grazing_gain;
    ctx->vol_substeps = substeps;
    return BHR_OK;
}
