"""The two Disk V2 parameter sets the suite pins: the defaults and one set away from them.  Shared by
tests/golden/make_golden.py (which writes the reference package's tables for both) and the tests that hold the
oracle and the device to those tables.  Plain keyword dictionaries: the reference's parameter classes and this
package's take the same names."""

MAX_TERMS = 32          # BHR_DV2_MAX_TERMS (include/bhr_disk_v2.h); the reference package has no upper limit

DEFAULT = dict(params={}, structure={}, fixture="disk_v2.npz")

# thick at the inner edge and flaring less than linearly, non-unit power laws and scales, as many shear components and
# hotspots as the device tables hold, and an edge as sharp as the reference package evaluates: it accepts
# edge_softness = 0 as a parameter but then raises in disk_radial_weight (its smoothstep gets r_in + 2.2e-16 == r_in as
# the upper edge), so the set takes 1e-15 -- a ramp of 4.5e-15, ten ulps of r_in, over which W_r goes from 0 to 1.
# edge_softness = 0 itself is covered against the oracle alone (SHARP)
ALT = dict(params=dict(r_in=3.0, r_out=7.5, h0=0.2, beta_h=-0.4, rho_power=1.7, temp_scale=0.8, omega_scale=1.3,
                       edge_softness=1e-15),
           structure=dict(mode1_strength=0.06, mode2_strength=0.02, shear_strength=0.35, shear_components=MAX_TERMS,
                          hotspot_strength=0.3, hotspot_count=MAX_TERMS, hotspot_phi_sigma=0.25,
                          hotspot_logr_sigma=0.2, hotspot_inner_bias=1.5),
           fixture="disk_v2_alt.npz")

SHARP = dict(params=dict(ALT["params"], edge_softness=0.0), structure=ALT["structure"], fixture=None)

SETS = {"default": DEFAULT, "alt": ALT, "sharp": SHARP}


def make(name):
    """(DiskV2Params, DiskV2StructureParams) of this package for the named set."""
    from bhr_amd import disk_v2 as dv
    s = SETS[name]
    return dv.DiskV2Params(**s["params"]), dv.DiskV2StructureParams(**s["structure"])
