"""math="hybrid" (BHR_MATH_HYBRID, csrc/hybrid.hip): the strict kernel on the 8x8 tiles whose rays pass near the photon
sphere, the fast kernel elsewhere.  Held to the bars the verdict of round 2 set: every reference-statement fixture (f32
and f64, 7 views), the e2e frame, video frames 0 / 2 / 7 and the whole fhd frame within 1e-4 per channel -- with the
stated margin: <= 3e-5 -- and ray-step totals within 2e-4.  No oracle involved: HIP vs the reference's statements, and
HIP hybrid vs HIP strict (which is bit-identical to the f32 statements in its ray paths)."""
import numpy as np
import pytest

from test_reference_kernels import FLARE, KW, MARCH, load_scene

pytestmark = pytest.mark.gpu

NORTH_STAR = 1e-4
MARGIN = 3e-5


def _rmse_c(a, b):
    return np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2, axis=(0, 1)))


def _ref_layer(g, mode, k):
    a = g[f"{mode}_{k}"]
    return a if k == "final" else a.transpose(1, 0, 2)


@pytest.mark.parametrize("name", MARCH)
def test_hybrid_vs_reference_statements(name, hip_lib):
    from bhr_amd import HipRenderer, _lib
    g, sky, tex = load_scene(name)
    hip = HipRenderer(int(g["width"]), int(g["height"]), sky, tex, lens_flare=(name in FLARE), math="hybrid", **KW[name])
    final = hip.render(list(g["cam_pos"]), float(g["fov"]), frame=int(g["frame"]))
    lay = dict(final=final, bg=hip.read_layer(_lib.LAYER_BG), disk=hip.read_layer(_lib.LAYER_DISK), blur=hip.read_layer(_lib.LAYER_BLUR))
    steps = hip.counters()["ray_steps"]
    info = hip.hybrid_info()                     # anti-aliased views run hybrid too (march_tile_aa_hybrid)
    assert 0 < info["strict_tiles"] <= info["tiles"]
    hip.close()
    for mode in ("f32", "f64"):
        ref_steps = int(g[f"{mode}_steps"].sum())
        assert abs(steps - ref_steps) <= 2e-4 * ref_steps, (name, mode, steps, ref_steps)
        for k in ("bg", "disk", "blur", "final"):
            e = float(_rmse_c(lay[k], _ref_layer(g, mode, k)).max())
            # f64 fixtures: the f32 evaluation of the reference's own statements is itself up to 3e-5 away on these frames
            bar = MARGIN if mode == "f32" else NORTH_STAR
            assert e <= bar, f"{name}/{mode}/{k}: per-channel RMSE {e:.3g} > {bar:.3g}"


def test_hybrid_e2e_frame(hip_lib):
    from bhr_amd import HipRenderer
    from test_reference_kernels import E2E_KW, load_e2e
    g, sky = load_e2e()
    hip = HipRenderer(320, 180, sky, g["disk_tex"], math="hybrid", **E2E_KW)
    out = hip.render([6, 0, 0.5], 60)
    steps, info = hip.counters()["ray_steps"], hip.hybrid_info()
    strict = hip.render_async([6, 0, 0.5], 60, math="strict")
    strict_steps = hip.counters()["ray_steps"]
    hip.close()
    e = _rmse_c(out, g["final"])
    assert (e <= MARGIN).all(), e                                 # measured 1.9e-6
    assert np.abs(out - g["final"]).max() <= 1e-3                 # measured 9e-5
    assert abs(steps - strict_steps) <= 2e-4 * strict_steps
    assert info["strict_tiles"] < info["tiles"]                   # a real mix of the two kernels


def test_hybrid_video_frames(hip_lib):
    """Frames 0, 2, 7 of the reference's video loop (populations ticking, orbit camera) with the hybrid march."""
    from bhr_amd import HipRenderer, drivers
    from bhr_amd.camera import orbit_position
    from test_reference_kernels import E2E_KW, load_video
    g, sky = load_video()
    n_r, n_phi = (int(v) for v in g["tex_shape"])
    r = HipRenderer(320, 180, sky, np.zeros((n_r, n_phi, 4), np.float32), math="hybrid", **E2E_KW)
    fac = drivers.init_lifecycle_system(r, n_r, n_phi, seed=42)
    dt = float(g["speed"])
    stored = [int(f) for f in g["frames"]]
    for frame in range(max(stored) + 1):
        drivers.advance_lifecycle_frame(r, fac, frame * dt, dt, recompute_stats=(frame % 60 == 0), compose=frame in stored)
        if frame not in stored:
            continue
        cam = orbit_position([6.0, 0.0, 0.5], frame, int(g["n_frames"]), float(g["orbit_degrees"]))
        img = r.render(cam, 60)
        e = _rmse_c(img, g[f"final_{frame}"])
        assert (e <= MARGIN).all(), (frame, e)
    r.close()


def test_hybrid_whole_fhd_frame_vs_strict(hip_lib):
    """The BASELINE fhd bench frame (procedural sky + lifecycle texture): hybrid vs strict on all 2 073 600 pixels of the
    three layers and the frame -- RMSE <= 3e-5 per channel (measured 1.0e-5 / 1.2e-5 / 1.5e-5), ray-step totals within
    2e-4 (measured 1.3e-7); strict tiles are a small share of the frame.

    Single pixels: the fast arithmetic's rounding can move a ray across one of the ALGORITHM'S OWN switches -- a disk
    crossing in the terminating step, a truncated mip level -- and such a pixel then differs by a visible share of a disk
    colour, far from the strict band (round 4: two mirror-image pixels at b = b_c + 1.0, 9e-3 and 4e-3; round 3's
    re-association of the same step had none).  Those are what the guard / fix-list launches exist for (hybrid_repair,
    default on for anti-aliased and tilted views, off here for its 17 % of the fhd frame rate): without them at most 4
    pixels beyond 1e-3 and none beyond 2e-2; with them none beyond 1e-3."""
    import bench
    from bhr_amd import _lib, workloads
    wl = bench.WORKLOADS["fhd"]
    r, _, _, _ = workloads.make_scene(wl, frame_slots=1)
    lay = {}
    for math, repair in (("strict", -1), ("hybrid", -1), ("hybrid", 1)):
        r.set_option("hybrid_repair", repair)
        r.render_async(wl["cam_pos"], wl["fov"], math=math)
        lay[(math, repair)] = dict(final=r.read_layer(_lib.LAYER_FINAL), bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK),
                                   steps=r.counters()["ray_steps"])
        if math == "hybrid":
            info = r.hybrid_info()
            assert (info["repaired_pixels"] > 0) == (repair == 1), info
    r.close()
    ref = lay[("strict", -1)]
    assert info["strict_tiles"] / info["tiles"] <= 0.12, info
    for repair in (-1, 1):
        got = lay[("hybrid", repair)]
        assert abs(got["steps"] - ref["steps"]) <= 2e-4 * ref["steps"]
        for k in ("final", "bg", "disk"):
            e = _rmse_c(got[k], ref[k])
            assert (e <= MARGIN).all(), (repair, k, e)
        d = np.abs(got["final"] - ref["final"]).max(axis=2)
        print(f"\n[hybrid fhd, repair {repair}] pixels beyond 1e-3: {int((d > 1e-3).sum())}, max {d.max():.3g}, per-channel RMSE {_rmse_c(got['final'], ref['final'])}")
        if repair == 1:
            assert (d > 1e-3).sum() == 0, (int((d > 1e-3).sum()), float(d.max()))
        else:
            assert (d > 1e-3).sum() <= 4 and d.max() <= 2e-2, (int((d > 1e-3).sum()), float(d.max()))


def test_hybrid_strict_tiles_are_bit_identical_to_strict(hip_lib):
    """Inside the strict band the hybrid frame IS the strict frame: with a band that covers every tile the two marches
    give identical frames (with the default band the pixels of the strict tiles are identical: the test below)."""
    import os
    from bhr_amd import HipRenderer, _lib, scenes
    s = scenes.SCENES["default"]
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    os.environ["BHR_HYBRID_BAND"] = "10,100"
    try:
        r = HipRenderer(s["width"], s["height"], sky, tex, options={"bloom_split": 0}, **s["kw"])   # one post-pass for both frames: the marches are compared
        a = r.render(s["cam_pos"], s["fov"])
        b_steps = None
        r.render_async(s["cam_pos"], s["fov"], math="hybrid")
        b = r.read_layer(_lib.LAYER_FINAL)
        info = r.hybrid_info()
        r.close()
    finally:
        os.environ.pop("BHR_HYBRID_BAND", None)
    assert info["strict_tiles"] == info["tiles"]
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("view", ["fhd", "8k", "cam2.6", "rows", "4k_aa"])
def test_hybrid_strict_tiles_are_the_strict_frame_at_the_default_band(view, hip_lib):
    """With the DEFAULT band, every pixel of the strict list's tiles has the strict march's bg and disk values bit for bit:
    the strict list is marched by the strict kernel (march_tile_plain_ilp; march_tile_aa_ilp for an anti-aliased view --
    the kernels math="strict" launches), only over a sub-list of the tiles."""
    from bhr_amd import HipRenderer, _lib, scenes
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk(256, 1024)
    kw = dict(step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=0.0)
    W, H, cam, fov, rows = 1920, 1080, [6.0, 0.0, 0.5], 90.0, None
    if view == "8k":
        W, H, kw["step_size"] = 7680, 4320, 0.05
    elif view == "cam2.6":
        W, H, cam, fov = 960, 540, [2.6, 0.3, 0.2], 110.0
    elif view == "rows":
        rows = (97, 251 + 8 * 40)
    elif view == "4k_aa":
        W, H, kw = 3840, 2160, dict(kw, disk_tilt=25.0, anti_alias="lod_radius")
    r = HipRenderer(W, H, sky, tex, rows=rows, frame_slots=1, **kw)
    mask = None
    for layer, name in ((_lib.LAYER_BG, "bg"), (_lib.LAYER_DISK, "disk")):      # one layer pair on the host at a time (8k)
        r.render_async(cam, fov, skip_bloom=True, math="strict")
        want = r.read_layer(layer)
        r.render_async(cam, fov, skip_bloom=True, math="hybrid")
        got = r.read_layer(layer)
        if mask is None:
            info, order = r.hybrid_info(), r.hybrid_launch_order()
            assert (info["band_below"], info["band_above"]) == (0.085, 0.36), info
            assert 0 < info["strict_tiles"] < info["tiles"], info
            tiles_x, rows_n = (W + 7) // 8, got.shape[0]
            ty, tx = np.divmod(order[:info["strict_tiles"]], tiles_x)
            tiles = np.zeros(((rows_n + 7) // 8, tiles_x), bool)
            tiles[ty, tx] = True
            mask = np.repeat(np.repeat(tiles, 8, axis=0), 8, axis=1)[:rows_n, :W]
        same = (got == want).all(axis=2)
        del got, want
        assert same[mask].all(), f"{view} {name}: {int((~same & mask).sum())} pixels of strict tiles differ from the strict frame"
    r.close()


@pytest.mark.parametrize("source", ["v2", "v2_volume"])
def test_hybrid_with_a_disk_v2_source_is_the_strict_march(source, hip_lib):
    """Hybrid does not split a frame whose disk comes from the Disk V2 model: include/bhr.h has it resolve to strict for
    those sources (bhr_resolve_math: the model's kernels have no fast / strict list pair; bench.py and the CLI rely on
    it).  No error is documented or returned, so the property the texture has on its strict tiles -- the pixels ARE the
    strict march's -- must hold on every tile: BG and DISK of a math="hybrid" frame are the FORCE_STRICT frame bit for
    bit, with the same ray steps, and no hybrid march is on record.  With adaptive supersampling on top the refinement
    runs the model's LIST kernels (march_launch.hip: BHR_MK_LIST_DV2 / _VOLUME) under the same resolution.  The view is
    one the texture splits into both tile kinds."""
    from bhr_amd import HipRenderer, _lib, scenes
    from bhr_amd.disk_v2 import DiskV2Params
    from test_reference_kernels import E2E_KW
    W, H, cam, fov = 320, 180, [6.0, 0.0, 0.5], 60.0
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    kw = dict(E2E_KW, r_disk_outer=10.0)                                        # the model's radii
    for extra in (dict(), dict(supersample=2, supersample_threshold=0.25)):
        r = HipRenderer(W, H, sky, tex, math="hybrid", **dict(kw, **extra))
        if not extra:
            r.render_async(cam, fov, skip_bloom=True)
            info = r.hybrid_info()
            assert 0 < info["strict_tiles"] < info["tiles"], info            # the texture: both kinds of tiles
        r.use_disk_v2(DiskV2Params(), volume=source == "v2_volume")
        frames = {}
        for math in ("hybrid", "strict"):
            r.render_async(cam, fov, frame=25, skip_bloom=True, math=math)
            frames[math] = (r.read_layer(_lib.LAYER_BG), r.read_layer(_lib.LAYER_DISK), r.counters()["ray_steps"],
                            r.adaptive_info() if extra else None)
        assert frames["strict"][1].max() > 0.3 and (frames["strict"][1].sum(axis=2) > 0).mean() > 0.1
        np.testing.assert_array_equal(frames["hybrid"][0], frames["strict"][0])
        np.testing.assert_array_equal(frames["hybrid"][1], frames["strict"][1])
        assert frames["hybrid"][2:] == frames["strict"][2:]
        if extra:
            assert 0 < frames["hybrid"][3]["refined"] < W * H
            assert frames["hybrid"][3]["strict"] == frames["hybrid"][3]["refined"]      # every refined pixel marched strict
        fresh = HipRenderer(W, H, sky, tex, math="hybrid", **dict(kw, **extra))
        fresh.use_disk_v2(DiskV2Params(), volume=source == "v2_volume")
        fresh.render_async(cam, fov, frame=25, skip_bloom=True)
        np.testing.assert_array_equal(fresh.read_layer(_lib.LAYER_DISK), frames["strict"][1])
        with pytest.raises(AssertionError):                                             # BHR_ERR_STATE: no hybrid march has run
            fresh.hybrid_info()
        fresh.close()
        r.close()


def test_hybrid_in_row_blocks(hip_lib):
    """Hybrid tiles in a group render (pipelined: band lists x strict / fast lists = four launches per tile) against one
    hybrid context: the classification is per 8x8 tile of the image, so the pixels are the same ones."""
    from bhr_amd import HipRenderer, multigpu, scenes
    s = scenes.SCENES["default"]
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    cuts = [0, 56, 120, 180]
    tiles = [HipRenderer(s["width"], s["height"], sky, tex, rows=(cuts[k], cuts[k + 1]), math="hybrid", **s["kw"]) for k in range(3)]
    full = HipRenderer(s["width"], s["height"], sky, tex, math="hybrid", **s["kw"])
    ref = full.render(s["cam_pos"], s["fov"])
    for sched in ("pipelined", "serial"):
        got = multigpu.group_render(tiles, s["cam_pos"], s["fov"], gather="host", schedule=sched)
        np.testing.assert_allclose(got, ref, atol=1e-6, rtol=0)
    assert sum(t.counters()["ray_steps"] for t in tiles) == full.counters()["ray_steps"]
    for t in tiles + [full]:
        t.close()


def test_hybrid_with_lod_anti_aliasing_4k(hip_lib):
    """BASELINE.json configs[2] (3840x2160, tilt 25 deg, lod_radius): the mip level is a truncated function of the ray
    differentials, so a plain fast march flips it on ~300 pixels by up to 0.8 (5e-4 RMSE on the disk layer,
    tools/hybrid_sweep.py).  The hybrid march re-marches every lane whose lod lies within 2e-3 of a level boundary with the
    strict arithmetic: whole frame vs strict RMSE <= 3e-5 per channel on every layer, no pixel of the frame beyond 1e-3."""
    import bench
    from bhr_amd import _lib, workloads
    wl = bench.WORKLOADS["4k"]
    r, _, _, _ = workloads.make_scene(wl, frame_slots=1)
    lay = {}
    for math in ("strict", "hybrid"):
        r.render_async(wl["cam_pos"], wl["fov"], math=math)
        lay[math] = dict(final=r.read_layer(_lib.LAYER_FINAL), bg=r.read_layer(_lib.LAYER_BG), disk=r.read_layer(_lib.LAYER_DISK),
                         steps=r.counters()["ray_steps"])
    info = r.hybrid_info()
    r.close()
    assert info["strict_tiles"] / info["tiles"] <= 0.12, info
    assert abs(lay["hybrid"]["steps"] - lay["strict"]["steps"]) <= 2e-4 * lay["strict"]["steps"]
    for k in ("final", "bg", "disk"):
        e = _rmse_c(lay["hybrid"][k], lay["strict"][k])
        assert (e <= MARGIN).all(), (k, e)
    d = np.abs(lay["hybrid"]["final"] - lay["strict"]["final"]).max(axis=2)
    assert d.max() <= 0.05 and (d > 1e-3).sum() <= 100, (float(d.max()), int((d > 1e-3).sum()))   # measured: 0.014, 30 of 8.3 M


def test_hybrid_guards_catch_the_algorithm_s_own_switches(hip_lib, capsys, monkeypatch):
    """Far from the photon ring the reference's algorithm still has switches that only the bit-identical arithmetic
    reproduces: a step whose new_pos has a plane function of exactly 0 is a crossing no step ever registers (the test is
    f_old f_new < 0: a black pixel inside the disk), a crossing in the terminating step registers no hit, the annulus test.
    ~1e-6 of the crossings of a TILTED disk -- but each is a whole disk colour.  With the guards on (the default for tilted
    disks and for anti-aliased views) those lanes are re-marched strict: no pixel of a 4k tilt-25 frame differs from strict
    by more than 0.05 (measured 0.0046); with the guards forced off the frame shows a dozen such pixels (12, max 0.79: printed,
    they are the reference's own discontinuities -- any two builds of it disagree there too)."""
    import bench
    from bhr_amd import _lib, workloads
    wl = dict(bench.WORKLOADS["4k"], anti_alias="disabled", lens_flare=False)
    r, _, _, _ = workloads.make_scene(wl, frame_slots=1)
    r.render_async(wl["cam_pos"], wl["fov"], math="strict")
    strict = r.read_layer(_lib.LAYER_DISK)
    out = {}
    for rep in ("default", "0"):
        r.set_option("hybrid_repair", -1 if rep == "default" else int(rep))     # BHR_HYBRID_REPAIR at bhr_create, or per context
        r.render_async(wl["cam_pos"], wl["fov"], math="hybrid")
        disk = r.read_layer(_lib.LAYER_DISK)
        d = np.abs(disk - strict).max(axis=2)
        out[rep] = (float(d.max()), int((d > 0.05).sum()), float(_rmse_c(disk, strict).max()))
    r.close()
    with capsys.disabled():
        print(f"\n[hybrid guards] 4k tilt 25, AA off, disk layer vs strict (max, pixels > 0.05, per-channel RMSE): guards on {out['default']}, off {out['0']}")
    assert out["default"][0] <= 0.05 and out["default"][1] == 0, out
    assert out["default"][2] <= 5e-5 and out["0"][2] <= 1e-3, out


def test_row_costs_split_by_arithmetic_and_hybrid_balanced_blocks(hip_lib):
    """BHR_ROW_COSTS under hybrid: the two tile lists fill two profiles (fast steps, strict steps) whose sum is the frame's
    ray-step total; the strict profile is confined to the rows through the photon ring; row blocks balanced on
    fast + STRICT_STEP_COST x strict move rows away from the blocks that hold the ring."""
    from bhr_amd import HipRenderer, multigpu, scenes
    W, H = 960, 544
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    kw = dict(step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=0.0)
    cam, fov = [6.0, 0.0, 0.5], 90.0
    r = HipRenderer(W, H, sky, tex, math="hybrid", **kw)
    fast, strict = r.row_costs(cam, fov, split=True)
    total = r.row_costs(cam, fov)
    np.testing.assert_array_equal(fast + strict, total)
    assert strict.sum() > 0 and fast.sum() > 0
    rows_with_strict = np.nonzero(strict)[0]
    assert rows_with_strict.min() > 5 and rows_with_strict.max() < len(strict) - 6      # the ring sits in the middle bands
    s = HipRenderer(W, H, sky, tex, math="strict", **kw)
    f0, s0 = s.row_costs(cam, fov, split=True)
    assert f0.sum() == 0 and s0.sum() > 0
    # the same rays whichever arithmetic: step totals of the hybrid frame within 2e-4 of the strict frame's
    assert abs(int(total.sum()) - int(s0.sum())) <= 2e-4 * s0.sum() + 64 * 8
    r.close()
    s.close()
    per_f, _ = multigpu.probe_row_costs(3840, 2160, cam, fov, math=None, **kw)
    per_h, _ = multigpu.probe_row_costs(3840, 2160, cam, fov, math="hybrid", **kw)
    bf = multigpu.balanced_row_blocks(2160, 8, per_f, 1, fixed_cost_per_row=0.1 * float(per_f.mean()))
    bh = multigpu.balanced_row_blocks(2160, 8, per_h, 1, fixed_cost_per_row=0.1 * float(per_h.mean()))
    mid_f = sum(b[1] - b[0] for b in bf[2:6])
    mid_h = sum(b[1] - b[0] for b in bh[2:6])
    assert mid_h < mid_f, (bf, bh)                     # the four middle blocks (the ring's) get fewer rows under hybrid costs


@pytest.mark.parametrize("cam,tilt", [([6.0, 0.0, 0.0], 0.0), ([-10.27977657706746, 3.4882456957730086, 5.652677980932753], 58.41173651690485)])
def test_edge_on_camera_marches_the_in_plane_rays_strict(cam, tilt, hip_lib):
    """A camera in the disk plane (exactly, or by 0.01 r_s of 12 as the fuzzed view that found this): the rays whose orbital
    plane all but coincides with the disk plane -- a line through the hole's image -- have a plane function of ~0 all along,
    their "crossings" are decided by rounding in any arithmetic, and the fast kernel's line-of-nodes basis is ill defined.
    Their tiles go to the strict list: hybrid == strict on them, and the frame stays inside the certified margin."""
    from bhr_amd import HipRenderer, _lib, scenes
    W, H = 640, 360
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    kw = dict(step_size=0.1, r_max=25.0, r_disk_inner=2.35, r_disk_outer=20.0, disk_tilt=tilt)
    r = HipRenderer(W, H, sky, tex, math="hybrid", **kw)
    lay = {}
    for math in ("hybrid", "strict"):
        r.render_async(cam, 100.0, skip_bloom=True, math=math)
        lay[math] = (r.read_layer(_lib.LAYER_BG), r.read_layer(_lib.LAYER_DISK))
        if math == "hybrid":
            info = r.hybrid_info()
    r.close()
    assert info["strict_tiles"] >= W // 8                   # at least the row (or diagonal) of tiles the line runs through
    for a, b in zip(lay["hybrid"], lay["strict"]):
        d = np.abs(a - b).max(axis=2)
        e = np.sqrt(np.mean((a.astype(np.float64) - b) ** 2, axis=(0, 1)))
        assert (e <= 3e-5).all() and int((d > 1e-2).sum()) == 0, (e, int((d > 1e-2).sum()), info)


def test_hybrid_repairs_are_counted_and_fit_their_list(hip_lib):
    """bhr_hybrid_repairs: a tilted anti-aliased view hands a small share of its pixels to the strict fix kernel, well inside the
    list (an eighth of the pixels); the default view runs without guards."""
    from bhr_amd import HipRenderer, scenes
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    kw = dict(step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0)
    r = HipRenderer(960, 544, sky, tex, math="hybrid", disk_tilt=25.0, anti_alias="lod_radius", aa_strength=1.5, **kw)
    r.render_async([6.0, 0.0, 0.5], 90.0, skip_bloom=True)
    info = r.hybrid_info()
    r.close()
    assert 0 < info["repaired_pixels"] <= 0.03 * 960 * 544 and info["repair_capacity"] == 960 * 544 // 8, info
    r = HipRenderer(960, 544, sky, tex, math="hybrid", disk_tilt=0.0, **kw)
    r.render_async([6.0, 0.0, 0.5], 90.0, skip_bloom=True)
    info = r.hybrid_info()
    r.close()
    assert info["repaired_pixels"] == 0 and info["repair_capacity"] == 0, info


@pytest.mark.parametrize("repair", [-1, 0])
def test_one_and_two_march_streams_give_the_same_frame(repair, hip_lib):
    """Option "hybrid_streams": the strict list of a hybrid march ahead of the fast one on the frame's stream (1), or beside it
    on the slot's second stream (2).  Both settings run the same three kernels over the same lists -- a tilted disk turns
    the guards and the fix list on by default; hybrid_repair 0 takes them out -- so the frame and the repair count are
    identical bit for bit."""
    from bhr_amd import HipRenderer, _lib, scenes
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    r = HipRenderer(256, 160, sky, tex, math="hybrid", frame_slots=2, step_size=0.1, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=25.0)
    r.set_option("hybrid_repair", repair)
    got = {}
    for streams in (1, 2):
        r.set_option("hybrid_streams", streams)
        r.render_async([6.0, 0.0, 0.5], 90.0)
        info = r.hybrid_info()
        got[streams] = (r.read_layer(_lib.LAYER_FINAL), (info["repaired_pixels"], info["repair_capacity"]), info["strict_tiles"])
    r.close()
    assert 0 < got[1][2] < (256 // 8) * (160 // 8)                 # both lists hold tiles: there is something for the second stream
    assert (got[1][1][0] > 0) == (repair != 0) and (got[1][1][1] > 0) == (repair != 0), got[1][1]
    assert got[1][1] == got[2][1], (got[1][1], got[2][1])
    np.testing.assert_array_equal(got[1][0], got[2][0])


def test_device_classification_makes_the_host_s_lists(hip_lib):
    """The tiles are classified and the launch order partitioned on the device by default (csrc/hybrid.hip: four small
    kernels on a stream of their own, the host waits for the strict count alone); option "hybrid_classify" 0 keeps the
    round-3 path on the submitting thread.  Same binary64 rule, same operations in the same order: the two paths must
    produce the same list, tile for tile -- on the BASELINE pov, cameras inside 3 r_s, in and next to the disk plane, tilted
    disks, a row block -- and the same frame bit for bit."""
    import time
    from bhr_amd import HipRenderer, _lib, scenes
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    rng = np.random.default_rng(20260405)
    views = [([6.0, 0.0, 0.5], 90.0, 0.0, None), ([6.0, 0.0, 0.0], 100.0, 0.0, None), ([2.6, 0.3, 0.2], 110.0, 0.0, None),
             ([-10.27977657706746, 3.4882456957730086, 5.652677980932753], 100.0, 58.41173651690485, None),
             ([6.0, 0.0, 0.5], 90.0, 0.0, (96, 251)), ([20.0, 3.0, 0.1], 30.0, 25.0, None)]
    for _ in range(6):
        d = rng.normal(size=3)
        views.append(((d / np.linalg.norm(d) * rng.uniform(2.2, 30.0)).tolist(), float(rng.uniform(30, 120)), float(rng.choice([0.0, rng.uniform(-60, 60)])), None))
    W, H = 648, 362                                    # ragged last tile column and row
    for cam, fov, tilt, rows in views:
        kw = dict(step_size=0.1, r_max=25.0, r_disk_inner=2.35, r_disk_outer=20.0, disk_tilt=tilt)
        got = {}
        for where in (1, 0):
            r = HipRenderer(W, H, sky, tex, math="hybrid", rows=rows, options={"hybrid_classify": where}, **kw)
            r.render_async(cam, fov)
            got[where] = (r.hybrid_launch_order(), r.hybrid_info()["strict_tiles"], r.read_final_u8())
            if where == 1:                              # a second view change on a live context, then back: the ring of list buffers
                r.render_async([c * 1.5 for c in cam], fov)
                other = r.hybrid_launch_order()
                r.render_async(cam, fov)
                assert np.array_equal(r.hybrid_launch_order(), got[1][0]) and np.array_equal(r.read_final_u8(), got[1][2])
                assert sorted(other.tolist()) == sorted(got[1][0].tolist())
            r.close()
        assert got[1][1] == got[0][1], (cam, fov, tilt, got[1][1], got[0][1])
        assert np.array_equal(got[1][0], got[0][0]), (cam, fov, tilt, int((got[1][0] != got[0][0]).sum()))
        assert np.array_equal(got[1][2], got[0][2])
        assert 0 < got[1][1] or np.linalg.norm(cam) > 3.0


def test_view_change_costs_a_tenth_of_a_millisecond_at_8k(hip_lib):
    """What moving the classification to the device is for: a camera path that changes its distance re-partitions the
    518 400 tiles of an 8k frame in front of every frame.  On the submitting thread that is ~50 ms of binary64 work; on the
    device the submit call returns in well under a millisecond (the wait for the strict count included)."""
    import time
    from bhr_amd import HipRenderer, scenes
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    kw = dict(step_size=0.3, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=0.0)
    cost = {}
    for where in (1, 0):
        r = HipRenderer(7680, 4320, sky, tex, math="hybrid", frame_slots=1, outputs="u8", options={"hybrid_classify": where}, **kw)
        r.render_async([6.0, 0.0, 0.5], 90.0)
        r.sync()
        same, moved = [], []
        for k in range(6):
            r.sync()
            t0 = time.perf_counter()
            r.render_async([6.0, 0.0, 0.5], 90.0)
            same.append(time.perf_counter() - t0)
            r.sync()
            t0 = time.perf_counter()
            r.render_async([6.0 + 0.01 * (k + 1), 0.0, 0.5], 90.0)
            moved.append(time.perf_counter() - t0)
        r.sync()
        r.close()
        cost[where] = (min(moved) - min(same)) * 1e3
    print(f"\n8k view change: device {cost[1]:.3f} ms, host {cost[0]:.3f} ms on the submit path")
    assert cost[1] <= 0.2 and cost[1] < cost[0] / 20, cost


def _frame_stats(a, b, chunk=256):
    """Per-channel RMSE of a - b and the per-pixel max |a - b| over channels, reduced in row chunks."""
    sq = np.zeros(3)
    dmax = np.empty(a.shape[:2], np.float32)
    for y in range(0, a.shape[0], chunk):
        d = a[y:y + chunk].astype(np.float64) - b[y:y + chunk]
        sq += (d * d).sum(axis=(0, 1))
        dmax[y:y + chunk] = np.abs(d).max(axis=2)
    return np.sqrt(sq / (a.shape[0] * a.shape[1])), dmax


def _hybrid_vs_strict(wl, variants):
    """The bench scene of wl on one frame_slots=1 context: the strict frame against the hybrid one under each
    hybrid_repair value of `variants`, layer by layer (at most three frame-sized f32 layers on the host at once).
    Returns {repair: dict(rmse={layer: per-channel RMSE}, beyond_1e3=pixels of the final layer beyond 1e-3, max=largest
    difference there, steps, strict_steps, info)}."""
    from bhr_amd import _lib, workloads
    r, _, _, _ = workloads.make_scene(wl, frame_slots=1)
    out = {rep: dict(rmse={}) for rep in variants}
    try:
        for name, layer in (("bg", _lib.LAYER_BG), ("disk", _lib.LAYER_DISK), ("blur", _lib.LAYER_BLUR), ("final", _lib.LAYER_FINAL)):
            r.set_option("hybrid_repair", -1)
            r.render_async(wl["cam_pos"], wl["fov"], math="strict")
            want, strict_steps = r.read_layer(layer), r.counters()["ray_steps"]
            for rep in variants:
                r.set_option("hybrid_repair", rep)
                r.render_async(wl["cam_pos"], wl["fov"], math="hybrid")
                got = r.read_layer(layer)
                o = out[rep]
                o["rmse"][name], d = _frame_stats(got, want)
                del got
                o.update(steps=r.counters()["ray_steps"], strict_steps=strict_steps, info=r.hybrid_info())
                if name == "final":
                    o.update(beyond_1e3=int((d > 1e-3).sum()), max=float(d.max()))
            del want
    finally:
        r.close()
    return out


_WHOLE = {}


def _whole_frame(W, H, step, variants=(-1,)):
    """_hybrid_vs_strict on the bench scene at W x H, cached for the tests of this module that read the same frames."""
    import bench
    key = (W, H, step, tuple(variants))
    if key not in _WHOLE:
        _WHOLE[key] = _hybrid_vs_strict(dict(bench.WORKLOADS["fhd"], width=W, height=H, step_size=step), variants)
        for rep, o in _WHOLE[key].items():
            print(f"\n[hybrid {W}x{H} step {step}, repair {rep}] strict tiles {o['info']['strict_tiles']} of {o['info']['tiles']}, "
                  f"repaired {o['info']['repaired_pixels']}; pixels beyond 1e-3: {o['beyond_1e3']}, max {o['max']:.3g}; steps "
                  f"{o['steps']} vs {o['strict_steps']}; worst-channel RMSE " + ", ".join(f"{k} {float(v.max()):.3g}" for k, v in o["rmse"].items()))
    return _WHOLE[key]


def _check_whole(o, known, tag):
    """Steps within 2e-4 of strict; every layer's worst-channel RMSE, the final layer's pixels beyond 1e-3 and its largest
    difference within `known` (measured ceilings of the bars a frame is known to miss) or else the certified bars."""
    assert abs(o["steps"] - o["strict_steps"]) <= 2e-4 * o["strict_steps"], (tag, o["steps"], o["strict_steps"])
    for k, e in o["rmse"].items():
        assert float(e.max()) <= known.get(k, MARGIN), (tag, k, e)
    assert o["beyond_1e3"] <= known["beyond_1e3"] and o["max"] <= known["max"], (tag, o["beyond_1e3"], o["max"])


# Measured on the 8k frame (7680 x 4320, step 0.05, bench scene): the differing pixels lie at b - b_c = 0.5 ... 2.1, outside the
# strict band (whose classification is sound and exact there: test_gpu_hybrid_band.py) -- the fast arithmetic's rounding on
# the 8k frame's finer disk texture, and with the guards off (the default at tilt 0) disk-colour flips at the algorithm's
# own switches.  Ceilings a little above the measured values, so that a regression turns red.
# guards off: 603 pixels beyond 1e-3, max 0.485, RMSE disk 2.0e-4, final 1.6e-4 (bg 1.4e-5, blur 1.5e-6 hold the margin);
# guards on (16 812 pixels repaired): 589 pixels beyond 1e-3, max 0.013, RMSE disk 4.2e-5, final 3.2e-5 (bg 5.5e-6, blur 6.7e-7)
KNOWN_8K = {-1: dict(disk=2.5e-4, final=2.0e-4, beyond_1e3=700, max=0.5),
            1: dict(disk=5e-5, final=4e-5, beyond_1e3=700, max=0.016)}


def test_hybrid_whole_8k_frame_vs_strict(hip_lib):
    """BASELINE.json configs[3] (7680 x 4320, step 0.05: the bench's row-block workload) under hybrid, whole frame against
    strict on one context, with the guards at their default (off at tilt 0) and forced on (hybrid_repair 1): ray-step
    totals within 2e-4, bg and blur RMSE <= 3e-5 per channel, disk / final RMSE and the final layer's single pixels within
    the measured ceilings of KNOWN_8K (the certified bars they miss: the xfail tests below); the guards repair pixels only
    when on; strict tiles a small share.  The 8k ring tiles span ~0.02 r_s of b, a quarter of fhd's: tile_pad pads them least."""
    res = _whole_frame(7680, 4320, 0.05, (-1, 1))
    for rep, o in res.items():
        _check_whole(o, KNOWN_8K[rep], f"8k repair {rep}")
        assert (o["info"]["repaired_pixels"] > 0) == (rep == 1), (rep, o["info"])
    assert res[-1]["info"]["strict_tiles"] / res[-1]["info"]["tiles"] <= 0.12, res[-1]["info"]


@pytest.mark.xfail(strict=True, raises=AssertionError, reason="measured RMSE from strict: guards off disk 2.0e-4, final 1.6e-4 "
                   "(beyond the 1e-4 north star); guards on disk 4.2e-5, final 3.2e-5 -- from pixels outside the strict band (KNOWN_8K)")
@pytest.mark.parametrize("repair", [-1, 1])
def test_hybrid_whole_8k_frame_within_the_certified_margin(repair, hip_lib):
    """The certified bar on the 8k frame, guards at their default and forced on: every layer within 3e-5 per channel of strict."""
    o = _whole_frame(7680, 4320, 0.05, (-1, 1))[repair]
    for k, e in o["rmse"].items():
        assert (e <= MARGIN).all(), (k, e)


@pytest.mark.xfail(strict=True, raises=AssertionError, reason="measured: the guarded 8k frame keeps 589 pixels beyond 1e-3 "
                   "of strict (max 0.013), outside the strict band (KNOWN_8K)")
def test_hybrid_guarded_8k_frame_has_no_pixel_beyond_1e_3(hip_lib):
    """The guarded fhd frame's bar at 8k: with hybrid_repair 1, no pixel of the final layer beyond 1e-3 of strict."""
    o = _whole_frame(7680, 4320, 0.05, (-1, 1))[1]
    assert o["beyond_1e3"] == 0, (o["beyond_1e3"], o["max"])


# The tile-span sweep, default guards.  Measured misses of the certified bars (RMSE <= 3e-5, no pixel beyond 2e-2, pixels
# beyond 1e-3 at the fhd rate), all from pixels far outside the band (b - b_c >= 0.4): 3840 x 2160 disk RMSE 6.5e-5 (max 0.067,
# 9 pixels beyond 1e-3); 512 x 288 and 1366 x 766 one mirror pair each of disk-colour flips at b - b_c = 1.4 / 1.7 (max 0.24 /
# 0.26; RMSE disk 8.6e-4 / 3.3e-4, final 8.7e-4 / 3.2e-4, blur 8.6e-5 at 512 x 288, whose bloom spreads the pair over 142 pixels
# beyond 1e-3).  Ceilings a little above the measured values; the other sizes meet the bars.
SWEEP = [(h * 16 // 9, h) for h in (2160, 1080, 720, 540, 432, 360, 288, 216)] + [(1366, 766)]
KNOWN_SWEEP = {(3840, 2160): dict(disk=8e-5, beyond_1e3=12, max=0.08),
               (512, 288): dict(disk=1.1e-3, final=1.1e-3, blur=1.1e-4, beyond_1e3=170, max=0.28),
               (1366, 766): dict(disk=4e-4, final=4e-4, max=0.3)}


def _fhd_bars(W, H):
    return dict(beyond_1e3=max(4, int(4 * W * H / 2073600)), max=2e-2)


@pytest.mark.parametrize("W,H", SWEEP, ids=[f"{w}x{h}" for w, h in SWEEP])
def test_hybrid_whole_frames_vs_strict_across_tile_spans(W, H, hip_lib):
    """The default pov from 216 to 2160 rows: the ring tiles' span of b crosses tile_pad's 0.1 and 0.2 r_s regimes.  Whole
    frame hybrid (default guards) vs strict: steps within 2e-4; RMSE <= 3e-5 per channel, no pixel beyond 2e-2, pixels
    beyond 1e-3 at most at the fhd frame's rate (4 per 2 073 600, and at least 4) -- or, for the sizes known to miss one of
    these, within its measured ceiling (KNOWN_SWEEP; the certified bars themselves: the xfail test below)."""
    o = _whole_frame(W, H, 0.1)[-1]
    _check_whole(o, dict(_fhd_bars(W, H), **KNOWN_SWEEP.get((W, H), {})), f"{W}x{H}")


@pytest.mark.xfail(strict=True, raises=AssertionError, reason="measured misses of the certified bars, pixels outside the strict band (KNOWN_SWEEP)")
@pytest.mark.parametrize("W,H", sorted(KNOWN_SWEEP), ids=[f"{w}x{h}" for w, h in sorted(KNOWN_SWEEP)])
def test_hybrid_whole_frames_across_tile_spans_meet_the_certified_bars(W, H, hip_lib):
    o = _whole_frame(W, H, 0.1)[-1]
    _check_whole(o, _fhd_bars(W, H), f"{W}x{H}")


def test_hybrid_8k_row_bands_match_oracle(oracle, hip_lib):
    """configs[3] under hybrid against the oracle on rows where a misclassified tile would show: the midline, the 8-row
    tile bands where the ring b = b_c touches the tile rows at its top and bottom, and one through b = b_c + hi.  The bars
    of the fhd whole frame (test_gpu_fullsize.test_hybrid_whole_frames_match_oracle): RMSE <= 3e-5 per channel, at most 4
    pixels beyond 1e-3, none beyond 2e-2."""
    import hybrid_band as hb
    from bhr_amd import HipRenderer, _lib, scenes
    W, H = 7680, 4320
    cam, fov = [6.0, 0.0, 0.5], 90.0
    kw = dict(step_size=0.05, r_max=10.0, r_disk_inner=2.0, r_disk_outer=15.0, disk_tilt=0.0, anti_alias="disabled")
    u = hb.uniforms(cam, fov, W, H)
    lo, hi = hb.effective_band(kw["step_size"])
    ys = np.arange(H)
    b = np.array([hb.pixel_geometry(u, W, H, y, y + 1)["b"][0].min() for y in ys[::8]])      # min of b along a row, every 8th row
    inside = np.nonzero(b < hb.B_CRIT)[0]
    top, bot = int(inside.min()) * 8, int(inside.max()) * 8
    # refine to the exact first / last row whose minimum b is below b_c, and take its tile band
    top = next(y for y in range(max(0, top - 8), top + 9) if hb.pixel_geometry(u, W, H, y, y + 1)["b"].min() < hb.B_CRIT)
    bot = next(y for y in range(min(H - 1, bot + 8), bot - 9, -1) if hb.pixel_geometry(u, W, H, y, y + 1)["b"].min() < hb.B_CRIT)
    outer = int(np.nonzero(b < hb.B_CRIT + hi)[0].min()) * 8
    bands = [(2158, 2162), (top // 8 * 8, top // 8 * 8 + 8), (bot // 8 * 8, bot // 8 * 8 + 8), (outer // 8 * 8, outer // 8 * 8 + 8)]
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk(256, 1024)
    hip = HipRenderer(W, H, sky, tex, math="hybrid", frame_slots=1, **kw)
    hip.render_async(cam, fov, skip_bloom=True)
    lay = {"bg": hip.read_layer(_lib.LAYER_BG), "disk": hip.read_layer(_lib.LAYER_DISK)}
    info = hip.hybrid_info()
    hip.close()
    assert (info["band_below"], info["band_above"]) == (lo, hi), info
    ora = oracle.OracleRenderer(W, H, sky, tex, **kw)
    for (r0, r1) in bands:
        rbg, rdisk = ora.march(cam, fov, rows=(r0, r1), want_steps=False, skip_differentials=True)
        ref = {"bg": rbg.transpose(1, 0, 2)[r0:r1], "disk": rdisk.transpose(1, 0, 2)[r0:r1]}
        for k in ("bg", "disk"):
            e, d = _frame_stats(lay[k][r0:r1], ref[k])
            print(f"\n[hybrid 8k vs oracle, rows {r0}-{r1} {k}] RMSE {e}, max {d.max():.3g}, pixels > 1e-3: {int((d > 1e-3).sum())}")
            assert (e <= MARGIN).all() and (d > 1e-3).sum() <= 4 and d.max() <= 2e-2, ((r0, r1), k, e, float(d.max()), int((d > 1e-3).sum()))
