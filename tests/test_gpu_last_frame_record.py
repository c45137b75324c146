"""What bhr_get_counters, bhr_get_row_costs* and bhr_adaptive_info report about "the last frame" while the kinds of frame
alternate on ONE context (bhr_last_frame, csrc/bhr_internal.h): rays, ray_steps and frames_timed after render / shutter /
adaptive / ray-map / fused ray-map shutter / row-cost frames, what a refused call leaves, and group renders with and without
BHR_GROUP_TIME_MARCH.  The same sequence runs once on a one-slot and once on a two-slot context; the tests read its log.

96 x 54 under the hybrid arithmetic: the smallest frame of the suite with a disk, a shadow and strict-band tiles in view.

With adaptive supersampling set every frame of a context is adaptive (ray maps, group and tile renders are refused), so no
sequence lets a frame of another kind follow an adaptive one without a change of the sampling, which resets bhr_adaptive_info:
what is pinned here is that a REFUSED ray-map frame behind an adaptive frame leaves bhr_adaptive_info and the counters alone."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, CAM, FOV, T = 96, 54, (6.0, 0.0, 0.5), 90.0, 0.25
TIMES = ("march_ms", "bloom_ms", "frame_ms", "background_ms", "compose_ms", "march_ms_sum", "bloom_ms_sum", "march_busy_ms", "span_ms")


def _mk(**kw):
    from bhr_amd import HipRenderer, scenes
    return HipRenderer(W, H, scenes.analytic_skybox(), scenes.noisy_disk(), math="hybrid", **kw)


def _samples(n):
    """Sample j: the camera turned by j / 7 of a 10 degree arc, with a t_offset of its own (as tests/test_gpu_shutter.py)."""
    x, y, z = CAM
    pos = [[x * math.cos(a) - y * math.sin(a), x * math.sin(a) + y * math.cos(a), z] for a in (math.radians(10.0) * j / 7 for j in range(n))]
    return pos, [0.3 + 0.17 * j for j in range(n)]


def _render(r, pos=CAM, t_offset=0.0):
    from bhr_amd import _lib
    cam = r.camera_uniforms(list(pos), FOV, t_offset=t_offset)
    _lib.check(r._lib.bhr_render(r._ctx, C.byref(cam), 0))


def _counts(c):
    return {k: v for k, v in c.items() if k not in TIMES}


def _row_costs_rc(r):
    """Return codes of bhr_get_row_costs and bhr_get_row_costs_split with the right band count."""
    n = (H + 7) // 8
    a, b = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))
    return r._lib.bhr_get_row_costs(r._ctx, p(a), n), r._lib.bhr_get_row_costs_split(r._ctx, p(a), p(b), n)


@functools.lru_cache(maxsize=None)
def _single_steps():
    """ray_steps of the three shutter samples rendered one by one, on a context of their own."""
    r = _mk()
    out = []
    for p, t in zip(*_samples(3)):
        _render(r, p, t)
        out.append(r.counters()["ray_steps"])
    r.close()
    return out


_RUNS = {}


def _sequence(slots):
    """The log of _run_sequence(slots), run ONCE per slot count: a failure is kept and raised again for every test that
    reads the log, never run a second time on the device."""
    if slots not in _RUNS:
        try:
            _RUNS[slots] = _run_sequence(slots)
        except BaseException as e:
            _RUNS[slots] = e
    if isinstance(_RUNS[slots], BaseException):
        raise _RUNS[slots]
    return _RUNS[slots]


def _run_sequence(slots):
    """The frame kinds in turn on one context; the counters (and what else a test needs) after each step, by name."""
    r = _mk(frame_slots=slots)
    log = {}

    def note(name, **extra):
        log[name] = dict(c=r.counters(), **extra)

    _render(r)
    note("render")
    pos, toff = _samples(3)
    r.render_shutter_async(pos, FOV, toff)
    note("shutter")
    _render(r)
    note("render_again")
    # adaptive, a refused ray-map frame behind it, then plain again
    r.set_supersample(2, T)
    _render(r)
    note("adaptive", ada=r.adaptive_info())
    rc = r._lib.bhr_raymap_render(r._ctx, 0.3, 0)
    note("adaptive_refused_map", rc=rc, ada=r.adaptive_info())
    r.set_supersample(1)
    _render(r)
    note("plain_after_adaptive", ada_rc=r._lib.bhr_adaptive_info(r._ctx, (C.c_int64 * 3)()))
    # ray-map frames: a map with overflow pixels (one slot), then one without (fused shutter)
    r.set_option("raymap_slots", 1)
    r.build_ray_map(list(CAM), FOV)
    r.render_from_ray_map_async(t_offset=0.3)
    note("map", info=r.ray_map_info(), passes=r.ray_map_passes())
    r.set_option("raymap_slots", 4)
    r.build_ray_map(list(CAM), FOV)
    r.render_shutter_from_ray_map_async([0.3 + 0.17 * j for j in range(4)])
    note("map_shutter", info=r.ray_map_info())
    _render(r)
    note("plain_after_map")
    # row costs, then a plain frame
    both = r.row_costs(list(CAM), FOV)
    fast, strict = r.row_costs(list(CAM), FOV, split=True)
    note("row_costs", both=both, fast=fast, strict=strict)
    _render(r)
    note("plain_after_row_costs", rcs=_row_costs_rc(r))
    # a refused call that launches nothing
    cam = r.camera_uniforms(list(CAM), FOV)
    rc = r._lib.bhr_render_shutter(r._ctx, C.byref(cam), 0, 0)           # 0 samples
    note("refused", rc=rc)
    r.close()
    return log


SLOTS = (1, 2)


@pytest.mark.parametrize("slots", SLOTS)
def test_render_shutter_render(slots, hip_lib):
    s = _sequence(slots)
    a, b, c = s["render"]["c"], s["shutter"]["c"], s["render_again"]["c"]
    assert a["rays"] == W * H and a["ray_steps"] > 0 and a["frames_timed"] == 1
    assert b["rays"] == 3 * W * H
    assert b["ray_steps"] == sum(_single_steps())
    assert b["frames_timed"] == a["frames_timed"] + 1
    assert b["march_ms"] > 0 and b["frame_ms"] >= b["march_ms"]
    assert c["rays"] == W * H and c["ray_steps"] == a["ray_steps"] and c["frames_timed"] == 3


@pytest.mark.parametrize("slots", SLOTS)
def test_adaptive_then_plain(slots, hip_lib):
    from bhr_amd import _lib
    s = _sequence(slots)
    ada = s["adaptive"]["ada"]
    assert 0 < ada["refined"] < W * H and ada["pixels"] == W * H
    assert s["adaptive"]["c"]["rays"] == W * H + 4 * ada["refined"]
    # a ray-map frame is refused while supersampling is on: the adaptive frame stays the one on record, in every field
    assert s["adaptive_refused_map"]["rc"] == _lib.BHR_ERR_STATE
    assert s["adaptive_refused_map"]["ada"] == ada
    assert s["adaptive_refused_map"]["c"] == s["adaptive"]["c"]            # the whole dict: the times are the same events' read again
    plain = s["plain_after_adaptive"]
    assert plain["c"]["rays"] == W * H and plain["c"]["ray_steps"] == s["render"]["c"]["ray_steps"]
    assert plain["ada_rc"] == _lib.BHR_ERR_STATE


@pytest.mark.parametrize("slots", SLOTS)
def test_ray_map_frames(slots, hip_lib):
    s = _sequence(slots)
    m, p = s["map"], s["map"]["passes"]
    over = p["crossings"] > 1
    assert m["info"]["overflow_pixels"] == int(over.sum()) > 0
    assert m["c"]["rays"] == W * H
    assert m["c"]["ray_steps"] == int(p["steps"][over].sum())            # the overflow re-march only
    assert m["c"]["frames_timed"] == s["plain_after_adaptive"]["c"]["frames_timed"] + 1
    f = s["map_shutter"]
    assert f["info"]["overflow_pixels"] == 0                              # so the shutter frame took the fused launch
    assert f["c"]["rays"] == 4 * W * H and f["c"]["ray_steps"] == 0
    assert f["c"]["frames_timed"] == m["c"]["frames_timed"] + 1
    assert f["c"]["march_ms"] > 0 and f["c"]["frame_ms"] >= f["c"]["march_ms"]
    back = s["plain_after_map"]["c"]
    assert back["rays"] == W * H and back["ray_steps"] == s["render"]["c"]["ray_steps"]


@pytest.mark.parametrize("slots", SLOTS)
def test_row_costs(slots, hip_lib):
    from bhr_amd import _lib
    s = _sequence(slots)
    rc = s["row_costs"]
    assert rc["both"].sum() > 0 and rc["fast"].sum() > 0 and rc["strict"].sum() > 0      # a hybrid frame fills both profiles
    np.testing.assert_array_equal(rc["both"], rc["fast"] + rc["strict"])
    assert s["plain_after_row_costs"]["rcs"] == (_lib.BHR_ERR_STATE, _lib.BHR_ERR_STATE)
    assert s["plain_after_row_costs"]["c"]["rays"] == W * H


@pytest.mark.parametrize("slots", SLOTS)
def test_refused_frame_leaves_every_counter(slots, hip_lib):
    from bhr_amd import _lib
    s = _sequence(slots)
    assert s["refused"]["rc"] == _lib.BHR_ERR_INVALID
    # the whole dict, times included: they are the same events' and the same ring's read again
    assert s["refused"]["c"] == s["plain_after_row_costs"]["c"]


def test_one_slot_against_two(hip_lib):
    one, two = _sequence(1), _sequence(2)
    assert list(one) == list(two)
    for name in one:
        assert _counts(one[name]["c"]) == _counts(two[name]["c"]), name
    assert one["adaptive"]["ada"] == two["adaptive"]["ada"]


def test_group_renders(hip_lib):
    """Two row-block contexts on one device, each after a frame of its own: a group render reports the scalar events and cell."""
    from bhr_amd import HipRenderer, multigpu, scenes
    sky, tex = scenes.analytic_skybox(), scenes.noisy_disk()
    cut = 24
    tiles = [HipRenderer(W, H, sky, tex, math="hybrid", rows=rows) for rows in ((0, cut), (cut, H))]
    for t in tiles:
        t.render_async(list(CAM), FOV, skip_bloom=True)              # a frame of the tile's own: a ring slot on record
        c = t.counters()
        assert c["frames_timed"] == 1 and c["march_ms"] > 0 and c["rays"] == W * t.rows
    own = [t.counters() for t in tiles]
    multigpu.group_render(tiles, list(CAM), FOV, gather="peer")
    for t, before in zip(tiles, own):
        c = t.counters()
        assert c["march_ms"] == -1 and c["bloom_ms"] == -1 and c["frame_ms"] > 0
        assert c["rays"] == W * t.rows and c["ray_steps"] > 0 and c["frames_timed"] == before["frames_timed"]
    untimed = [t.counters()["ray_steps"] for t in tiles]
    multigpu.group_render(tiles, list(CAM), FOV, gather="peer", time_march=True)
    for t, steps in zip(tiles, untimed):
        c = t.counters()
        assert c["march_ms"] > 0 and c["bloom_ms"] >= 0 and c["frame_ms"] >= c["march_ms"]
        assert c["rays"] == W * t.rows and c["ray_steps"] == steps
    for t in tiles:
        t.close()
