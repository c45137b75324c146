"""--spin_line / --spin_g_map on the command line and in the drivers: the flags, their defaults and value checks, every row of
rules.FEATURES["kerr_line"] in order and with the same words on both surfaces, the keyword reaching the drivers only when it is set,
the .npz's keys and shapes through a stand-in renderer, and the redshift map's colours on a synthetic g plane."""
import contextlib
import io

import numpy as np
import pytest

from bhr_amd import cli, drivers, line, rules

BASE = ["--spin", "0.9"]
LINE = BASE + ["--spin_line", "l.npz"]
ROWS = ("no_spin video_no_spin_map video_orbit shutter supersample_or_threshold spin_map_supersample spin_shutter_map spin_observer spin_projection "
        "kerr_anti_alias kerr_disk_model gpus_or_world kerr_line_not_npz g_map_not_png g_map_video").split()


def _error(argv):
    err = io.StringIO()
    with contextlib.redirect_stderr(err), pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2
    return err.getvalue()


def test_flags_parse_and_reach_the_drivers_as_one_dict():
    args = cli.parse_args(LINE)
    assert args.spin_line == "l.npz" and cli.kerr_line_from_args(args) == dict(kerr_line=dict(path="l.npz", g_map_path=None))
    args = cli.parse_args(LINE + ["--spin_line_bins", "1000", "--spin_line_range", "0.2", "1.4", "--spin_line_index", "2.5", "--spin_line_emissivity", "texture",
                                  "--spin_line_orders", "all", "--spin_line_energy", "6.7", "--spin_g_map", "g.png"])
    assert cli.kerr_line_from_args(args)["kerr_line"] == dict(path="l.npz", g_map_path="g.png", n_bins=1000, g_range=(0.2, 1.4), index=2.5, emissivity="texture",
                                                              orders="all", energy_kev=6.7)
    for argv in (LINE + ["--spin_polarization", "toroidal"], LINE + ["--spin_stars", "point"], LINE + ["--spin_passes", "p.npz"],
                 LINE + ["--video", "--spin_map"], ["--redshift", "exact", "--spin_g_map", "g.png"], LINE + ["--redshift", "exact", "--lens_flare"]):
        cli.parse_args(argv)
    checked = drivers._checked_kerr_line(dict(path="l.npz"), dict(spin=0.9, kerr_line=True, kerr_line_path="l.npz"))
    assert checked["settings"] == line.DEFAULTS and checked["energy_kev"] == 6.4 and checked["g_map_path"] is None
    assert line.DEFAULTS["n_bins"] == 256 and line.DEFAULTS["g_range"] == (0.0, 2.0) and line.DEFAULTS["index"] == 3.0 and line.DEFAULTS["power"] == 4.0
    assert line.DEFAULTS["emissivity"] == "powerlaw" and line.DEFAULTS["orders"] == "first"


def test_a_line_without_the_flags_has_the_namespace_it_had():
    for argv in ([], BASE, BASE + ["--video", "--spin_map"], BASE + ["--spin_passes", "p.npz"]):
        ns = vars(cli.parse_args(argv))
        assert not any("spin_line" in k or "g_map" in k or "kerr_line" in k for k in ns), sorted(ns)
        assert cli.kerr_line_from_args(cli.parse_args(argv)) == {}
    assert rules.FACTS["kerr_line"] is False and rules.FACTS["kerr_line_path"] is None and rules.FACTS["g_map_path"] is None


@pytest.mark.parametrize("argv, word", [
    (LINE + ["--spin_line_bins", "0"], "n_bins"), (LINE + ["--spin_line_bins", "4097"], "n_bins"), (LINE + ["--spin_line_range", "1", "1"], "range"),
    (LINE + ["--spin_line_range", "2", "0"], "range"), (LINE + ["--spin_line_index", "-1"], "index"), (LINE + ["--spin_line_index", "17"], "index"),
    (LINE + ["--spin_line_energy", "0"], "--spin_line_energy"), (LINE + ["--spin_line_emissivity", "flat"], "--spin_line_emissivity"),
    (LINE + ["--spin_line_orders", "second"], "--spin_line_orders"), (BASE + ["--spin_line_bins", "64"], "needs --spin_line"),
    (BASE + ["--spin_line_energy", "6.7"], "needs --spin_line")])
def test_value_checks(argv, word):
    assert word in _error(argv)


REFUSED = [
    (["--spin_line", "l.npz"], "needs --spin"),
    (LINE + ["--video"], "--spin_map"),
    (LINE + ["--video", "--spin_map", "--orbit"], "--orbit"),
    (LINE + ["--supersample", "2"], "--supersample"),
    (LINE + ["--video", "--spin_map", "--spin_map_supersample", "2"], "--spin_map_supersample"),
    (LINE + ["--video", "--shutter", "0.5", "--spin_shutter_map"], "--shutter"),
    (LINE + ["--spin_observer", "zamo"], "--spin_observer"),
    (LINE + ["--spin_projection", "fisheye"], "--spin_projection"),
    (LINE + ["--spin_anti_alias", "lod_radius"], "--spin_anti_alias"),
    (LINE + ["--spin_disk_model", "v2"], "--spin_disk_model"),
    (LINE + ["--gpus", "2"], "--gpus"),
    (BASE + ["--spin_line", "l.txt"], ".npz"),
    (LINE + ["--spin_g_map", "g.jpg"], ".png"),
    (LINE + ["--video", "--spin_map", "--spin_g_map", "g.png"], "--spin_g_map"),
]


@pytest.mark.parametrize("argv, word", REFUSED, ids=lambda v: "_".join(w.strip("-") for w in v[2:]) if isinstance(v, list) else None)
def test_the_command_line_refuses(argv, word):
    assert word in _error(argv)


def test_every_row_in_order_with_the_same_words_on_both_surfaces():
    assert rules.FEATURES["kerr_line"]["rows"].split() == ROWS
    ok = dict(kerr_line=True, spin=0.9, kerr_line_path="l.npz", g_map_path="g.png")
    assert rules.refusal("kerr_line", ok) is None and rules.refusal("kerr_line", dict(ok, spin=0.0, redshift="exact")) is None
    assert rules.refusal("kerr_line", dict(ok, g_map_path=None, video=True, spin_map=True)) is None
    for beside in (dict(kerr_polarization=True), dict(kerr_stars=True), dict(kerr_passes_path="p.npz")):
        assert rules.refusal("kerr_line", dict(ok, **beside)) is None
    # each row's facts violate that row and every later one they can: the first refusal is the row's own
    cases = [
        (dict(ok, spin=0.0), "needs --spin"), (dict(ok, video=True, g_map_path=None), "needs --spin_map"),
        (dict(ok, video=True, spin_map=True, orbit=True), "--orbit"), (dict(ok, shutter=0.5, supersample=2), "--shutter"),
        (dict(ok, supersample=2, spin_map_supersample=2), "--supersample other than 1"), (dict(ok, supersample_threshold=0.1), "--supersample other than 1"),
        (dict(ok, spin_map_supersample=2, spin_shutter_map=True), "--spin_map_supersample"), (dict(ok, spin_shutter_map=True, spin_observer=True), "--spin_shutter_map"),
        (dict(ok, spin_observer=True, spin_projection=True), "--spin_observer"), (dict(ok, spin_projection=True, kerr_anti_alias=True), "--spin_projection"),
        (dict(ok, kerr_anti_alias=True, kerr_disk_model="v2"), "--spin_anti_alias"), (dict(ok, kerr_disk_model="v2_volume", gpus=2), "--spin_disk_model"),
        (dict(ok, gpus=2, kerr_line_path="l.txt"), "--gpus"), (dict(ok, world=2), "ranks"), (dict(ok, kerr_line_path="l.txt", g_map_path="g.jpg"), "--spin_line writes a .npz"),
        (dict(ok, g_map_path="g.jpg", video=True, spin_map=True), "--spin_g_map writes a .png"), (dict(ok, video=True, spin_map=True), "does not combine with --video")]
    assert len(cases) == len(ROWS) + 2                                     # supersample_or_threshold and gpus_or_world twice
    for facts, word in cases:
        text = rules.refusal("kerr_line", facts)
        assert text is not None and word in text, (facts, text)
        assert rules.refusal("kerr_line", facts, "cli") == text
    rules.refuse_on("kerr_line", dict(spin=0.0, gpus=2))                   # off: nothing to refuse


class _Reached(Exception):
    pass


def test_the_drivers_refuse_before_the_device(monkeypatch, tmp_path):
    def no_device(*a, **kw):
        raise _Reached()
    monkeypatch.setattr(drivers, "make_renderer", no_device)
    args = dict(width=32, height=16, cam_pos=[6, 0, 0.5], fov=90, step_size=0.1)
    with pytest.raises(ValueError, match="needs --spin"):
        drivers.render_image(**args, kerr_line=dict(path="l.npz"))
    with pytest.raises(ValueError, match="--spin_disk_model"):
        drivers.render_image(**args, spin=0.9, kerr_line=dict(path="l.npz"), kerr_disk_model="v2")
    with pytest.raises(ValueError, match="n_bins"):
        drivers.render_image(**args, spin=0.9, kerr_line=dict(path="l.npz", n_bins=5000))
    with pytest.raises(ValueError, match="unknown settings"):
        drivers.render_image(**args, spin=0.9, kerr_line=dict(path="l.npz", bins=64))
    with pytest.raises(ValueError, match="nothing to write"):
        drivers.render_image(**args, spin=0.9, kerr_line=dict(n_bins=64))
    with pytest.raises(_Reached):
        drivers.render_image(**args, spin=0.9, kerr_line=dict(path="l.npz"), kerr_passes_path="p.npz")

    class Fake:
        spin, redshift, supersample, supersample_threshold, disk_tilt, anti_alias, _dv2, _kerr_anti_alias = 0.9, "model", 1, None, 0.0, "disabled", None, None

        def __getattr__(self, name):
            raise _Reached()
    video = dict(width=8, height=8, n_frames=2, fps=24, output_path=str(tmp_path / "v.mp4"), fov=90.0, static_cam_pos=[6.0, 0.0, 0.5])
    with pytest.raises(ValueError, match="needs --spin_map"):
        drivers.render_video(Fake(), **video, kerr_line=dict(path="l.npz"))
    with pytest.raises(ValueError, match="--orbit"):
        drivers.render_video(Fake(), **video, spin_map=True, orbit=True, kerr_line=dict(path="l.npz"))
    with pytest.raises(ValueError, match="--resume"):
        drivers.render_video(Fake(), **video, spin_map=True, resume=True, kerr_line=dict(path="l.npz"))


def test_main_hands_the_line_to_the_drivers_only_when_it_is_set(monkeypatch):
    calls = []
    monkeypatch.setattr(drivers, "render_image", lambda **kw: calls.append(kw) or np.zeros((2, 2, 3), np.float32))
    monkeypatch.setattr(drivers, "save_image", lambda *a, **kw: None)
    with contextlib.redirect_stdout(io.StringIO()):
        cli.main(BASE)
        cli.main(LINE + ["--spin_line_bins", "64", "--spin_g_map", "g.png"])
    assert "kerr_line" not in calls[0]
    assert calls[1]["kerr_line"] == dict(path="l.npz", g_map_path="g.png", n_bins=64)


class _StandIn:
    """What _save_kerr_line and HipRenderer.kerr_line ask of a renderer, from rows made here."""
    def __init__(self, counts, settings):
        self.counts, self.settings = counts, settings

    def kerr_line(self, first_row=0, n_rows=None, energy_kev=6.4):
        c = self.counts[first_row] if n_rows is None else self.counts[first_row:first_row + n_rows]
        z = np.zeros(c.shape[:-1], dtype=np.uint64)
        return line.profile(c, z, z + np.uint64(3), self.settings, 0.9, "exact", energy_kev)

    def kerr_line_info(self, row=0):
        return dict(samples=17, overflow_pixels=2)


def test_the_npz_s_keys_and_shapes(tmp_path):
    s = line.check_settings(n_bins=8, g_range=(0.0, 2.0))
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 1 << 40, size=(5, 8)).astype(np.uint64)
    counts[:, :2] = 0
    counts[:, 7] = 0
    still, video = str(tmp_path / "still.npz"), str(tmp_path / "video.npz")
    with contextlib.redirect_stdout(io.StringIO()):
        drivers._save_kerr_line(_StandIn(counts, s), dict(path=still, energy_kev=6.4))
        drivers._save_kerr_line(_StandIn(counts, s), dict(path=video, energy_kev=6.7), 5)
    keys = {"edges", "flux", "counts", "under", "over", "g_mean", "g_red", "g_blue", "energy", "energy_kev", "spin", "redshift", "n_bins", "g_min", "g_max",
            "index", "power", "emissivity", "orders", "r_inner", "r_outer"}
    a, b = np.load(still), np.load(video)
    assert set(a.files) == keys and set(b.files) == keys
    assert a["flux"].shape == (8,) and a["counts"].shape == (8,) and a["edges"].shape == (9,) and a["energy"].shape == (8,) and a["g_mean"].shape == ()
    assert b["flux"].shape == (5, 8) and b["counts"].shape == (5, 8) and b["g_mean"].shape == (5,) and b["under"].shape == (5,) and b["over"].shape == (5,)
    assert a["counts"].dtype == np.uint64 and np.array_equal(b["counts"], counts) and int(a["over"]) == 3
    assert float(a["g_red"]) == 0.5 and float(a["g_blue"]) == 1.75 and 0.5 < float(a["g_mean"]) < 1.75
    assert np.allclose(a["energy"], 6.4 * (np.arange(8) + 0.5) * 0.25) and float(b["energy_kev"]) == 6.7 and str(b["redshift"]) == "exact"
    # the host turns a row into flux: Q / unit / bin width
    assert np.array_equal(a["flux"], counts[0].astype(np.float64) / float(np.float32(2.0 ** 32 / 1.5 ** 4)) / 0.25)
    empty = line.moments(line.edges_of(8, (0.0, 2.0)), np.zeros(8, dtype=np.uint64))
    assert all(np.isnan(v) for v in empty.values())
    with pytest.raises(ValueError, match=".npz"):
        line.save_npz(str(tmp_path / "l.txt"), line.profile(counts[0], 0, 0, s, 0.9, "model"))


def test_the_colour_map():
    g = np.array([1.0, np.nan, 0.0, -1.0, 0.2, 0.5, 0.9, 1.1, 1.3, 1.5, 3.0])
    c = line.g_colors(g).astype(int)
    assert c.shape == (11, 3) and line.g_colors(g).dtype == np.uint8
    assert tuple(c[0]) == (255, 255, 255)                                   # g = 1: neutral
    assert not c[1].any() and not c[2].any() and not c[3].any()             # NaN, 0, negative: black
    red, blue = c[4:7], c[7:10]
    assert (red[:, 0] == 255).all() and (np.diff(red[:, 1]) > 0).all() and (np.diff(red[:, 2]) > 0).all() and (red[:, 1] == red[:, 2]).all()    # redder as g falls
    assert (blue[:, 2] == 255).all() and (np.diff(blue[:, 0]) < 0).all() and (blue[:, 0] == blue[:, 1]).all()                                 # bluer as g rises
    assert tuple(c[9]) == tuple(c[10]) == (0, 0, 255)                       # saturates at the g-factor's cap
    planes = np.zeros((3, 2, 2), dtype=np.float32)
    planes[1, 0, 0], planes[2, 0, 0], planes[0, 1, 1] = 0.7, 1.2, 1.1
    first = line.first_g(planes)
    assert first[0, 0] == np.float32(0.7) and first[1, 1] == np.float32(1.1) and first[0, 1] == 0 and first[1, 0] == 0
