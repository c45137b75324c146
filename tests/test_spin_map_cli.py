"""--spin_map on the command line and in the drivers: it parses and reaches render_video, every refusal names --spin_map and the
flag it does not go with before any device is touched, and a line without it parses to the namespace it always did.  No GPU."""
import pytest

from bhr_amd import cli, drivers

BASE = ["--spin", "0.7", "--video", "--spin_map"]


def _run_main(monkeypatch, argv):
    seen = {}

    def make_renderer(*a, **kw):
        seen["renderer"] = kw
        return object(), None, None, None

    def render_video(renderer, *a, **kw):
        seen["video"] = kw
        raise RuntimeError("stop here")

    monkeypatch.setattr(drivers, "make_renderer", make_renderer)
    monkeypatch.setattr(drivers, "render_video", render_video)
    try:
        cli.main(argv)
    except RuntimeError as e:
        assert str(e) == "stop here"
    return seen


@pytest.mark.parametrize("extra", [[], ["--orbit"], ["--redshift", "exact"], ["--orbit", "--redshift", "exact"], ["--lens_flare", "--tonemap", "aces"],
                                   ["--video_codec", "mjpeg"], ["--video_hdr", "pq"], ["--bit_depth", "16"], ["--dither", "blue"]],
                         ids=lambda e: "_".join(e) or "plain")
def test_spin_map_parses_and_reaches_the_driver(extra, monkeypatch):
    args = cli.parse_args(BASE + extra)
    assert args.spin_map is True and args.spin == 0.7
    cli.validate_args(args)
    seen = _run_main(monkeypatch, BASE + extra)
    assert seen["video"]["spin_map"] is True and seen["renderer"]["spin"] == 0.7
    assert seen["video"]["orbit"] == ("--orbit" in extra)
    assert not seen["video"]["ray_map"] and not seen["video"]["orbit_map"] and not seen["video"]["shutter_map"]


def test_the_exact_redshift_at_spin_zero_is_a_kerr_context(monkeypatch):
    assert cli.parse_args(["--redshift", "exact", "--video", "--spin_map"]).spin_map is True
    assert _run_main(monkeypatch, ["--redshift", "exact", "--video", "--spin_map"])["video"]["spin_map"] is True


REFUSALS = [
    (["--video", "--spin_map"], ["--spin", "--redshift exact"]),                       # no spin, model redshift
    (["--spin", "0.7", "--spin_map"], ["--video"]),
    (BASE + ["--shutter", "0.5"], ["--shutter"]),
    (BASE + ["--supersample", "2"], ["--supersample"]),
    (BASE + ["--map_supersample", "2"], ["--map_supersample"]),
    (BASE + ["--gpus", "2"], ["--gpus"]),
    (BASE + ["--ray_map"], ["--ray_map"]),
    (BASE + ["--orbit", "--orbit_map"], ["--orbit_map"]),
    (BASE + ["--shutter_map"], ["--shutter_map"]),
    (BASE + ["--observer", "circular"], ["--observer"]),
    (BASE + ["--observer_velocity", "0.1", "0", "0"], ["--observer_velocity"]),
    (BASE + ["--projection", "fisheye"], ["--projection"]),
    (BASE + ["--light_delay"], ["--light_delay"]),
    (BASE + ["--stars", "point"], ["--stars point"]),
    (BASE + ["--polarization", "toroidal"], ["--polarization"]),
]


@pytest.mark.parametrize("argv, words", REFUSALS, ids=lambda v: "_".join(w.lstrip("-") for w in v if isinstance(w, str))[:40] if isinstance(v, list) else None)
def test_refusals_are_argparse_errors(argv, words, capsys, monkeypatch):
    monkeypatch.setattr(drivers, "make_renderer", lambda *a, **kw: pytest.fail("a refusal touched the device"))
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--spin_map" in err
    for w in words:
        assert w in err, (w, err)


def test_without_the_flag_the_namespace_is_what_it_was():
    """(No key at all: tests/test_projection_cli.py pins the default namespace key for key, so the flag is absent unless given.)"""
    for line in ([], ["--spin", "0.7", "--video"], ["--spin", "0.7", "--video", "--orbit", "--redshift", "exact"], ["--video", "--ray_map"],
                 ["--video", "--orbit", "--orbit_map"], ["--video", "--shutter", "0.5", "--shutter_map"]):
        ns = vars(cli.parse_args(line))
        assert "spin_map" not in ns
        if "--spin" in line:
            with_flag = vars(cli.parse_args(line + ["--spin_map"]))
            assert with_flag.pop("spin_map") is True and with_flag == ns


class _Renderer:
    spin, redshift, supersample, anti_alias, disk_tilt = 0.7, "model", 1, "disabled", 0.0


@pytest.mark.parametrize("kw, words", [
    (dict(spin=0.0, redshift="model"), ["--spin", "--redshift exact"]),
    (dict(spin=0.7, video=False), ["--video"]),
    (dict(spin=0.7, shutter=0.5), ["--shutter"]),
    (dict(spin=0.7, supersample=2), ["--supersample"]),
    (dict(spin=0.7, map_supersample=2), ["--map_supersample"]),
    (dict(spin=0.7, gpus=2), ["--gpus"]),
    (dict(spin=0.7, world=2), ["ranks"]),
    (dict(spin=0.7, ray_map=True), ["--ray_map"]),
    (dict(spin=0.7, orbit_map=True), ["--orbit_map"]),
    (dict(spin=0.7, shutter_map=True), ["--shutter_map"]),
    (dict(spin=0.7, observer=True), ["--observer"]),
    (dict(spin=0.7, projection=True), ["--projection"]),
    (dict(spin=0.7, light_delay=True), ["--light_delay"]),
    (dict(spin=0.7, stars=True), ["--stars point"]),
    (dict(spin=0.7, polarization=True), ["--polarization"]),
], ids=lambda v: "_".join(v) if isinstance(v, dict) else None)
def test_check_spin_map_raises_the_same_refusals(kw, words):
    with pytest.raises(ValueError) as e:
        drivers.check_spin_map(True, **kw)
    for w in ["--spin_map"] + words:
        assert w in str(e.value), (w, str(e.value))
    drivers.check_spin_map(False, **kw)                      # without the flag nothing is asked
    drivers.check_spin_map(True, spin=0.7)
    drivers.check_spin_map(True, spin=0.0, redshift="exact")


@pytest.mark.parametrize("kw, word", [(dict(shutter=0.5), "--shutter"), (dict(supersample=2), "--supersample"), (dict(ray_map=True), "--ray_map"),
                                      (dict(world=2, rank=0), "ranks"), (dict(light_delay=1.0), "--light_delay"),
                                      (dict(projection="fisheye"), "--projection"), (dict(observer="circular"), "--observer")],
                         ids=lambda v: "_".join(v) if isinstance(v, dict) else None)
def test_render_video_refuses_before_it_touches_the_renderer(kw, word, tmp_path):
    """The renderer here has no device behind it: anything beyond reading its settings would raise AttributeError."""
    with pytest.raises(ValueError) as e:
        drivers.render_video(_Renderer(), 64, 40, 6, 24, str(tmp_path / "v.mp4"), 90.0, [6, 0, 0.5], spin_map=True, **kw)
    assert "--spin_map" in str(e.value) and word in str(e.value)


def test_progress_params_carry_spin_map_only_when_set():
    base = drivers.progress_params(6, 90.0, False, 0.1, 360.0)
    assert "spin_map" not in base and base == drivers.progress_params(6, 90.0, False, 0.1, 360.0, spin_map=False)
    assert drivers.progress_params(6, 90.0, False, 0.1, 360.0, spin_map=True) == {**base, "spin_map": True}
