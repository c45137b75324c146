"""--spin_anti_alias lod_radius / --spin_aa_strength on the command line and in the drivers: the flags parse, every combination
rules.FEATURES["kerr_anti_alias"] refuses is an argparse error that names both flags, a line without the flags has the namespace
it had, and the keyword reaches the drivers only when it is set."""
import contextlib
import io

import pytest

from bhr_amd import cli, drivers, rules

BASE = ["--spin", "0.9"]


def _error(argv):
    err = io.StringIO()
    with contextlib.redirect_stderr(err), pytest.raises(SystemExit) as e:
        cli.parse_args(argv)
    assert e.value.code == 2
    return err.getvalue()


def test_flags_parse():
    args = cli.parse_args(BASE + ["--spin_anti_alias", "lod_radius"])
    assert args.spin_anti_alias == "lod_radius" and not hasattr(args, "spin_aa_strength")
    assert cli.kerr_anti_alias_from_args(args) == {"kerr_anti_alias": 1.0}
    args = cli.parse_args(["--redshift", "exact", "--spin_anti_alias", "lod_radius", "--spin_aa_strength", "1.5", "--supersample", "2", "--lens_flare"])
    assert cli.kerr_anti_alias_from_args(args) == {"kerr_anti_alias": 1.5}
    args = cli.parse_args(BASE + ["--spin_anti_alias", "lod_radius", "--video", "--orbit", "--tonemap", "aces"])
    assert cli.kerr_anti_alias_from_args(args) == {"kerr_anti_alias": 1.0}
    assert "--spin_anti_alias" in _error(BASE + ["--spin_anti_alias", "bilinear"])          # argparse's own: not a choice


def test_a_line_without_the_flags_has_the_namespace_it_had():
    for argv in ([], BASE, BASE + ["--video", "--spin_map"], ["--anti_alias", "lod_radius"]):
        ns = vars(cli.parse_args(argv))
        assert not any("spin_anti_alias" in k or "spin_aa" in k or "kerr_anti_alias" in k for k in ns), sorted(ns)
        assert cli.kerr_anti_alias_from_args(cli.parse_args(argv)) == {}


REFUSED = [
    ([], "--spin"),                                                        # without a spin
    (["--anti_alias", "lod_radius"], "--spin"),
    (BASE + ["--video", "--spin_map"], "--spin_map"),
    (BASE + ["--video", "--shutter", "0.5", "--spin_shutter_map"], "--spin_shutter_map"),
    (BASE + ["--spin_polarization", "toroidal"], "--spin_polarization"),
    (BASE + ["--spin_stars", "point"], "--spin_stars"),
    (BASE + ["--spin_passes", "p.npz"], "--spin_passes"),
    (BASE + ["--spin_observer", "zamo"], "--spin_observer"),
    (BASE + ["--spin_observer_velocity", "0.1", "0", "0"], "--spin_observer"),
    (BASE + ["--spin_projection", "fisheye"], "--spin_projection"),
    (BASE + ["--gpus", "2"], "--gpus"),
]


@pytest.mark.parametrize("argv, other", REFUSED, ids=lambda v: "_".join(w.strip("-") for w in v) if isinstance(v, list) else None)
def test_refusals_name_both_flags(argv, other):
    msg = _error(argv + ["--spin_anti_alias", "lod_radius"])
    assert "--spin_anti_alias" in msg and other in msg, msg


def test_strength_needs_the_flag_and_a_value_in_range():
    assert "--spin_aa_strength needs --spin_anti_alias" in _error(BASE + ["--spin_aa_strength", "2"])
    for bad in ("-0.5", "nan", "inf"):
        assert "--spin_aa_strength" in _error(BASE + ["--spin_anti_alias", "lod_radius", "--spin_aa_strength", bad])


def test_anti_alias_of_the_schwarzschild_march_stays_refused_with_a_spin():
    msg = _error(BASE + ["--anti_alias", "lod_radius"])
    assert "--spin does not combine with --anti_alias lod_radius" in msg and "Kerr's variational equations" in msg


def test_the_rule_on_the_drivers_surface():
    ok = dict(kerr_anti_alias=True, spin=0.9)
    assert rules.refusal("kerr_anti_alias", ok) is None
    assert rules.refusal("kerr_anti_alias", dict(kerr_anti_alias=True, redshift="exact")) is None
    for facts, word in ((dict(kerr_anti_alias=True), "needs --spin"), (dict(ok, spin_map=True), "--spin_map"), (dict(ok, spin_shutter_map=True), "--spin_shutter_map"),
                        (dict(ok, kerr_polarization=True), "--spin_polarization"), (dict(ok, kerr_stars=True), "--spin_stars"),
                        (dict(ok, kerr_passes_path="p.npz"), "--spin_passes"), (dict(ok, spin_observer=True), "--spin_observer"),
                        (dict(ok, spin_projection=True), "--spin_projection"), (dict(ok, gpus=2), "--gpus"), (dict(ok, world=2), "ranks")):
        text = rules.refusal("kerr_anti_alias", facts)
        assert text is not None and "--spin_anti_alias" in text and word in text, (facts, text)
    rules.refuse_on("kerr_anti_alias", dict(spin_map=True))               # off: nothing to refuse


class _Reached(Exception):
    pass


def test_render_image_refuses_before_the_device_and_passes_the_strength_on(monkeypatch):
    def no_device(*a, **kw):
        raise _Reached()
    monkeypatch.setattr(drivers, "make_renderer", no_device)
    args = dict(width=32, height=16, cam_pos=[6, 0, 0.5], fov=90, step_size=0.1)
    with pytest.raises(ValueError, match="needs --spin"):
        drivers.render_image(**args, kerr_anti_alias=1.0)
    with pytest.raises(ValueError, match="--spin_passes"):
        drivers.render_image(**args, spin=0.9, kerr_anti_alias=1.0, kerr_passes_path="p.npz")
    with pytest.raises(ValueError, match="one GPU"):                     # (a spin's own refusal: the rule sits behind every older one)
        drivers.render_image(**args, spin=0.9, kerr_anti_alias=1.0, gpus=2)
    with pytest.raises(ValueError, match="--spin_aa_strength"):
        drivers.render_image(**args, spin=0.9, kerr_anti_alias=-1.0)
    with pytest.raises(_Reached):
        drivers.render_image(**args, spin=0.9, kerr_anti_alias=1.5, supersample=2, redshift="exact", lens_flare=True)


def test_main_passes_the_keyword_only_when_it_is_set(monkeypatch):
    calls = []
    monkeypatch.setattr(drivers, "render_image", lambda **kw: calls.append(kw) or _raise())
    for argv, want in ((BASE, None), (BASE + ["--spin_anti_alias", "lod_radius"], 1.0),
                       (BASE + ["--spin_anti_alias", "lod_radius", "--spin_aa_strength", "0.5"], 0.5)):
        with pytest.raises(_Reached), contextlib.redirect_stdout(io.StringIO()):
            cli.main(argv)
        kw = calls.pop()
        assert kw.get("kerr_anti_alias") == want and ("kerr_anti_alias" in kw) == (want is not None)


def _raise():
    raise _Reached()


class _Video:
    """A renderer for render_video's checks: the settings they read; anything else is device work."""
    supersample, supersample_threshold, disk_tilt, anti_alias, _dv2 = 1, None, 0.0, "disabled", None

    def __init__(self, spin=0.9, aa=None):
        self.spin, self.redshift, self._kerr_anti_alias = spin, "model", aa

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        raise _Reached(name)


def test_render_video_refuses_what_the_call_says_and_what_the_renderer_is_set_to(tmp_path):
    args = (32, 16, 4, 24, str(tmp_path / "v.mp4"), 90, [6, 0, 0.5])
    with pytest.raises(ValueError, match="needs --spin"):
        drivers.render_video(_Video(spin=0.0), *args, kerr_anti_alias=1.0)
    with pytest.raises(ValueError, match="--spin_map"):
        drivers.render_video(_Video(), *args, kerr_anti_alias=1.0, spin_map=True)
    with pytest.raises(ValueError, match="ranks"):
        drivers.render_video(_Video(), *args, kerr_anti_alias=1.0, world=2)
    with pytest.raises(ValueError, match="--spin_aa_strength"):
        drivers.render_video(_Video(), *args, kerr_anti_alias=float("nan"))
    with pytest.raises(ValueError, match="--spin_anti_alias does not combine with --spin_map"):      # on in the renderer already
        drivers.render_video(_Video(aa=1.0), *args, spin_map=True)
    with pytest.raises(_Reached, match="set_kerr_anti_alias"):
        drivers.render_video(_Video(), *args, kerr_anti_alias=1.0, orbit=True)
