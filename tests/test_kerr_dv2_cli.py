"""--spin_disk_model v2 | v2_volume on the command line and in the drivers: the flag parses, every combination
rules.FEATURES["kerr_disk_model"] refuses is an argparse error that names both flags, a line without the flag has the namespace it
had, --disk_model with a spin stays refused word for word, and the keyword reaches the drivers only when it is set."""
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


def test_flag_parses_with_what_it_combines_with():
    for argv in (BASE + ["--spin_disk_model", "v2"], BASE + ["--spin_disk_model", "v2_volume", "--supersample", "2", "--lens_flare"],
                 ["--redshift", "exact", "--spin_disk_model", "v2"], BASE + ["--spin_disk_model", "v2", "--redshift", "exact", "--tonemap", "aces"],
                 BASE + ["--spin_disk_model", "v2_volume", "--video", "--orbit", "--video_codec", "mjpeg"],
                 BASE + ["--spin_disk_model", "v2", "--video", "--video_hdr", "pq"], BASE + ["--spin_disk_model", "v2", "--bit_depth", "16"]):
        args = cli.parse_args(argv)
        assert args.spin_disk_model == argv[argv.index("--spin_disk_model") + 1] and args.disk_model == "texture"
    assert "--spin_disk_model" in _error(BASE + ["--spin_disk_model", "texture"])          # argparse's own: not a choice


def test_a_line_without_the_flag_has_the_namespace_it_had():
    for argv in ([], BASE, BASE + ["--video", "--spin_map"], ["--disk_model", "v2"]):
        ns = vars(cli.parse_args(argv))
        assert not any("spin_disk_model" in k or "kerr_disk_model" in k for k in ns), sorted(ns)
    assert rules.FACTS["kerr_disk_model"] == "texture"


REFUSED = [
    ([], "--spin"),                                                        # without a spin
    (["--disk_model", "v2"], "--spin"),
    (BASE + ["--disk_model", "v2"], "--disk_model"),
    (BASE + ["--disk_model", "v2_volume"], "--disk_model"),
    (BASE + ["--video", "--spin_map"], "--spin_map"),
    (BASE + ["--video", "--shutter", "0.5", "--spin_shutter_map"], "--spin_shutter_map"),
    (BASE + ["--spin_polarization", "toroidal"], "--spin_polarization"),
    (BASE + ["--spin_stars", "point"], "--spin_stars"),
    (BASE + ["--spin_passes", "p.npz"], "--spin_passes"),
    (BASE + ["--spin_observer", "zamo"], "--spin_observer"),
    (BASE + ["--spin_observer_velocity", "0.1", "0", "0"], "--spin_observer"),
    (BASE + ["--spin_projection", "fisheye"], "--spin_projection"),
    (BASE + ["--spin_anti_alias", "lod_radius"], "--spin_anti_alias"),
    (BASE + ["--gpus", "2"], "--gpus"),
]


@pytest.mark.parametrize("model", ["v2", "v2_volume"])
@pytest.mark.parametrize("argv, other", REFUSED, ids=lambda v: "_".join(w.strip("-") for w in v) if isinstance(v, list) else None)
def test_refusals_name_both_flags(argv, other, model):
    msg = _error(argv + ["--spin_disk_model", model])
    assert "--spin_disk_model" in msg and other in msg, msg


def test_the_volume_with_the_exact_redshift_is_refused_and_the_surface_is_not():
    msg = _error(BASE + ["--redshift", "exact", "--spin_disk_model", "v2_volume"])
    assert "--spin_disk_model v2_volume does not combine with --redshift exact" in msg
    assert cli.parse_args(BASE + ["--redshift", "exact", "--spin_disk_model", "v2"]).spin_disk_model == "v2"


def test_disk_model_with_a_spin_stays_refused_with_todays_words():
    for model in ("v2", "v2_volume"):
        msg = _error(BASE + ["--disk_model", model])
        assert "--spin does not combine with --disk_model other than texture: the Kerr march shades the disk texture" in msg
    msg = _error(["--redshift", "exact", "--disk_model", "v2"])
    assert "--redshift exact (the Kerr march, as with --spin) does not combine with --disk_model other than texture" in msg


def test_the_rule_has_the_same_words_on_both_surfaces():
    ok = dict(kerr_disk_model="v2", spin=0.9)
    assert rules.refusal("kerr_disk_model", ok) is None and rules.refusal("kerr_disk_model", dict(ok, kerr_disk_model="v2_volume")) is None
    assert rules.refusal("kerr_disk_model", dict(kerr_disk_model="v2", redshift="exact")) is None
    rows = ((dict(kerr_disk_model="v2"), "needs --spin"), (dict(ok, disk_model="v2"), "--disk_model"), (dict(ok, spin_map=True), "--spin_map"),
            (dict(ok, spin_shutter_map=True), "--spin_shutter_map"), (dict(ok, kerr_polarization=True), "--spin_polarization"),
            (dict(ok, kerr_stars=True), "--spin_stars"), (dict(ok, kerr_passes_path="p.npz"), "--spin_passes"), (dict(ok, spin_observer=True), "--spin_observer"),
            (dict(ok, spin_projection=True), "--spin_projection"), (dict(ok, kerr_anti_alias=True), "--spin_anti_alias"), (dict(ok, gpus=2), "--gpus"),
            (dict(ok, world=2), "ranks"), (dict(ok, kerr_disk_model="v2_volume", redshift="exact"), "--redshift exact"))
    assert len(rows) == len(rules.FEATURES["kerr_disk_model"]["rows"].split()) + 1          # every row (gpus_or_world twice)
    for facts, word in rows:
        text = rules.refusal("kerr_disk_model", facts)
        assert text is not None and "--spin_disk_model" in text and word in text, (facts, text)
        assert rules.refusal("kerr_disk_model", facts, "cli") == text
    rules.refuse_on("kerr_disk_model", dict(spin_map=True))               # off: nothing to refuse


class _Reached(Exception):
    pass


def _raise():
    raise _Reached()


def test_render_image_refuses_before_the_device(monkeypatch):
    def no_device(*a, **kw):
        raise _Reached()
    monkeypatch.setattr(drivers, "make_renderer", no_device)
    args = dict(width=32, height=16, cam_pos=[6, 0, 0.5], fov=90, step_size=0.1)
    with pytest.raises(ValueError, match="needs --spin"):
        drivers.render_image(**args, kerr_disk_model="v2")
    with pytest.raises(ValueError, match="--spin_disk_model does not combine with --disk_model"):
        drivers.render_image(**args, spin=0.9, kerr_disk_model="v2", disk_model="v2")
    with pytest.raises(ValueError, match="--spin_passes"):
        drivers.render_image(**args, spin=0.9, kerr_disk_model="v2", kerr_passes_path="p.npz")
    with pytest.raises(ValueError, match="--spin_anti_alias"):
        drivers.render_image(**args, spin=0.9, kerr_disk_model="v2_volume", kerr_anti_alias=1.0)
    with pytest.raises(ValueError, match="--spin_disk_model .*--gpus"):
        drivers.render_image(**args, spin=0.9, kerr_disk_model="v2", gpus=2)
    with pytest.raises(ValueError, match="--redshift exact"):
        drivers.render_image(**args, spin=0.9, kerr_disk_model="v2_volume", redshift="exact")
    with pytest.raises(ValueError, match="--spin_disk_model is one of"):
        drivers.render_image(**args, spin=0.9, kerr_disk_model="v3")
    with pytest.raises(ValueError, match="the Kerr march shades the disk texture|Disk V2 are Schwarzschild's"):      # today's refusal of disk_model under a spin
        drivers.render_image(**args, spin=0.9, disk_model="v2")
    with pytest.raises(_Reached):
        drivers.render_image(**args, spin=0.9, kerr_disk_model="v2", supersample=2, redshift="exact", lens_flare=True)
    with pytest.raises(_Reached):
        drivers.render_image(**args, spin=0.9, kerr_disk_model="v2_volume", grade=dict(tonemap="aces"))


def test_main_passes_the_keyword_only_when_it_is_set(monkeypatch):
    calls = []
    monkeypatch.setattr(drivers, "render_image", lambda **kw: calls.append(kw) or _raise())
    for argv, want in ((BASE, None), (BASE + ["--spin_disk_model", "v2"], "v2"), (BASE + ["--spin_disk_model", "v2_volume"], "v2_volume")):
        with pytest.raises(_Reached), contextlib.redirect_stdout(io.StringIO()):
            cli.main(argv)
        kw = calls.pop()
        assert kw.get("kerr_disk_model") == want and ("kerr_disk_model" in kw) == (want is not None)
        assert kw["disk_model"] == "texture"


class _Video:
    """A renderer for render_video's checks: the settings they read; anything else is device work."""
    supersample, supersample_threshold, disk_tilt, anti_alias, _dv2, r_disk_inner, r_disk_outer = 1, None, 0.0, "disabled", None, 2.0, 15.0

    def __init__(self, spin=0.9, aa=None, redshift="model"):
        self.spin, self.redshift, self._kerr_anti_alias = spin, redshift, aa

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        raise _Reached(name)


def test_render_video_refuses_what_the_call_says_and_what_the_renderer_is_set_to(tmp_path):
    args = (32, 16, 4, 24, str(tmp_path / "v.mp4"), 90, [6, 0, 0.5])
    with pytest.raises(ValueError, match="needs --spin"):
        drivers.render_video(_Video(spin=0.0), *args, kerr_disk_model="v2")
    with pytest.raises(ValueError, match="--spin_disk_model does not combine with --spin_map"):
        drivers.render_video(_Video(), *args, kerr_disk_model="v2", spin_map=True)
    with pytest.raises(ValueError, match="--spin_disk_model .*ranks"):
        drivers.render_video(_Video(), *args, kerr_disk_model="v2_volume", world=2)
    with pytest.raises(ValueError, match="--spin_disk_model does not combine with --spin_anti_alias"):
        drivers.render_video(_Video(), *args, kerr_disk_model="v2", kerr_anti_alias=1.0)
    with pytest.raises(ValueError, match="--spin_disk_model does not combine with --spin_anti_alias"):      # on in the renderer already
        drivers.render_video(_Video(aa=1.0), *args, kerr_disk_model="v2")
    with pytest.raises(ValueError, match="--redshift exact"):
        drivers.render_video(_Video(redshift="exact"), *args, kerr_disk_model="v2_volume")
    with pytest.raises(_Reached, match="use_kerr_disk_v2"):
        drivers.render_video(_Video(), *args, kerr_disk_model="v2", orbit=True)
