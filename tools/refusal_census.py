"""The refusal census: what the command line, the drivers' check_* functions and the two drivers say to every combination of a
fixed list of features, before any device is touched -- the refusal's whole text, or that the line was accepted.

    python tools/refusal_census.py            writes tests/golden/refusal_census.json
    python tools/refusal_census.py --check    recomputes everything and compares it with the recording

It uses the package's public surface only (cli.parse_args / validate_args / main, drivers.check_*, drivers.render_image /
render_video), so the same file runs on any commit: the recording is made on the commit BEFORE a change to the rules and
checked on the commit after it.  tests/test_refusal_census.py checks a part of it (every tenth triple of section 1) in the suite.

Sections, each one flat list of indices into ``outcomes``, in enumeration order:
  cli           every combination of 1, 2 and 3 of CLI_ATOMS (itertools.combinations order)
  cli_ranks     the accepted --video lines of ``cli`` again under WORLD_SIZE=2, up to the first call that needs a device
  checks        every public drivers.check_*: a base call that is accepted, then every keyword alone and every pair
  render_image  drivers.render_image up to the device: every feature keyword alone and in pairs, without and with a spin
  render_video  drivers.render_video on a renderer that has only what the checks read: likewise
"""
import argparse
import contextlib
import hashlib
import inspect
import io
import itertools
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "refusal_census.json")

CLI_ATOMS = [
    "--video", "--orbit", "--spin 0.9", "--redshift exact", "--disk_tilt 10", "--anti_alias lod_radius", "--disk_model v2", "--gpus 2",
    "--supersample 2", "--supersample_threshold 0.1",
    "--observer circular", "--observer_velocity 0.1 0 0", "--observer_sky plain", "--infall_to 2",
    "--projection equirect", "--projection_fov 180",
    "--spin_observer zamo", "--spin_observer_velocity 0.1 0 0", "--spin_observer_sky plain", "--spin_projection fisheye", "--spin_projection_fov 180",
    "--light_delay 1", "--polarization toroidal", "--spin_polarization toroidal", "--polarization_cell 16", "--stokes_output s.npz",
    "--polarization_ticks t.png",
    "--shutter 0.5", "--ray_map", "--orbit_map", "--shutter_map", "--spin_map", "--spin_shutter_map", "--spin_map_supersample 2", "--map_supersample 2",
    "--passes p.npz", "--stars point", "--spin_stars point", "--spin_passes q.npz", "--texture sky.png",
    "--tonemap aces", "--video_hdr pq", "--video_codec mjpeg", "--bit_depth 16", "--dither blue", "--hdr_output h.pfm", "--fov 60",
    # values that are refused as such
    "--star_gain 0", "--light_delay 17", "--spin 1.5",
]


class Device(Exception):
    """Raised by the stand-ins for everything that needs a device."""


def short(obj) -> str:
    return hashlib.sha1(json.dumps(obj, sort_keys=True, default=str).encode()).hexdigest()[:8]


# ---- 1. command lines ---------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def recorders(drivers, calls, world=None):
    """cli.main's four calls into the drivers replaced by recorders; with ``world`` ranks make_renderer ends the run instead."""
    def make_renderer(*a, **kw):
        if world is not None:
            raise Device()
        calls.append(("make_renderer", a, kw))
        return type("R", (), {"close": lambda self: None})(), False, 0, 0
    names = {"make_renderer": make_renderer}
    for name in ("render_image", "render_video", "save_image"):
        names[name] = lambda *a, _n=name, **kw: calls.append((_n, a[1:] if _n == "render_video" else a, kw))
    before = {n: getattr(drivers, n) for n in names}
    env = {k: os.environ.pop(k, None) for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "BHR_FORCE_DEVICE")}
    if world is not None:
        os.environ.update(RANK="0", WORLD_SIZE=str(world), LOCAL_RANK="0", BHR_FORCE_DEVICE="0")
    for n, fn in names.items():
        setattr(drivers, n, fn)
    try:
        yield
    finally:
        for n, fn in before.items():
            setattr(drivers, n, fn)
        for k, v in env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def cli_line(argv):
    """-> (outcome, outcome under two ranks or None)."""
    from bhr_amd import cli, drivers
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            args = cli.parse_args(argv)
    except SystemExit as e:
        return f"exit {e.code}: {err.getvalue().strip().splitlines()[-1].split(': error: ', 1)[-1]}", None     # (without the program's name)
    try:
        cli.validate_args(args)
    except ValueError as e:
        return f"validate_args: {e}", None
    out = "ok:" + short(vars(args))
    calls = []
    try:
        with recorders(drivers, calls), contextlib.redirect_stdout(io.StringIO()):
            cli.main(argv)
        out += " main:" + short(calls)
    except ValueError as e:
        out += f" main: {e}"
    ranks = None
    if args.video:
        try:
            with recorders(drivers, [], world=2), contextlib.redirect_stdout(io.StringIO()):
                cli.main(argv)
            ranks = "returned"
        except Device:
            ranks = "reached the device"
        except ValueError as e:
            ranks = str(e)
    return out, ranks


def cli_cases(n_max=3):
    for n in range(1, n_max + 1):
        for combo in itertools.combinations(CLI_ATOMS, n):
            yield n, [word for atom in combo for word in atom.split()]


# ---- 2. the drivers' checks ---------------------------------------------------------------------------------------------------------
POL = dict(field=(0.0, 1.0, 0.0))
# per check: the base call, which is accepted
CHECK_BASE = {
    "check_depth_and_dither": dict(bit_depth=8, dither="none"), "check_hdr_path": dict(path="a.pfm"), "check_grade": dict(grade=dict(tonemap="aces")),
    "check_stars": dict(stars={}), "check_kerr_stars": dict(kerr_stars={}, spin=0.5), "check_kerr_passes": dict(kerr_passes_path="p.npz", spin=0.5),
    "check_observer": dict(observer=(0.1, 0.0, 0.0)), "check_projection": dict(projection="equirect"), "check_light_delay": dict(scale=1.0),
    "check_kerr_view": dict(kerr_view=dict(observer="zamo"), spin=0.5), "check_passes": dict(passes_path="p.npz"),
    "check_polarization": dict(polarization=POL), "check_kerr_polarization": dict(kerr_polarization=POL, spin=0.5),
    "check_ray_map": dict(ray_map=True), "check_orbit_map": dict(orbit_map=True), "check_shutter_map": dict(shutter_map=True),
    "check_spin_map": dict(spin_map=True, spin=0.5), "check_spin_shutter_map": dict(spin_shutter_map=True, spin=0.5),
    "check_shutter": dict(shutter=0.5, shutter_samples=8), "check_map_supersample": dict(k=1), "check_spin_map_supersample": dict(k=1),
    "check_video_hdr": dict(video_hdr="pq"),
}
# per keyword: the other values it is set to (a bool without an entry is flipped)
CHECK_VALUES = {
    "spin": [0.0, 0.9], "redshift": ["exact"], "skybox_path": ["sky.png"], "supersample": [2, None], "gpus": [2], "world": [2], "disk_model": ["v2"],
    "disk_tilt": [10.0], "anti_alias": ["lod_radius"], "supersample_threshold": [0.1], "shutter": [0.0, 0.5, 2.0], "map_supersample": [2],
    "spin_map_supersample": [2], "stokes_path": ["s.npz", "s.txt"], "ticks_path": ["t.png", "t.jpg"], "projection_fov": [(180.0,)], "video_codec": ["mjpeg"],
    "video_stream": ["off"], "width": [3], "height": [3], "hdr_white": [20000.0], "hdr_exposure": [20.0], "dither": ["blue", "red"], "bit_depth": [16, 12],
    "k": [2, 3], "shutter_samples": [0], "path": ["a.txt"], "passes_path": [None, "p.txt"], "kerr_passes_path": [None, "q.txt"],
    "stars": [None, dict(gain=0.0), dict(colour=1)], "kerr_stars": [None, dict(gain=0.0), dict(colour=1)], "scale": [None, 17.0, "x"],
    "observer": [None, (2.0, 0.0, 0.0)], "projection": [None, "fisheye", "cube"], "polarization": [None, dict(field=(0.0, 0.0, 0.0)), dict(cell=16)],
    "kerr_polarization": [None, dict(field=(0.0, 0.0, 0.0)), dict(cell=16)], "video_hdr": [None, "hlg", "dolby"],
    "kerr_view": [None, dict(projection="fisheye"), dict(observer="infall"), dict(sky="plain"), dict(observer="zamo", colour=1)],
    "grade": [None, dict(tonemap="aces", white=0.0), dict(exposure=1.0)],
    "ray_map": [False], "orbit_map": [False], "shutter_map": [False], "spin_map": [False], "spin_shutter_map": [False],
}
# keywords that are a bool in one check and the feature's own value in another
CHECK_BOOLS = {"check_stars": {"observer": [(0.1, 0.0, 0.0)]}}


def check_cases():
    from bhr_amd import drivers
    for name in sorted(n for n in dir(drivers) if n.startswith("check_") and callable(getattr(drivers, n))):
        fn, base = getattr(drivers, name), CHECK_BASE[name]
        atoms = []
        for i, (p, par) in enumerate(inspect.signature(fn).parameters.items()):
            if i > 0 and name in CHECK_BOOLS and p in CHECK_BOOLS[name]:
                values = CHECK_BOOLS[name][p]
            elif i > 0 and isinstance(par.default, bool):
                values = [not par.default]
            else:
                values = CHECK_VALUES[p]
            atoms += [(p, v) for v in values if v != base.get(p, par.default) or v is None]
        yield name, fn, dict(base)
        for n in (1, 2):
            for combo in itertools.combinations(atoms, n):
                if len({p for p, _ in combo}) == n:
                    yield name, fn, {**base, **dict(combo)}


def check_outcome(fn, kw) -> str:
    try:
        return "-> " + repr(fn(**kw))
    except ValueError as e:
        return str(e)


# ---- 3. the drivers up to the device -------------------------------------------------------------------------------------------------
IMAGE_ATOMS = [
    dict(gpus=2), dict(disk_model="v2"), dict(supersample=2), dict(supersample_threshold=0.1), dict(disk_tilt=10.0), dict(anti_alias="lod_radius"),
    dict(grade=dict(tonemap="aces")), dict(hdr_path="h.pfm"), dict(passes_path="p.npz"), dict(spin=0.5), dict(redshift="exact"),
    dict(observer=(0.1, 0.0, 0.0)), dict(stars={}), dict(projection="equirect"), dict(projection_fov=(180.0,)), dict(light_delay=1.0),
    dict(polarization=POL), dict(stokes_path="s.npz"), dict(ticks_path="t.png"), dict(kerr_polarization=POL), dict(kerr_view=dict(observer="zamo")),
    dict(kerr_view=dict(projection="fisheye")), dict(kerr_stars={}), dict(kerr_passes_path="q.npz"), dict(skybox_path="sky.png"), dict(bit_depth=16),
    dict(dither="blue"), dict(passes_path="p.txt"), dict(stokes_path="s.txt"),
]
VIDEO_ATOMS = [
    dict(orbit=True), dict(supersample=2), dict(supersample=1), dict(supersample_threshold=0.1), dict(shutter=0.5), dict(ray_map=True), dict(orbit_map=True),
    dict(shutter_map=True), dict(map_supersample=2), dict(observer="circular"), dict(observer_velocity=(0.1, 0.0, 0.0)), dict(infall_to=2.0), dict(stars={}),
    dict(projection="equirect"), dict(projection_fov=(180.0,)), dict(light_delay=1.0), dict(polarization=POL), dict(stokes_path="s.npz"),
    dict(spin_map=True), dict(kerr_polarization=POL), dict(kerr_view=dict(observer="zamo")), dict(kerr_view=dict(projection="fisheye")),
    dict(spin_map_supersample=2), dict(spin_shutter_map=True), dict(kerr_stars={}), dict(world=2), dict(video_hdr="pq"), dict(video_codec="mjpeg"),
    dict(grade=dict(tonemap="aces")), dict(bit_depth=16), dict(dither="blue"), dict(video_stream="off"), dict(stokes_path="s.txt"),
    # what the renderer is set to ("r." + the attribute)
    {"r.spin": 0.6}, {"r.redshift": "exact"}, {"r.supersample": 2}, {"r.supersample_threshold": 0.1}, {"r.disk_tilt": 10.0}, {"r.anti_alias": "lod_radius"},
    {"r._dv2": "a Disk V2 source"},
]


# cases of more than two keywords where render_video says something else, or in another order, than the feature's check_* alone
VIDEO_DEEPER = [
    {"r.spin": 0.6, "spin_map": True, "kerr_polarization": POL, "supersample_threshold": 0.1},
    {"r.spin": 0.6, "spin_map": True, "kerr_polarization": POL, "r.supersample_threshold": 0.1},
    {"r.spin": 0.6, "spin_map": True, "kerr_polarization": POL, "supersample": 2, "supersample_threshold": 0.1},
    {"spin_shutter_map": True, "shutter": 0.5, "map_supersample": 2},
    {"spin_shutter_map": True, "shutter": 0.5, "map_supersample": 2, "supersample": 2},
    {"spin_shutter_map": True, "shutter": 0.5, "map_supersample": 2, "r.supersample": 2},
    {"r.spin": 0.6, "spin_shutter_map": True, "shutter": 0.5, "world": 2, "r.supersample": 2},
    {"ray_map": True, "stars": {}, "shutter_map": True, "map_supersample": 2, "world": 2},
    {"ray_map": True, "stars": {}, "map_supersample": 2, "world": 2},
]


def combos(atoms, bases):
    for base in bases:
        for n in (1, 2):
            for combo in itertools.combinations(atoms, n):
                kw = dict(base)
                for atom in combo:
                    kw.update(atom)
                if len(kw) == len(base) + n:          # (two values of one keyword are one keyword)
                    yield kw


class FakeRenderer:
    """What render_video's checks read, and nothing else: every other attribute is the device."""
    def __init__(self, **attrs):
        self.__dict__.update(dict(spin=0.0, redshift="model", supersample=1, supersample_threshold=None, disk_tilt=0.0, anti_alias="disabled", _dv2=None), **attrs)

    def stars_info(self):
        return {"n": 1}

    def kerr_stars_info(self):
        return {"n": 1}

    def __getattr__(self, name):
        raise Device()


def driver_outcome(call) -> str:
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            call()
    except Device:
        return "reached the device"
    except ValueError as e:
        return str(e)
    return "returned"


def device_stub(*a, **kw):
    raise Device()


def image_outcomes():
    from bhr_amd import drivers, multigpu
    before = drivers.make_renderer, multigpu.render_image_tiled
    drivers.make_renderer = multigpu.render_image_tiled = device_stub
    try:
        for kw in combos(IMAGE_ATOMS, [{}, dict(spin=0.6)]):
            yield driver_outcome(lambda: drivers.render_image(8, 8, [6.0, 0.0, 0.5], 90.0, 0.1, **kw))
    finally:
        drivers.make_renderer, multigpu.render_image_tiled = before


def video_outcomes():
    from bhr_amd import drivers
    before = drivers.FrameSink
    drivers.FrameSink = device_stub
    try:
        with tempfile.TemporaryDirectory() as tmp:
            for kw in list(combos(VIDEO_ATOMS, [{}, {"r.spin": 0.6}])) + VIDEO_DEEPER:
                renderer = FakeRenderer(**{k[2:]: v for k, v in kw.items() if k.startswith("r.")})
                kw = {k: v for k, v in kw.items() if not k.startswith("r.")}
                yield driver_outcome(lambda: drivers.render_video(renderer, 8, 8, 2, 24, os.path.join(tmp, "v.mp4"), 90.0, [6.0, 0.0, 0.5], png_level=1, **kw))
    finally:
        drivers.FrameSink = before


LABELS = {}          # per section the cases of the last census, for --check's report


# ---- the census ----------------------------------------------------------------------------------------------------------------------
def census(cli_sizes=3, cli_triple_step=1):
    """-> (outcomes, sections).  ``cli_triple_step`` = s: only every s-th triple of the command lines is run (the others are None)."""
    table, sections = {}, {"cli": [], "cli_ranks": [], "checks": [], "render_image": [], "render_video": []}
    LABELS.clear()

    def index(outcome):
        return table.setdefault(outcome, len(table))
    triple = 0
    for n, argv in cli_cases(cli_sizes):
        if n == 3:
            triple += 1
            if (triple - 1) % cli_triple_step:
                sections["cli"].append(None)
                continue
        out, ranks = cli_line(argv)
        sections["cli"].append(index(out))
        if ranks is not None:
            sections["cli_ranks"].append(index(ranks))
            LABELS.setdefault("cli_ranks", []).append(argv)
    for name, fn, kw in check_cases():
        sections["checks"].append(index(f"{name}: {check_outcome(fn, kw)}"))
    sections["render_image"] = [index(o) for o in image_outcomes()]
    sections["render_video"] = [index(o) for o in video_outcomes()]
    LABELS.update(cli=[argv for _, argv in cli_cases(cli_sizes)], checks=[(name, kw) for name, _, kw in check_cases()],
                  render_image=list(combos(IMAGE_ATOMS, [{}, dict(spin=0.6)])), render_video=list(combos(VIDEO_ATOMS, [{}, {"r.spin": 0.6}])) + VIDEO_DEEPER)
    return list(table), sections


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--check", action="store_true", help="compare with the recording instead of writing it")
    args = ap.parse_args()
    outcomes, sections = census()
    record = {"cli_atoms": CLI_ATOMS, "image_atoms": IMAGE_ATOMS, "video_atoms": VIDEO_ATOMS, "outcomes": outcomes, "sections": sections}
    accepted = sum(outcomes[i].startswith("ok:") for i in sections["cli"])
    print(f"{', '.join(f'{k}: {len(v)} cases' for k, v in sections.items())}; {len(outcomes)} distinct outcomes, {accepted} command lines accepted")
    if not args.check:
        with open(GOLDEN, "w") as f:
            json.dump(record, f, separators=(",", ":"), default=str)
        print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")
        return 0
    with open(GOLDEN) as f:
        golden = json.load(f)
    differences = 0
    for name, want in golden["sections"].items():
        got = sections[name]
        bad = [i for i in range(max(len(want), len(got))) if i >= len(want) or i >= len(got) or golden["outcomes"][want[i]] != outcomes[got[i]]]
        differences += len(bad)
        print(f"{name}: {len(want)} cases, {len(bad)} differences")
        for i in bad[:20]:
            print(f"  case {i}: {LABELS[name][i] if i < len(LABELS[name]) else None}\n           recorded {golden['outcomes'][want[i]] if i < len(want) else None!r}\n           now      {outcomes[got[i]] if i < len(got) else None!r}")
    print(f"{differences} differences")
    return 1 if differences else 0


if __name__ == "__main__":
    sys.exit(main())
