"""HipRenderer: the reference's ``TaichiRenderer`` surface (render.py:2189-4028) on libbhr_hip.so.

Same constructor arguments, methods, attribute names and error behaviour, so the drivers and
tests that talk to ``TaichiRenderer`` read the same against this class.  All device work goes
through the C ABI in include/bhr.h; nothing here computes pixels on the host except the
lens flare, which the reference also does in NumPy (render.py:3925-4028).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .camera import build_camera
from .textures import compute_edge_alpha, keplerian_omega_rows

R_DISK_INNER_DEFAULT = 2.0   # render.py:433
R_DISK_OUTER_DEFAULT = 15.0  # render.py:434
DISK_COLOR_TEMPERATURE = 6000  # render.py:52


class _FieldView:
    """Stand-in for a Taichi field that tests read with ``.to_numpy()``."""

    def __init__(self, reader, shape):
        self._reader = reader
        self.shape = tuple(shape)

    def to_numpy(self) -> np.ndarray:
        return self._reader()


SUPERSAMPLE_FACTORS = (1, 2, 4, 8)


TONEMAPS = ("clip", "reinhard", "aces")
TRANSFERS = ("linear", "srgb")


def check_grade(grade) -> Optional[dict]:
    """A grade as set_grade takes it -- None, or a dict with any of tonemap, exposure, white, transfer, keep_hdr -- checked and
    completed with the defaults: None or dict(tonemap, exposure, white, transfer, keep_hdr).  Raises ValueError."""
    if grade is None or grade.get("tonemap") is None:
        if grade and any(k != "tonemap" for k in grade):
            raise ValueError("a grade needs a tonemap: 'clip', 'reinhard' or 'aces'")
        return None
    unknown = set(grade) - {"tonemap", "exposure", "white", "transfer", "keep_hdr"}
    if unknown:
        raise ValueError(f"grade: unknown field(s) {sorted(unknown)}")
    tonemap, transfer = grade["tonemap"], grade.get("transfer", "linear")
    if tonemap not in TONEMAPS:
        raise ValueError(f"tonemap must be one of {TONEMAPS} or None, got {tonemap!r}")
    if transfer not in TRANSFERS:
        raise ValueError(f"transfer must be one of {TRANSFERS}, got {transfer!r}")
    exposure, white = float(grade.get("exposure", 0.0)), float(grade.get("white", 2.5))
    if not (np.isfinite(exposure) and -16.0 <= exposure <= 16.0):
        raise ValueError(f"exposure must be a finite number of stops in [-16, 16], got {exposure!r}")
    if not (np.isfinite(white) and 0.0 < white <= 65504.0):
        raise ValueError(f"white must be finite and in (0, 65504], got {white!r}")
    return dict(tonemap=tonemap, exposure=float(np.float32(exposure)), white=float(np.float32(white)), transfer=transfer,
                keep_hdr=bool(grade.get("keep_hdr", False)))


def _check_supersample(k) -> None:
    if isinstance(k, bool) or k not in SUPERSAMPLE_FACTORS:
        raise ValueError(f"supersample must be one of {SUPERSAMPLE_FACTORS}, got {k!r}")


def _check_threshold(t) -> None:
    if t is None:
        return
    if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)) or t != t:
        raise ValueError(f"supersample_threshold must be a number (not NaN) or None, got {t!r}")


class HipRenderer:
    """Renders Schwarzschild black-hole frames on one MI355X (or one row block of a frame).

    Usage (render.py:2193-2196)::

        renderer = HipRenderer(width, height, skybox, disk_tex, ...)
        img1 = renderer.render(cam_pos=[6, 0, 0.5], fov=90)
    """

    def __init__(self, width, height, skybox, disk_tex,
                 step_size=0.1, r_max=10.0, device="hip",
                 r_disk_inner=R_DISK_INNER_DEFAULT, r_disk_outer=R_DISK_OUTER_DEFAULT,
                 disk_tilt=0.0, lens_flare=False, anti_alias="disabled", aa_strength=1.0,
                 disk_rotation_speed=0.1, ignore_taichi_cache=False,
                 device_index: int = 0, rows: Optional[Sequence[int]] = None, math: str = "strict",
                 frame_slots: Optional[int] = None, outputs: Optional[str] = None, options: Optional[dict] = None,
                 supersample: int = 1, supersample_threshold: Optional[float] = None, spin: float = 0.0,
                 redshift: str = "model"):
        # supersample=k: k x k rays per pixel, box-filtered inside the march (bhr_set_supersample; include/bhr.h states the filter)
        # supersample_threshold=T: adaptive -- k x k rays only for the pixels whose k = 1 neighbours differ by more than T
        # (bhr_set_adaptive_supersample); None: every pixel
        _check_supersample(supersample)
        _check_threshold(supersample_threshold)
        if device not in ("hip", "gpu"):
            raise ValueError(f"HipRenderer runs on the GPU only (device={device!r}); there is no CPU path")
        # math="strict" (default): the RK4 loop in the reference's operation order with IEEE sqrt and
        # divide -- ray paths bit-identical to a strict f32 evaluation of render.py:2854-3006.
        # math="fast": 2-D orbital-plane state, v_rsq/v_rcp, fast-math (Taichi's fast_math=True
        # analogue); ~3x faster, deviates from strict by f32 rounding noise only.
        # math="hybrid": the strict kernel on the 8x8 tiles whose rays pass near the photon sphere (impact parameter
        # within a band around 3 sqrt(3)/2 r_s -- the only rays that amplify rounding), the fast kernel on all others.
        if math not in ("fast", "strict", "hybrid"):
            raise ValueError(f"math must be 'fast', 'strict' or 'hybrid', got {math!r}")
        self.math = math
        if anti_alias not in ("disabled", "lod_radius"):
            raise ValueError(f"anti_alias must be 'disabled' or 'lod_radius', got {anti_alias!r}")
        self.width, self.height = int(width), int(height)
        self.step_size, self.r_max = step_size, r_max
        self.r_disk_inner, self.r_disk_outer = r_disk_inner, r_disk_outer
        self.disk_tilt = disk_tilt
        self.lens_flare = lens_flare
        self.anti_alias, self.aa_strength = anti_alias, aa_strength
        self.disk_rotation_speed = disk_rotation_speed
        self.device_index = int(device_index)
        self.row0, self.row1 = (0, self.height) if rows is None else (int(rows[0]), int(rows[1]))

        self._lib = _lib.load()
        cfg = _lib.Config(self.width, self.height, self.row0, self.row1, float(step_size), float(r_max),
                          float(r_disk_inner), float(r_disk_outer), float(disk_tilt),
                          0 if anti_alias == "disabled" else 1, float(aa_strength), float(disk_rotation_speed),
                          self.device_index, {"strict": _lib.MATH_STRICT, "fast": _lib.MATH_FAST, "hybrid": _lib.MATH_HYBRID}[math])
        handle = C.c_void_p()
        # frame_slots: 2 (library default) = successive render_async calls alternate between two frame slots /
        # streams and overlap; 1 = one frame at a time on the context's stream (isolated kernel timing).  The
        # library reads BHR_FRAME_SLOTS when the context is created.
        if frame_slots not in (None, 1, 2):
            raise ValueError(f"frame_slots must be 1 or 2, got {frame_slots!r}")
        saved = os.environ.get("BHR_FRAME_SLOTS")
        if frame_slots is not None:
            os.environ["BHR_FRAME_SLOTS"] = str(frame_slots)
        try:
            _lib.check(self._lib.bhr_create(C.byref(cfg), C.byref(handle)))
        finally:
            if frame_slots is not None:
                if saved is None:
                    os.environ.pop("BHR_FRAME_SLOTS", None)
                else:
                    os.environ["BHR_FRAME_SLOTS"] = saved
        self._ctx = handle
        self.frame_slots = frame_slots if frame_slots is not None else (1 if saved == "1" else 2)
        # outputs: what a frame keeps in memory besides the bg / disk layers -- "f32" (default: what render() returns),
        # "u8" (the quantised rows only: video loop, PNG sink, u8 gather), or several joined by "+" ("f32+blur+u8");
        # anything not kept is produced on demand by the call that reads it.  options: {name: value} for bhr_set_option.
        self._outputs = "f32"
        if outputs is not None:
            self.set_outputs(outputs)
        for name, value in (options or {}).items():
            self.set_option(name, value)
        self._supersample = 1
        self._supersample_threshold = None
        if supersample != 1 or supersample_threshold is not None:
            try:
                self.set_supersample(supersample, supersample_threshold)
            except Exception:
                self.close()
                raise

        # spin=A: a spinning (Kerr) hole, A = a / M (set_spin)
        # redshift="exact": the disk's g-factor of the Kerr metric instead of the reference's model (set_redshift)
        self._spin, self._force_kerr = 0.0, False
        self._redshift, self._redshift_forced = "model", False
        self._kerr_dv2 = None              # "v2" / "v2_volume" while the Kerr march shades a Disk V2 source (use_kerr_disk_v2)
        self._kerr_anti_alias = None       # the LOD strength while the Kerr march carries ray differentials (set_kerr_anti_alias)
        if spin != 0.0 or redshift != "model":
            try:
                if spin != 0.0:
                    self.set_spin(spin)
                if redshift != "model":
                    self.set_redshift(redshift)
            except Exception:
                self.close()
                raise

        skybox = np.ascontiguousarray(skybox, dtype=np.float32)
        disk_tex = np.ascontiguousarray(disk_tex, dtype=np.float32)
        assert skybox.ndim == 3 and skybox.shape[2] == 3, "skybox must be (tex_h, tex_w, 3)"
        assert disk_tex.ndim == 3 and disk_tex.shape[2] == 4, "disk_tex must be (n_r, n_phi, 4)"
        self.tex_h, self.tex_w = skybox.shape[:2]
        self.dtex_h, self.dtex_w = disk_tex.shape[:2]
        _lib.check(self._lib.bhr_set_skybox(self._ctx, _lib.fptr(skybox), self.tex_h, self.tex_w))
        _lib.check(self._lib.bhr_set_disk_texture(self._ctx, _lib.fptr(disk_tex), self.dtex_h, self.dtex_w))
        self.num_mip_levels = int(self._lib.bhr_num_mip_levels(self._ctx))

        self.disk_texture_field = _FieldView(self._read_disk_texture, (self.dtex_h, self.dtex_w))
        self.disk_mips_field = _FieldView(self._read_mips_padded, (self.num_mip_levels, self.dtex_h, self.dtex_w))
        self._bg_ready = False
        self._parametric_gpu_ready = False

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        for ref in getattr(self, "_sinks", []):      # frame sinks hold this context: drain and free them first
            sink = ref()
            if sink is not None:
                sink.close()
        self._sinks = []
        ctx, self._ctx = getattr(self, "_ctx", None), None
        if ctx:
            self._lib.bhr_destroy(ctx)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rows(self) -> int:
        return self.row1 - self.row0

    # ------------------------------------------------------------------ textures
    def add_skybox_glow(self) -> None:
        """Milky-Way glow + clip of generate_skybox (render.py:296-341) on the device, in place; the sky given to the
        constructor must be generate_skybox(..., glow=False)."""
        _lib.check(self._lib.bhr_skybox_add_glow(self._ctx))

    def build_procedural_skybox(self, seed: int = 42, n_stars: int = 6000, starless: bool = False) -> None:
        """generate_skybox(tex_w, tex_h, seed, n_stars) (render.py:153-341) into this renderer's skybox, on the
        device: the host draws the random tables (skybox.sky_tables), bhr_skybox_build rasterises them bit-identically
        to NumPy / Pillow, bhr_skybox_add_glow adds the Milky-Way glow and clips.  The skybox given to the constructor
        only fixes the size.  ``starless``: the same sky without its baked star blobs (stars.starless_tables) -- the nebula
        and the glow of a sky whose stars are drawn as points (set_stars)."""
        from .skybox import STAR_PATCH_R, pillow_bilinear_coeffs, sky_tables
        t = sky_tables(self.tex_w, self.tex_h, seed, n_stars)
        if starless:
            from .stars import starless_tables
            t = starless_tables(t)
        ch, cw = t["coarse_u8"].shape[:2]
        kh, bh = pillow_bilinear_coeffs(cw, self.tex_w)
        kv, bv = pillow_bilinear_coeffs(ch, self.tex_h)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
        coarse = np.ascontiguousarray(t["coarse_u8"])
        _lib.check(self._lib.bhr_skybox_build(
            self._ctx, self.tex_h, self.tex_w, coarse.ctypes.data_as(C.POINTER(C.c_uint8)), ch, cw, i32(kh), i32(bh), kh.shape[1],
            i32(kv), i32(bv), kv.shape[1], len(t["cx"]), _lib.fptr(t["cx"]), _lib.fptr(t["cy"]), _lib.fptr(t["colors"]),
            _lib.fptr(t["vals"]), STAR_PATCH_R))
        self.add_skybox_glow()

    def read_skybox(self) -> np.ndarray:
        out = np.empty((self.tex_h, self.tex_w, 3), dtype=np.float32)
        _lib.check(self._lib.bhr_get_skybox(self._ctx, _lib.fptr(out)))
        return out

    def update_disk_texture(self, new_disk_tex: np.ndarray) -> None:
        """Replace the disk texture and rebuild its mip chain (render.py:2292-2312)."""
        dtex_h, dtex_w = new_disk_tex.shape[:2]
        assert dtex_h == self.dtex_h and dtex_w == self.dtex_w, \
            f"Texture size mismatch: expected {self.dtex_h}x{self.dtex_w}, got {dtex_h}x{dtex_w}"
        tex = np.ascontiguousarray(new_disk_tex, dtype=np.float32)
        _lib.check(self._lib.bhr_set_disk_texture(self._ctx, _lib.fptr(tex), dtex_h, dtex_w))

    def _read_disk_texture(self) -> np.ndarray:
        out = np.empty((self.dtex_h, self.dtex_w, 4), dtype=np.float32)
        _lib.check(self._lib.bhr_get_disk_texture(self._ctx, _lib.fptr(out)))
        return out

    def read_mip_level(self, level: int) -> np.ndarray:
        h, w = self.dtex_h, self.dtex_w
        for _ in range(level):
            h, w = h // 2, w // 2
        out = np.empty((h, w, 4), dtype=np.float32)
        _lib.check(self._lib.bhr_get_disk_mip(self._ctx, level, _lib.fptr(out)))
        return out

    def _read_mips_padded(self) -> np.ndarray:
        """Same padded (levels, n_r, n_phi, 4) array disk_mips_field.to_numpy() yields (render.py:2244-2251)."""
        out = np.zeros((self.num_mip_levels, self.dtex_h, self.dtex_w, 4), dtype=np.float32)
        for lev in range(self.num_mip_levels):
            m = self.read_mip_level(lev)
            out[lev, :m.shape[0], :m.shape[1]] = m
        return out

    # ------------------------------------------------------------------ parametric texture state
    def upload_parametric_state(self, state) -> None:
        """Upload a 13-component rotating-texture state and its normalisation statistics
        (render.py:2314-2387).  ``state`` is any object with the DiskTextureRotatingState fields."""
        n_r, n_phi = state.n_r, state.n_phi
        packed = np.stack([
            state.temp_base, state.spiral, state.spiral_temp, state.turbulence, state.turb_temp,
            state.arcs, state.arcs_temp, state.rt_spikes, state.rt_temp, state.hotspot,
            state.hotspot_temp, state.az_hotspot, state.disturb_mod], axis=0).astype(np.float32)
        edge = np.ascontiguousarray(state.edge, dtype=np.float32)
        omega = np.ascontiguousarray(state.omega_rows, dtype=np.float32)
        _lib.check(self._lib.bhr_bg_init(self._ctx, n_r, n_phi, 0, 0.0, _lib.fptr(edge), _lib.fptr(omega)))
        _lib.check(self._lib.bhr_set_comp(self._ctx, _lib.fptr(np.ascontiguousarray(packed))))
        self._bg_n_r, self._bg_n_phi = n_r, n_phi
        self._install_field_views(n_r, n_phi, edge, omega)

        rt_weight = 0.20 if state.enable_rt else 0.0
        density = (0.15 + 0.10 * state.spiral + 0.30 * state.turbulence + 0.20 * state.hotspot
                   + 0.30 * state.arcs + rt_weight * state.rt_spikes) * state.disturb_mod
        density *= state.edge[:, None]
        density_p98 = float(np.percentile(density, 98))
        temp_struct = (state.spiral_temp + state.turb_temp + state.arcs_temp + state.rt_temp
                       + state.hotspot_temp) * state.disturb_mod
        pos = temp_struct > 0
        struct_scale = float(np.percentile(temp_struct[pos], 95)) if np.any(pos) else 1.0
        scaled = np.clip(temp_struct / (struct_scale + 1e-6) * 0.8, 0, 1.2)
        row_stats = np.stack([np.max(scaled, axis=1).astype(np.float32),
                              np.quantile(scaled, 0.7, axis=1).astype(np.float32)], axis=1).astype(np.float32)
        self._set_stats(density_p98, struct_scale, row_stats)
        self._param_enable_rt = 1 if state.enable_rt else 0
        self._param_color_temp = float(state.color_temp)
        self._parametric_gpu_ready = True

    def update_disk_texture_gpu(self, t_offset: float) -> None:
        """Compose the rotated texture and its mips on the device (render.py:3792-3817)."""
        assert self._parametric_gpu_ready, \
            "Must call upload_parametric_state() before update_disk_texture_gpu()"
        _lib.check(self._lib.bhr_compose_texture(self._ctx, float(t_offset), self._param_enable_rt,
                                                 self._param_color_temp))

    # ------------------------------------------------------------------ lifecycle texture pipeline
    def init_background_layer(self, n_r: int, n_phi: int, seed: int = 42) -> None:
        """render.py:3491-3547: draws az_freq / az_shear (in that order), uploads edge, omega rows and
        the permissive initial statistics."""
        rng = np.random.default_rng(seed)
        self._bg_az_freq = int(rng.integers(2, 5))
        self._bg_az_shear = float(rng.uniform(2.0, 4.0))
        edge = compute_edge_alpha(n_r).astype(np.float32)
        omega_rows = keplerian_omega_rows(n_r, self.r_disk_inner, self.r_disk_outer)
        _lib.check(self._lib.bhr_bg_init(self._ctx, n_r, n_phi, self._bg_az_freq, self._bg_az_shear,
                                         _lib.fptr(edge), _lib.fptr(omega_rows)))
        self._bg_omega_all_np = omega_rows
        self._bg_r_norm_all = np.linspace(0, 1, n_r)
        self._profile_pool = None
        self._bg_n_r, self._bg_n_phi = n_r, n_phi
        self._install_field_views(n_r, n_phi, edge, omega_rows)
        tb_init = np.clip(1.0 - np.linspace(0, 1, n_r), 0, 1) ** 1.3 * 0.25
        self._stats_np = np.array([0.5, 0.5], dtype=np.float32)
        self._row_stats_np = np.column_stack([np.maximum(tb_init, 0.25).astype(np.float32),
                                              np.maximum(tb_init * 0.8, 0.10).astype(np.float32)])
        self._param_enable_rt = 1
        self._param_color_temp = float(DISK_COLOR_TEMPERATURE)
        self._bg_ready = True

    def _install_field_views(self, n_r, n_phi, edge, omega):
        self._edge_np, self._omega_np = edge, omega
        self._comp_field = _FieldView(self.read_comp, (13, n_r, n_phi))
        self._edge_field = _FieldView(lambda: self._edge_np.copy(), (n_r,))
        self._omega_rows_field = _FieldView(lambda: self._omega_np.copy(), (n_r,))
        self._param_stats_field = _FieldView(lambda: self._stats_np.copy(), (2,))
        self._param_row_stats_field = _FieldView(lambda: self._row_stats_np.copy(), (n_r,))

    def _set_stats(self, density_p98: float, struct_scale: float, row_stats: np.ndarray) -> None:
        self._stats_np = np.array([density_p98, struct_scale], dtype=np.float32)
        self._row_stats_np = np.ascontiguousarray(row_stats, dtype=np.float32)
        _lib.check(self._lib.bhr_set_compose_stats(self._ctx, float(self._stats_np[0]), float(self._stats_np[1]),
                                                   _lib.fptr(self._row_stats_np)))

    def generate_background(self, t: float) -> None:
        """Background components comp[0,1,2,3,4,11,12] at time t on the device (render.py:3549-3562)."""
        assert self._bg_ready, "Must call init_background_layer() first"
        _lib.check(self._lib.bhr_generate_background(self._ctx, float(t)))

    def read_comp(self) -> np.ndarray:
        out = np.empty((13, self._bg_n_r, self._bg_n_phi), dtype=np.float32)
        _lib.check(self._lib.bhr_read_comp(self._ctx, _lib.fptr(out)))
        return out

    def accumulate_entity_layer(self, factories: dict, now: float, pairs_on_host: bool = False) -> None:
        """Rasterise the alive entities into comp[5:11] on the device (render.py:3564-3653).  The host hands over
        entity records (rebuilt only when a population changes); the library evaluates the fades and the per-(entity,
        row) scalars, csrc/lifecycle.hip does the per-texel work, nothing waits for the stream.
        ``pairs_on_host=True`` builds the (entity, row) pair tables in NumPy instead (round-1 path, same result)."""
        from . import lifecycle_device as ld
        if getattr(self, "_profile_pool", None) is None:
            self._profile_pool = ld.ProfilePool(self._lib, self._ctx, self._bg_n_phi)
            self._population_tables = ld.PopulationTables()
        if not pairs_on_host and ld.accumulate_population(self._lib, self._ctx, self._profile_pool, self._population_tables,
                                                          factories, now, self._bg_n_r, self._bg_n_phi,
                                                          self._bg_omega_all_np, self._bg_r_norm_all):
            return
        ld.accumulate_on_device(self._lib, self._ctx, self._profile_pool, factories, now, self._bg_n_r,
                                self._bg_n_phi, self._bg_omega_all_np, self._bg_r_norm_all)

    def recompute_interactive_stats(self) -> None:
        """Normalisation statistics from the current components, selected on the device (render.py:3655-3712)."""
        if self._bg_n_phi > 32768:
            raise ValueError(f"device statistics support textures up to 32768 columns, got {self._bg_n_phi}")
        from . import lifecycle_device as ld
        p98, scale, row_stats = ld.stats_on_device(self._lib, self._ctx, self._bg_n_r, self._bg_n_phi,
                                                   self._param_enable_rt)
        self._set_stats(p98, scale, row_stats)

    def compose_interactive_texture(self, solo_idx: int = -1) -> None:
        """Compose comp -> RGBA texture + mips with t_offset = 0 (render.py:3714-3767)."""
        if solo_idx >= 0:
            pairs = {0: [], 1: [2], 2: [1], 3: [4], 4: [3], 5: [6], 6: [5], 7: [8], 8: [7], 9: [10], 10: [9],
                     11: [], 12: []}
            keep = {solo_idx} | set(pairs.get(solo_idx, []))
            for i in range(13):
                if i not in keep:
                    _lib.check(self._lib.bhr_fill_comp_slice(self._ctx, i, 1.0 if i == 12 else 0.0))
            self.recompute_interactive_stats()
        _lib.check(self._lib.bhr_compose_texture(self._ctx, 0.0, self._param_enable_rt, self._param_color_temp))

    def eval_noise(self, coords: np.ndarray, mode: str = "simplex", octaves: int = 4,
                   persistence: float = 0.5, lacunarity: float = 2.0) -> np.ndarray:
        """Simplex / FBM values at (N, 3) coordinates (render.py:3769-3790)."""
        c = np.ascontiguousarray(coords, dtype=np.float32)
        out = np.empty(c.shape[0], dtype=np.float32)
        _lib.check(self._lib.bhr_eval_noise(self._ctx, _lib.fptr(c), c.shape[0], 0 if mode == "simplex" else 1,
                                            int(octaves), float(persistence), float(lacunarity), _lib.fptr(out)))
        return out

    # ------------------------------------------------------------------ analytic disk source
    def use_disk_v2(self, params=None, structure_params=None, seed: int = 42, volume: bool = False,
                    absorption: float = 4.0, grazing_gain: float = 1.0, substeps: int = 2) -> None:
        """Shade the disk from the Disk V2 model inside the march kernel instead of the texture
        (include/bhr_disk_v2.h: bhr_set_disk_source).  ``volume=False``: the model's mid-plane fields at
        every plane crossing; ``volume=True``: the finite-thickness emission-absorption integral of
        docs/design_ad_v2.md 4.3 (absorption coefficient per unit density, grazing-angle gain, pieces per
        RK4 step).  Pass ``params=None`` to go back to the texture."""
        from . import disk_v2 as dv
        lib = self._lib
        lib.bhr_set_disk_source.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_double]
        lib.bhr_set_disk_source.restype = C.c_int32
        lib.bhr_set_disk_volume_options.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int32]
        lib.bhr_set_disk_volume_options.restype = C.c_int32
        if params is None:
            _lib.check(lib.bhr_set_disk_source(self._ctx, 0, None, 0.0, 0.0, 0.0))
            self._dv2 = None
            return
        cp, m_sh, m_hs, t_peak = dv.reference_norms(params, structure_params, seed, ctx=self._ctx)
        if volume:
            _lib.check(lib.bhr_set_disk_volume_options(self._ctx, absorption, grazing_gain, substeps))
        _lib.check(lib.bhr_set_disk_source(self._ctx, 2 if volume else 1, C.byref(cp), m_sh, m_hs, t_peak))
        self._dv2 = (cp, m_sh, m_hs, t_peak)

    def use_kerr_disk_v2(self, params=None, structure_params=None, seed: int = 42, volume: bool = False,
                         absorption: float = 4.0, grazing_gain: float = 1.0, substeps: int = 2) -> None:
        """use_disk_v2 for a spinning hole: the Kerr march shades the Disk V2 model instead of the texture for the frames
        rendered from now on (include/bhr_disk_v2.h: bhr_set_kerr_disk_source states the model).  ``volume=False``: the
        mid-plane fields at every crossing of the plane z = 0, with the model or the exact redshift; ``volume=True``: the
        finite-thickness emission-absorption integral along every ray (the model redshift only).  It is the Kerr march's own
        setting (use_disk_v2 is the Schwarzschild marches' and stays refused with a spin): AssertionError without a spin or the
        forced Kerr march.  While it is set, Kerr ray map builds, the Kerr camera, the Kerr anti-aliasing and a set_spin that
        switches the Kerr march off are refused.  ``params=None``: back to the texture."""
        from . import disk_v2 as dv
        lib = self._lib
        lib.bhr_set_disk_volume_options.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int32]
        lib.bhr_set_disk_volume_options.restype = C.c_int32
        if params is None:
            _lib.check(lib.bhr_set_kerr_disk_source(self._ctx, 0, None, 0.0, 0.0, 0.0))
            self._kerr_dv2 = None
            return
        cp, m_sh, m_hs, t_peak = dv.reference_norms(params, structure_params, seed, ctx=self._ctx)
        if volume:
            _lib.check(lib.bhr_set_disk_volume_options(self._ctx, absorption, grazing_gain, substeps))
        _lib.check(lib.bhr_set_kerr_disk_source(self._ctx, 2 if volume else 1, C.byref(cp), m_sh, m_hs, t_peak))
        self._kerr_dv2 = "v2_volume" if volume else "v2"

    @property
    def kerr_disk_model(self) -> str:
        """The Kerr march's disk source: "texture", "v2" or "v2_volume" (use_kerr_disk_v2)."""
        return self._kerr_dv2 or "texture"

    def kerr_disk_resources(self, volume: bool = False, supersampled: bool = False, redshift: str = "model") -> dict:
        """Registers per lane, LDS and scratch bytes of the Kerr march kernel over a Disk V2 source (bhr_kerr_disk_resources)."""
        from . import kerr
        out = (C.c_int32 * 3)()
        mode = _lib.REDSHIFT_EXACT if kerr.check_redshift(redshift) == "exact" else _lib.REDSHIFT_MODEL
        _lib.check(self._lib.bhr_kerr_disk_resources(2 if volume else 1, mode, 1 if supersampled else 0, out))
        return dict(vgprs=int(out[0]), lds_bytes=int(out[1]), scratch_bytes=int(out[2]))

    # ------------------------------------------------------------------ rendering
    def camera_uniforms(self, cam_pos, fov: float, frame: int = 0, t_offset: Optional[float] = None) -> _lib.Camera:
        """f64 camera -> the f32 uniforms of render.py:3880-3897.  ``t_offset``: the disk's roll given directly (a sample of a
        shutter frame) instead of ``frame * disk_rotation_speed``."""
        eye, right, up, fwd, pw, ph = build_camera(np.array(cam_pos, dtype=np.float64), fov, self.width,
                                                   self.height)
        cam = _lib.Camera()
        cam.pos[:] = list(eye.astype(np.float32))
        cam.right[:] = list(right.astype(np.float32))
        cam.up[:] = list(up.astype(np.float32))
        cam.forward[:] = list(fwd.astype(np.float32))
        cam.pixel_width, cam.pixel_height = float(pw), float(ph)
        cam.r_escape = float(max(self.r_max, float(np.linalg.norm(eye)) * 2))
        cam.t_offset = float(frame) * self.disk_rotation_speed if t_offset is None else float(t_offset)
        return cam

    @staticmethod
    def _flags(skip_differentials: bool, skip_bloom: bool, compaction: bool = False, math=None) -> int:
        return ((_lib.SKIP_DIFFERENTIALS if skip_differentials else 0) | (_lib.SKIP_BLOOM if skip_bloom else 0)
                | (_lib.PERSISTENT if compaction else 0)
                | {None: 0, "fast": _lib.FORCE_FAST, "strict": _lib.FORCE_STRICT, "hybrid": _lib.FORCE_HYBRID}[math])

    def render_async(self, cam_pos, fov: float, frame: int = 0, skip_differentials: bool = False,
                     skip_bloom: bool = False, compaction: bool = False, math=None, lens_flare=None,
                     observer=None, observer_sky: bool = True, projection=None, projection_fov=None, light_delay=None,
                     kerr_observer=None, kerr_observer_sky: bool = True, kerr_projection=None, kerr_projection_fov=None) -> None:
        """Launch march + bloom + combine; the frame stays in HBM (counterpart of render_to_field,
        render.py:3819-3863, without the GUI flip).

        ``observer``: a velocity (beta_x, beta_y, beta_z) in units of c, |beta| <= 0.995 -- the frame as a camera sees it that
        moves through ``cam_pos`` with it (bhr_render_observer; include/bhr.h states the model, bhr_amd.observer names
        velocities): aberration, the Doppler factor in the disk's g and, with ``observer_sky``, on the sky.  Marched by the
        observer kernel whatever ``math`` the renderer has (``math=`` here is refused), (0, 0, 0) included, which is the
        strict frame.  The velocity belongs to this call alone.  None (the default): the camera stands still, as ever.

        ``projection``: "equirect" or "fisheye" -- the frame through an equirectangular panorama or an equidistant fisheye
        instead of the pinhole (bhr_render_projected; include/bhr.h states the model, bhr_amd.projection the arguments).
        ``projection_fov``: (h, v) degrees for equirect, (full_angle,) for fisheye; None: (360, 180) and (180,).  ``fov`` is then
        unused.  Combines with ``observer``; without one the camera stands still.  Marched by the projected kernel whatever
        ``math`` the renderer has (``math=`` here is refused).  None (the default): the pinhole camera, as ever.

        ``light_delay``: a scale in [0, 16] -- every disk crossing is shaded at the time its light left the gas, the texture's
        roll under t_offset - scale * T with T the coordinate time along the ray (bhr_render_delayed; include/bhr.h states the
        model).  1 is physical, larger values exaggerate, 0 is the strict frame.  Marched by the delayed kernel whatever ``math``
        the renderer has; refused together with ``observer``, ``projection`` or ``math=``.  The scale belongs to this call
        alone.  None (the default): the whole disk at the frame's one instant, as ever.

        ``kerr_observer`` / ``kerr_projection``: the same camera model in front of the Kerr march of a renderer with a spin (or
        the forced Kerr march) set (bhr_render_kerr_view; include/bhr.h states the model, bhr_amd.observer.kerr_velocity names
        velocities).  ``kerr_observer``: a velocity as the static observer at ``cam_pos`` measures it, or "rest" for the call
        without one; ``kerr_observer_sky``: the Doppler factor on the sky; ``kerr_projection`` and ``kerr_projection_fov``:
        as ``projection`` and ``projection_fov``.  Either selects the Kerr camera; at rest under the pinhole the frame is the
        Kerr frame of this method bit for bit.  Refused together with ``observer``, ``projection``, ``light_delay`` or ``math=``.
        None (the default): the hovering pinhole camera, as ever."""
        kerr_view = kerr_observer is not None or kerr_projection is not None or kerr_projection_fov is not None
        if kerr_view:
            if observer is not None or projection is not None or light_delay is not None or math is not None:
                raise ValueError("kerr_observer / kerr_projection do not combine with observer, projection, light_delay or math=: "
                                 "those marches are Schwarzschild's, the Kerr camera is the Kerr march's own")
            if kerr_projection is None and kerr_projection_fov is not None:
                raise ValueError("kerr_projection_fov without kerr_projection")
            projection, projection_fov = kerr_projection, kerr_projection_fov     # checked and turned into a bhr_projection below
        if light_delay is not None:
            if observer is not None or projection is not None or math is not None:
                raise ValueError("light_delay does not combine with observer, projection or math=: the delayed march is the strict "
                                 "Schwarzschild march of the pinhole camera that stands still")
            scale = float(light_delay)
            if not 0.0 <= scale <= 16.0:          # a NaN fails the comparison too
                raise ValueError(f"light_delay = {light_delay!r}: a scale in [0, 16]")
        if projection is not None:
            from . import projection as proj_mod
            kind, fov_h, fov_v = proj_mod.check(projection, projection_fov)
            fov = 90.0                        # the camera's basis and position are used, its image plane is not
        cam = self.camera_uniforms(cam_pos, fov, frame)
        flags = self._flags(skip_differentials, skip_bloom, compaction, math)
        if self.lens_flare if lens_flare is None else lens_flare:
            flags |= _lib.LENS_FLARE          # device twin of _apply_lens_flare (render.py:3920-4028)
        if observer is not None:
            from . import observer as obs_mod
            obs = _lib.Observer()
            obs.beta[:] = obs_mod.check_beta(observer)
            obs.sky_shift = 1 if observer_sky else 0
        if kerr_view:
            from . import observer as obs_mod
            kobs = None
            if kerr_observer is not None and not (isinstance(kerr_observer, str) and kerr_observer == "rest"):
                kobs = _lib.Observer()
                kobs.beta[:] = obs_mod.check_beta(kerr_observer)
                kobs.sky_shift = 1 if kerr_observer_sky else 0
            proj = None
            if kerr_projection is not None:
                proj = _lib.Projection(_lib.PROJ_EQUIRECT if kind == "equirect" else _lib.PROJ_FISHEYE, fov_h, fov_v, 0)
            _lib.check(self._lib.bhr_render_kerr_view(self._ctx, C.byref(cam), None if kobs is None else C.byref(kobs),
                                                      None if proj is None else C.byref(proj), flags))
            return
        if light_delay is not None:
            d = _lib.LightDelay(scale, 0)
            _lib.check(self._lib.bhr_render_delayed(self._ctx, C.byref(cam), C.byref(d), flags))
            return
        if projection is not None:
            proj = _lib.Projection(_lib.PROJ_EQUIRECT if kind == "equirect" else _lib.PROJ_FISHEYE, fov_h, fov_v, 0)
            _lib.check(self._lib.bhr_render_projected(self._ctx, C.byref(cam), C.byref(proj), None if observer is None else C.byref(obs), flags))
            return
        if observer is not None:
            _lib.check(self._lib.bhr_render_observer(self._ctx, C.byref(cam), C.byref(obs), flags))
            return
        _lib.check(self._lib.bhr_render(self._ctx, C.byref(cam), flags))

    def render_shutter_async(self, cam_positions, fov: float, t_offsets, skip_differentials: bool = False,
                             skip_bloom: bool = False, math=None, lens_flare=None) -> None:
        """Motion blur: one frame as the mean of ``len(cam_positions)`` marches (bhr_render_shutter; include/bhr.h states the
        frame).  Sample j is marched from ``cam_positions[j]`` with the disk rolled by ``t_offsets[j]``; the BG and DISK layers
        are the f32 means of the samples', the post-pass runs once on them.  1..64 samples; whole-frame contexts only."""
        cam_positions, t_offsets = list(cam_positions), list(t_offsets)
        if len(cam_positions) != len(t_offsets):
            raise ValueError(f"{len(cam_positions)} camera positions for {len(t_offsets)} t_offsets")
        cams = (_lib.Camera * max(len(cam_positions), 1))()
        for j, (pos, t) in enumerate(zip(cam_positions, t_offsets)):
            cams[j] = self.camera_uniforms(pos, fov, t_offset=t)
        flags = self._flags(skip_differentials, skip_bloom, False, math)
        if self.lens_flare if lens_flare is None else lens_flare:
            flags |= _lib.LENS_FLARE
        _lib.check(self._lib.bhr_render_shutter(self._ctx, cams, len(cam_positions), flags))

    def render_shutter(self, cam_positions, fov: float, t_offsets, skip_differentials: bool = False,
                       skip_bloom: bool = False, math=None, lens_flare=None) -> np.ndarray:
        """render_shutter_async, then the frame: (rows, width, 3) float32 in [0, 1], as render returns it."""
        self.render_shutter_async(cam_positions, fov, t_offsets, skip_differentials, skip_bloom, math, lens_flare)
        return self.read_layer(_lib.LAYER_FINAL)

    # ------------------------------------------------------------------ ray map
    def _map_frame_flags(self, skip_bloom: bool, lens_flare) -> int:
        """The flag word of a frame from either map: the lens flare as render_async decides it."""
        flare = self.lens_flare if lens_flare is None else lens_flare
        return (_lib.SKIP_BLOOM if skip_bloom else 0) | (_lib.LENS_FLARE if flare else 0)

    def _map_planes(self, read_fn, h: int, w: int, k: int, nc: int) -> dict:
        """A map's planes through its read entry point, (h, w) pixels with k records of nc floats each."""
        def read(which, shape, dtype):
            out = np.empty(shape, dtype=dtype)
            _lib.check(read_fn(self._ctx, which, out.ctypes.data, out.nbytes))
            return out
        return {"steps": read(_lib.RAYMAP_STEPS, (h, w), np.int32), "status": read(_lib.RAYMAP_STATUS, (h, w), np.int32),
                "escape_dir": read(_lib.RAYMAP_ESCAPE_DIR, (h, w, 3), np.float32),
                "crossings": read(_lib.RAYMAP_CROSSINGS, (h, w), np.int32), "hits": read(_lib.RAYMAP_HITS, (k, h, w, nc), np.float32)}

    @staticmethod
    def _map_info(info, names) -> dict:
        """The integer fields `names` of a map's info struct, and the build camera's pos / r_escape."""
        out = {name: int(getattr(info, name)) for name in names}
        out["cam_pos"] = [float(v) for v in info.cam.pos]
        out["r_escape"] = float(info.cam.r_escape)
        return out

    def build_ray_map(self, cam_pos, fov: float, skip_differentials: bool = False, supersample: int = 1) -> None:
        """March the view once with the strict arithmetic and keep what the march finds before it shades anything
        (bhr_raymap_build; include/bhr.h states the map).  The slot count is option "raymap_slots" (1..8, default 4).
        Whole-frame contexts with one ray per pixel and the texture disk source only.  Synchronises.

        ``supersample`` = k in {1, 2, 4, 8} is the map's own factor (option "raymap_supersample"; the renderer's
        ``set_supersample`` stays at 1): the map of the fine frame, k x k records per pixel, which every frame from the map
        resolves with set_supersample's filter -- bit for bit the strict frame of a renderer with ``set_supersample(k)``."""
        if supersample not in (1, 2, 4, 8):
            raise ValueError(f"build_ray_map: supersample {supersample!r} (1, 2, 4 or 8)")
        self.set_option("raymap_supersample", supersample)
        cam = self.camera_uniforms(cam_pos, fov, 0)
        _lib.check(self._lib.bhr_raymap_build(self._ctx, C.byref(cam), _lib.SKIP_DIFFERENTIALS if skip_differentials else 0))

    def render_from_ray_map_async(self, frame: int = 0, t_offset: Optional[float] = None, skip_bloom: bool = False,
                                  lens_flare=None, cam_pos=None, fov: Optional[float] = None) -> None:
        """One frame from the ray map under the scene as it is now (bhr_raymap_render): bit for bit the frame
        render_async(cam_pos, fov, frame, math="strict") of the build's view leaves, without marching it again.  The disk is
        rolled by ``t_offset``, or by ``frame * disk_rotation_speed``; the lens flare as render_async decides it.

        With ``cam_pos`` (and ``fov``): the frame seen from that camera, which has to be the build's turned about the z axis
        (a position of camera.orbit_position) over a disk that is not tilted (bhr_raymap_render_view).  The stored rays are turned
        with the camera: the frame is the strict march of the build view's rays, NOT bit-identical to
        render_async(cam_pos, ...) -- as far from it as two strict marches of symmetric views are from each other; at the
        build's own position it is the frame described above, bit for bit."""
        t = float(frame) * self.disk_rotation_speed if t_offset is None else float(t_offset)
        flags = self._map_frame_flags(skip_bloom, lens_flare)
        if cam_pos is not None:
            if fov is None:
                raise ValueError("render_from_ray_map_async: cam_pos needs fov")
            cam = self.camera_uniforms(cam_pos, fov, frame, t_offset)
            _lib.check(self._lib.bhr_raymap_render_view(self._ctx, C.byref(cam), flags))
            return
        _lib.check(self._lib.bhr_raymap_render(self._ctx, t, flags))

    def render_shutter_from_ray_map_async(self, t_offsets, cam_positions=None, fov: Optional[float] = None, skip_bloom: bool = False,
                                          lens_flare=None) -> None:
        """Motion blur from the ray map: one frame as the mean of ``len(t_offsets)`` frames from the map, without a march
        (bhr_raymap_render_shutter; include/bhr.h states the frame).  Sample j is the map's frame with the disk rolled by
        ``t_offsets[j]``, seen from ``cam_positions[j]`` -- each the build's position or a turn of it about the z axis over a disk
        that is not tilted, as render_from_ray_map_async(cam_pos=) takes them -- or, with ``cam_positions=None``, from the build
        view itself (a camera that stands still, on any disk).  The BG and DISK layers are the f32 means of the samples' in
        render_shutter_async's order and the strict arithmetic's whatever the renderer's ``math``; the post-pass runs once on them, with
        the kernels bloom_only() would take in this context (exact f32 under math="strict", split f16 under fast / hybrid).
        1..64 samples."""
        t_offsets = list(t_offsets)
        if cam_positions is not None:
            cam_positions = list(cam_positions)
            if len(cam_positions) != len(t_offsets):
                raise ValueError(f"{len(cam_positions)} camera positions for {len(t_offsets)} t_offsets")
            if fov is None:
                raise ValueError("render_shutter_from_ray_map_async: cam_positions needs fov")
        cams = (_lib.Camera * max(len(t_offsets), 1))()
        if cam_positions is None:
            info = _lib.RayMapInfo()       # without a map its camera is zeros, and the call below says that there is none
            _lib.check(self._lib.bhr_raymap_get_info(self._ctx, C.byref(info)))
            for j, t in enumerate(t_offsets):
                cams[j] = info.cam
                cams[j].t_offset = float(t)
        else:
            for j, (pos, t) in enumerate(zip(cam_positions, t_offsets)):
                cams[j] = self.camera_uniforms(pos, fov, t_offset=t)
        flags = self._map_frame_flags(skip_bloom, lens_flare)
        _lib.check(self._lib.bhr_raymap_render_shutter(self._ctx, cams, len(t_offsets), flags))

    def ray_map_info(self) -> dict:
        """The context's ray map (bhr_raymap_get_info): built, diff, slots, width, rows (the output frame's), supersample (the
        map's own factor), crossings_stored, overflow_pixels, device_bytes, ray_steps of the build (fine rays), and the build
        camera's pos / r_escape."""
        info = _lib.RayMapInfo()
        _lib.check(self._lib.bhr_raymap_get_info(self._ctx, C.byref(info)))
        return self._map_info(info, ("built", "diff", "slots", "width", "rows", "supersample", "crossings_stored", "overflow_pixels",
                                     "device_bytes", "ray_steps"))

    def ray_map_passes(self) -> dict:
        """The map's planes as NumPy arrays in (H, W[, ...]) order -- of the fine frame, (k H, k W[, ...]), for a map with
        supersample k: ``steps``, ``status`` (0 captured, 1 escaped, 2 out of
        iterations), ``escape_dir`` (H, W, 3), ``crossings``, ``hits`` (K, H, W, 5 | 9: hit_x, hit_y, to_cam xyz[, dxx, dxy, dyx,
        dyy]) and, computed on the host from the first record (output.hit_polar), ``hit_r`` and ``hit_phi`` of the first
        crossing, NaN where there is none."""
        from .output import hit_polar
        info = self.ray_map_info()
        if not info["built"]:
            raise AssertionError("no ray map has been built (build_ray_map)")
        ss = max(info["supersample"], 1)
        passes = self._map_planes(self._lib.bhr_raymap_read, info["rows"] * ss, info["width"] * ss, info["slots"], 9 if info["diff"] else 5)
        passes["hit_r"], passes["hit_phi"] = hit_polar(passes["hits"], passes["crossings"])
        return passes

    def free_ray_map(self) -> None:
        """Release the ray map's device memory (bhr_raymap_free); close() does it too."""
        _lib.check(self._lib.bhr_raymap_free(self._ctx))

    # ------------------------------------------------------------------ Kerr ray map
    def build_kerr_ray_map(self, cam_pos, fov: float, supersample: int = 1) -> None:
        """March the view once with the Kerr march of the renderer's spin and redshift mode and keep what the march finds
        before it shades anything (bhr_kerr_raymap_build; include/bhr.h states the map).  A map of its own beside build_ray_map's,
        which stays the call for a hole that does not spin.  The slot count is option "raymap_slots" (1..8, default 4);
        whole-frame renderers only.  Synchronises.

        ``supersample`` = k in {1, 2, 4, 8} is the map's own factor (option "kerr_raymap_supersample"; the renderer's
        ``set_supersample`` stays at 1): the map of the fine frame, k x k records per pixel, which every frame from the map
        resolves with set_supersample's filter -- bit for bit the marched Kerr frame of a renderer with ``set_supersample(k)``."""
        if supersample not in (1, 2, 4, 8):
            raise ValueError(f"build_kerr_ray_map: supersample {supersample!r} (1, 2, 4 or 8)")
        self.set_option("kerr_raymap_supersample", supersample)
        cam = self.camera_uniforms(cam_pos, fov, 0)
        _lib.check(self._lib.bhr_kerr_raymap_build(self._ctx, C.byref(cam), 0))
        self._kerr_map_fov = float(fov)

    def render_from_kerr_ray_map_async(self, frame: int = 0, t_offset: Optional[float] = None, cam_pos=None, skip_bloom: bool = False,
                                       lens_flare=None) -> None:
        """One frame from the Kerr ray map under the scene as it is now (bhr_kerr_raymap_render): bit for bit the frame
        render_async(cam_pos, fov, frame) of the build's view leaves, without marching it again.  The disk is rolled by
        ``t_offset``, or by ``frame * disk_rotation_speed``; the lens flare as render_async decides it.  The renderer's spin and
        redshift mode have to be the build's still.

        With ``cam_pos``: the frame seen from that camera under the build's field of view, which has to be the build's turned about
        the z axis, the spin axis (a position of camera.orbit_position; bhr_kerr_raymap_render_view).  The stored rays are turned with the camera:
        the frame is the Kerr march of the build view's rays, NOT bit-identical to render_async(cam_pos, ...); at the build's own
        position it is the frame described above, bit for bit."""
        t = float(frame) * self.disk_rotation_speed if t_offset is None else float(t_offset)
        flags = self._map_frame_flags(skip_bloom, lens_flare)
        if cam_pos is not None:
            fov = getattr(self, "_kerr_map_fov", None)
            if fov is None:
                raise AssertionError("no Kerr ray map has been built (build_kerr_ray_map)")
            cam = self.camera_uniforms(cam_pos, fov, frame, t_offset)
            _lib.check(self._lib.bhr_kerr_raymap_render_view(self._ctx, C.byref(cam), flags))
            return
        _lib.check(self._lib.bhr_kerr_raymap_render(self._ctx, t, flags))

    def render_shutter_from_kerr_ray_map_async(self, t_offsets, cam_positions=None, fov: Optional[float] = None, skip_bloom: bool = False,
                                               lens_flare=None) -> None:
        """Motion blur from the Kerr ray map: one frame as the mean of ``len(t_offsets)`` frames from the map, without a march
        (bhr_kerr_raymap_render_shutter; include/bhr.h states the frame) -- render_shutter_from_ray_map_async for the spinning
        hole.  Sample j is the map's frame with the disk rolled by ``t_offsets[j]``, seen from ``cam_positions[j]`` -- each the
        build's position or a turn of it about the z axis, the spin axis, as render_from_kerr_ray_map_async(cam_pos=) takes them
        -- or, with ``cam_positions=None``, from the build view itself (a camera that stands still; the build camera out of
        bhr_kerr_raymap_info).  ``fov`` defaults to the build's.  The BG and DISK layers are the f32 means of the samples' in
        render_shutter_async's order; the post-pass runs once on them, with the kernels bloom_only() would take in this context.
        1..64 samples."""
        t_offsets = list(t_offsets)
        if cam_positions is not None:
            cam_positions = list(cam_positions)
            if len(cam_positions) != len(t_offsets):
                raise ValueError(f"{len(cam_positions)} camera positions for {len(t_offsets)} t_offsets")
            if fov is None:
                fov = getattr(self, "_kerr_map_fov", None)
            if fov is None:
                raise AssertionError("no Kerr ray map has been built (build_kerr_ray_map)")
        cams = (_lib.Camera * max(len(t_offsets), 1))()
        if cam_positions is None:
            info = _lib.KerrRayMapDesc()   # without a map its camera is zeros, and the call below says that there is none
            _lib.check(self._lib.bhr_kerr_raymap_info(self._ctx, C.byref(info)))
            for j, t in enumerate(t_offsets):
                cams[j] = info.cam
                cams[j].t_offset = float(t)
        else:
            for j, (pos, t) in enumerate(zip(cam_positions, t_offsets)):
                cams[j] = self.camera_uniforms(pos, fov, t_offset=t)
        flags = self._map_frame_flags(skip_bloom, lens_flare)
        _lib.check(self._lib.bhr_kerr_raymap_render_shutter(self._ctx, cams, len(t_offsets), flags))

    def kerr_ray_map_info(self) -> dict:
        """The renderer's Kerr ray map (bhr_kerr_raymap_info): built, slots, width, rows (the output frame's), supersample (the
        map's own factor, bhr_kerr_raymap_get_supersample; 1 without a map), ray_steps of the build, crossings_stored,
        overflow_pixels (fine rays), device_bytes, the spin and the redshift ("model" / "exact") it was built under, and the build
        camera's pos / r_escape."""
        info = _lib.KerrRayMapDesc()
        _lib.check(self._lib.bhr_kerr_raymap_info(self._ctx, C.byref(info)))
        out = self._map_info(info, ("built", "slots", "width", "rows", "crossings_stored", "overflow_pixels", "device_bytes", "ray_steps"))
        out["spin"] = float(info.spin)
        out["redshift"] = "exact" if info.redshift == _lib.REDSHIFT_EXACT else "model"
        k = C.c_int32(1)
        _lib.check(self._lib.bhr_kerr_raymap_get_supersample(self._ctx, C.byref(k)))
        out["supersample"] = int(k.value)
        return out

    def kerr_ray_map_passes(self) -> dict:
        """The Kerr map's planes as NumPy arrays in (H, W[, ...]) order -- of the fine frame, (k H, k W[, ...]), for a map with
        supersample k: ``steps``, ``status`` (0 captured, 1 escaped, 2 out of
        iterations), ``escape_dir`` (H, W, 3), ``crossings`` and ``hits`` (K, H, W, 5: hit_x, hit_y, and to_cam xyz under the
        model redshift or the photon's momentum (p_x, p_y, 0) under the exact one)."""
        info = self.kerr_ray_map_info()
        if not info["built"]:
            raise AssertionError("no Kerr ray map has been built (build_kerr_ray_map)")
        ss = max(info["supersample"], 1)
        return self._map_planes(self._lib.bhr_kerr_raymap_read, info["rows"] * ss, info["width"] * ss, info["slots"], 5)

    def kerr_ray_map_momentum(self) -> np.ndarray:
        """The photon's covariant momentum (p_x, p_y, p_z) at each stored crossing of a Kerr map built under a Kerr polarisation,
        (K, H, W, 3) float32 in record order (bhr_kerr_raymap_read, BHR_RAYMAP_MOMENTUM); refused for a map built without."""
        info = self.kerr_ray_map_info()
        if not info["built"]:
            raise AssertionError("no Kerr ray map has been built (build_kerr_ray_map)")
        out = np.empty((info["slots"], info["rows"], info["width"], 3), dtype=np.float32)
        _lib.check(self._lib.bhr_kerr_raymap_read(self._ctx, _lib.RAYMAP_MOMENTUM, out.ctypes.data, out.nbytes))
        return out

    def free_kerr_ray_map(self) -> None:
        """Release the Kerr ray map's device memory (bhr_kerr_raymap_free); close() does it too."""
        _lib.check(self._lib.bhr_kerr_raymap_free(self._ctx))
        self._kerr_map_fov = None

    # ------------------------------------------------------------------ point stars
    def set_stars(self, dirs, flux, max_magnification: float = 32.0, max_span_deg: float = 10.0) -> None:
        """Set the star catalogue the frames from the ray map render as lensed points (bhr_set_stars; include/bhr.h states the
        model, bhr_amd.stars makes catalogues): ``dirs`` (n, 3) unit vectors in the sky's convention, ``flux`` (n, 3) RGB in
        sky value x steradian.  n = 0 removes it.  A triangle of the map whose magnification exceeds ``max_magnification`` is
        capped at it; one whose escape directions are more than ``max_span_deg`` apart contributes nothing.  Marched frames
        (render_async and its kin) ignore the catalogue; shutter frames from the map and supersampled maps refuse it.
        Synchronises."""
        self._set_catalog(self._lib.bhr_set_stars, dirs, flux, max_magnification, max_span_deg)

    def _set_catalog(self, setter, dirs, flux, max_magnification, max_span_deg) -> None:
        """bhr_set_stars or bhr_set_kerr_stars with a checked catalogue."""
        from . import stars as stars_mod
        d, f = stars_mod.check_catalog(dirs, flux)
        rec = np.ascontiguousarray(np.concatenate([d, f], axis=1), dtype=np.float32)      # bhr_star: dir[3], flux[3]
        par = _lib.StarParams(float(max_magnification), float(max_span_deg))
        _lib.check(setter(self._ctx, rec.ctypes.data if len(rec) else None, len(rec), C.byref(par)))

    def clear_stars(self) -> None:
        """Remove the star catalogue (bhr_set_stars with n = 0): every frame is again what it is without one."""
        _lib.check(self._lib.bhr_set_stars(self._ctx, None, 0, None))

    def stars_info(self) -> dict:
        """The catalogue (bhr_get_stars_info): n (0: none), bins_theta, bins_phi, max_magnification, max_span_deg, device_bytes,
        and of the last gather launched: images (deposits), capped and skipped_span (triangles)."""
        return self._catalog_info(self._lib.bhr_get_stars_info)

    def _catalog_info(self, getter) -> dict:
        info = _lib.StarsInfo()
        _lib.check(getter(self._ctx, C.byref(info)))
        out = {name: int(getattr(info, name)) for name in ("n", "bins_theta", "bins_phi", "device_bytes", "images", "capped", "skipped_span")}
        out["max_magnification"] = float(info.params.max_magnification)
        out["max_span_deg"] = float(info.params.max_span_deg)
        return out

    def read_star_plane(self) -> np.ndarray:
        """The star plane of the ray map's build view, (rows, width, 3) float32 (bhr_raymap_read, BHR_RAYMAP_STARS): the sum of
        all star images' deposits, which a frame from the map adds to its sky sample.  Gathered now if the map or the catalogue
        changed since the last time."""
        out = np.empty((self.rows, self.width, 3), dtype=np.float32)
        _lib.check(self._lib.bhr_raymap_read(self._ctx, _lib.RAYMAP_STARS, out.ctypes.data, out.nbytes))
        return out

    def stars_resources(self, turned: bool = False) -> dict:
        """Registers, LDS bytes and scratch bytes of the star gather kernel (bhr_stars_resources); ``turned``: the one of a
        turned view."""
        out = (C.c_int32 * 3)()
        _lib.check(self._lib.bhr_stars_resources(1 if turned else 0, out))
        return {"vgprs": int(out[0]), "lds_bytes": int(out[1]), "scratch_bytes": int(out[2])}

    # ------------------------------------------------------------------ Kerr point stars
    def set_kerr_stars(self, dirs, flux, max_magnification: float = 32.0, max_span_deg: float = 10.0) -> None:
        """Set the star catalogue the frames from the KERR ray map render as lensed points (bhr_set_kerr_stars; include/bhr.h
        "Kerr point stars"): the arguments and the model of set_stars, read over the Kerr map's escape directions.  A catalogue of
        its own beside set_stars', which every Kerr frame ignores -- as this one is ignored by everything but
        render_from_kerr_ray_map_async and read_kerr_star_plane.  Shutter frames from the Kerr map and supersampled Kerr maps
        refuse it; overflow pixels get no star light.  Synchronises."""
        self._set_catalog(self._lib.bhr_set_kerr_stars, dirs, flux, max_magnification, max_span_deg)

    def clear_kerr_stars(self) -> None:
        """Remove the Kerr star catalogue (bhr_set_kerr_stars with n = 0): every Kerr map frame is again what it is without one."""
        _lib.check(self._lib.bhr_set_kerr_stars(self._ctx, None, 0, None))

    def kerr_stars_info(self) -> dict:
        """The Kerr catalogue and its last gather (bhr_get_kerr_stars_info): the keys of stars_info."""
        return self._catalog_info(self._lib.bhr_get_kerr_stars_info)

    def read_kerr_star_plane(self) -> np.ndarray:
        """The star plane of the Kerr ray map's build view, (rows, width, 3) float32 (bhr_kerr_raymap_read, BHR_RAYMAP_STARS):
        what a frame from the Kerr map adds to its sky sample.  Gathered now if the map or the catalogue changed since."""
        out = np.empty((self.rows, self.width, 3), dtype=np.float32)
        _lib.check(self._lib.bhr_kerr_raymap_read(self._ctx, _lib.RAYMAP_STARS, out.ctypes.data, out.nbytes))
        return out

    def kerr_stars_resources(self, redshift: str = "model", turned: bool = False) -> dict:
        """Registers, LDS bytes and scratch bytes of the Kerr map's STARS shade kernel of a redshift mode
        (bhr_kerr_stars_resources); ``turned``: the one of a turned view."""
        if redshift not in ("model", "exact"):
            raise ValueError(f"redshift mode {redshift!r}: 'model' or 'exact'")
        out = (C.c_int32 * 3)()
        _lib.check(self._lib.bhr_kerr_stars_resources(1 if redshift == "exact" else 0, 1 if turned else 0, out))
        return {"vgprs": int(out[0]), "lds_bytes": int(out[1]), "scratch_bytes": int(out[2])}

    # ------------------------------------------------------------------ polarisation
    def set_polarization(self, field="toroidal", fraction: float = 0.7, cell: int = 16) -> None:
        """Set the polarisation the frames from the ray map compute Stokes planes under (bhr_set_polarization; include/bhr.h
        states the model, bhr_amd.polarization the presets): ``field`` a preset name or (b_r, b_phi, b_z) in the gas frame,
        ``fraction`` Pi_0 in [0, 1], ``cell`` the side of a cell of the grid (8, 16 or 32); ``field=None`` switches it off.  The
        frames themselves are what they are without it.  Turned views, shutter frames from the map and supersampled maps are
        refused while it is set; a spin, Disk V2 and row-block renderers refuse the setter.  Synchronises."""
        if field is None:
            _lib.check(self._lib.bhr_set_polarization(self._ctx, None))
            return
        from . import polarization as pol_mod
        b = pol_mod.field_vector(field)
        par = _lib.Polarization(b[0], b[1], b[2], float(fraction), int(cell))
        _lib.check(self._lib.bhr_set_polarization(self._ctx, C.byref(par)))

    def clear_polarization(self) -> None:
        """Switch the polarisation off (bhr_set_polarization with NULL)."""
        self.set_polarization(None)

    def stokes(self) -> np.ndarray:
        """Stokes I, Q, U of the last frame from the ray map, (3, rows, width) float32 (bhr_read_stokes).  chi = atan2(U, Q) / 2 is
        counted from image-right towards image-up.  Synchronises."""
        out = np.empty((3, self.rows, self.width), dtype=np.float32)
        for k in range(3):
            _lib.check(self._lib.bhr_read_stokes(self._ctx, k, _lib.fptr(out[k])))
        return out

    def stokes_cells(self) -> np.ndarray:
        """The means of I, Q, U of that frame over the cells of the grid, (gh, gw, 3) float32 (bhr_read_stokes_cells)."""
        dims = (C.c_int32 * 2)()
        _lib.check(self._lib.bhr_read_stokes_cells(self._ctx, None, dims))
        out = np.empty((int(dims[0]), int(dims[1]), 3), dtype=np.float32)
        _lib.check(self._lib.bhr_read_stokes_cells(self._ctx, _lib.fptr(out), dims))
        return out

    def stokes_resources(self, diff: bool = False) -> dict:
        """Registers, LDS bytes and scratch bytes of the Stokes kernel (bhr_stokes_resources); ``diff``: the one of a map with
        differentials."""
        out = (C.c_int32 * 3)()
        _lib.check(self._lib.bhr_stokes_resources(1 if diff else 0, out))
        return {"vgprs": int(out[0]), "lds_bytes": int(out[1]), "scratch_bytes": int(out[2])}

    def set_kerr_polarization(self, field="toroidal", fraction: float = 0.7, cell: int = 16) -> None:
        """Set the polarisation the frames from the KERR ray map compute Stokes planes under (bhr_set_kerr_polarization;
        include/bhr.h "Kerr polarisation" states the transport by the Walker-Penrose constant): the arguments of
        set_polarization; ``field=None`` switches it off.  It needs a spin or the forced Kerr march (set_spin).  Set it BEFORE
        build_kerr_ray_map: the build then keeps the photon's momentum per crossing, which a frame under it needs (a map built
        without is refused, naming the rebuild).  Turned views are refused while it is set.  stokes() and stokes_cells() read the
        planes of the last such frame.  Synchronises."""
        if field is None:
            _lib.check(self._lib.bhr_set_kerr_polarization(self._ctx, None))
            return
        from . import polarization as pol_mod
        b = pol_mod.field_vector(field)
        par = _lib.Polarization(b[0], b[1], b[2], float(fraction), int(cell))
        _lib.check(self._lib.bhr_set_kerr_polarization(self._ctx, C.byref(par)))

    def clear_kerr_polarization(self) -> None:
        """Switch the Kerr polarisation off (bhr_set_kerr_polarization with NULL)."""
        self.set_kerr_polarization(None)

    def kerr_stokes_resources(self, redshift: str = "model") -> dict:
        """Registers, LDS bytes and scratch bytes of the Kerr Stokes kernel of a redshift mode (bhr_kerr_stokes_resources)."""
        if redshift not in ("model", "exact"):
            raise ValueError(f"redshift mode {redshift!r}: 'model' or 'exact'")
        out = (C.c_int32 * 3)()
        _lib.check(self._lib.bhr_kerr_stokes_resources(_lib.REDSHIFT_EXACT if redshift == "exact" else _lib.REDSHIFT_MODEL, out))
        return {"vgprs": int(out[0]), "lds_bytes": int(out[1]), "scratch_bytes": int(out[2])}

    # ------------------------------------------------------------------ Kerr line profile
    def set_kerr_line(self, n_bins=256, g_range=(0.0, 2.0), index: float = 3.0, power: float = 4.0, emissivity: str = "powerlaw",
                      orders: str = "first", r_inner: Optional[float] = None, r_outer: Optional[float] = None, samples: bool = False) -> None:
        """Set the emission line the frames from the KERR ray map compute the profile of (bhr_set_kerr_line; include/bhr.h "Kerr
        line profile" states the model): the flux g^power eps dOmega of every counted disk crossing, binned in g over
        ``g_range`` into ``n_bins`` bins.  ``emissivity`` "powerlaw" is (r / r_inner)^-index, "texture" that times the disk
        texture's opacity under the frame's roll; ``orders`` "first" counts a pixel's first crossing (an opaque disk), "all"
        every one.  ``r_inner`` / ``r_outer``: the line's annulus inside the disk's (neither: the disk's).  ``samples`` makes
        the pass keep the per-record g and w planes (kerr_line_samples()).  ``n_bins=None`` switches the line off.  It needs
        a spin or the forced Kerr march; the frames themselves are what they are without it.  Turned views, shutter frames and
        supersampled Kerr maps are refused while it is set.  Synchronises; reserves two device rows."""
        if n_bins is None:
            _lib.check(self._lib.bhr_set_kerr_line(self._ctx, None))
            self._kerr_line = None
            return
        from . import line as line_mod
        s = line_mod.check_settings(n_bins, g_range, index, power, emissivity, orders, r_inner, r_outer)
        par = _lib.KerrLine(s["n_bins"], s["g_range"][0], s["g_range"][1], s["power"], s["index"],
                            _lib.LINE_TEXTURE if s["emissivity"] == "texture" else _lib.LINE_POWERLAW,
                            _lib.LINE_ALL if s["orders"] == "all" else _lib.LINE_FIRST,
                            0.0 if s["r_inner"] is None else s["r_inner"], 0.0 if s["r_outer"] is None else s["r_outer"])
        _lib.check(self._lib.bhr_set_kerr_line(self._ctx, C.byref(par)))
        self.set_option("kerr_line_samples", 1 if samples else 0)
        self.set_option("kerr_line_row", 0)
        self._kerr_line = s

    def clear_kerr_line(self) -> None:
        """Switch the Kerr line off (bhr_set_kerr_line with NULL)."""
        self.set_kerr_line(None)

    def kerr_line_reserve(self, n_rows: int) -> None:
        """``n_rows`` zeroed device rows for the line's histograms, e.g. one per frame of a video (bhr_kerr_line_reserve); the
        row a frame fills is ``set_kerr_line_row``'s.  Synchronises."""
        _lib.check(self._lib.bhr_kerr_line_reserve(self._ctx, int(n_rows)))

    def set_kerr_line_row(self, row: int) -> None:
        """The device row the line pass of the next frame from the Kerr map fills (option "kerr_line_row")."""
        self.set_option("kerr_line_row", int(row))

    def kerr_line_counts(self, first_row: int = 0, n_rows: int = 1):
        """The raw integers of rows [first_row, first_row + n_rows): (bins (n_rows, n_bins), under (n_rows,), over (n_rows,)),
        uint64 (bhr_kerr_line_read).  Synchronises."""
        s = getattr(self, "_kerr_line", None)
        if s is None:
            raise AssertionError("no Kerr line is set (set_kerr_line)")
        bins = np.zeros((int(n_rows), s["n_bins"]), dtype=np.uint64)
        uo = np.zeros((int(n_rows), 2), dtype=np.uint64)
        _lib.check(self._lib.bhr_kerr_line_read(self._ctx, int(first_row), int(n_rows), bins.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                uo.ctypes.data_as(C.POINTER(C.c_uint64))))
        return bins, uo[:, 0].copy(), uo[:, 1].copy()

    def kerr_line_info(self, row: int = 0) -> dict:
        """``overflow_pixels`` (pixels on the map's overflow list, which contribute nothing) and ``samples`` (counted records)
        of a device row (bhr_kerr_line_info)."""
        out = (C.c_int64 * 2)()
        _lib.check(self._lib.bhr_kerr_line_info(self._ctx, int(row), out))
        return {"overflow_pixels": int(out[0]), "samples": int(out[1])}

    def kerr_line(self, first_row: int = 0, n_rows: Optional[int] = None, energy_kev: float = 6.4) -> dict:
        """The line profile of a device row -- or, with ``n_rows``, of that many rows, one per frame: ``edges`` (n_bins + 1),
        ``flux`` per unit g, ``counts`` (the raw integers), ``under``, ``over``, ``g_mean``, ``g_red`` and ``g_blue`` (the outer
        edges of the outermost non-empty bins), ``energy`` = g E0 at the bin centres, ``spin``, ``redshift`` and the
        ``settings`` (bhr_amd.line.profile).  One row: 1-D arrays and numbers; several: a leading frame axis."""
        from . import line as line_mod
        bins, under, over = self.kerr_line_counts(first_row, 1 if n_rows is None else n_rows)
        if n_rows is None:
            bins, under, over = bins[0], under[0], over[0]
        return line_mod.profile(bins, under, over, self._kerr_line, self._spin, self._redshift, energy_kev)

    def kerr_line_samples(self) -> dict:
        """The per-record planes ``g`` and ``w`` of the last frame whose line pass kept them (set_kerr_line(samples=True)), (K, rows,
        width) float32 each in record order, 0 where a record does not count (bhr_kerr_raymap_read, BHR_RAYMAP_LINE_G / _W)."""
        info = self.kerr_ray_map_info()
        if not info["built"]:
            raise AssertionError("no Kerr ray map has been built (build_kerr_ray_map)")
        out = {}
        for name, which in (("g", _lib.RAYMAP_LINE_G), ("w", _lib.RAYMAP_LINE_W)):
            a = np.empty((info["slots"], info["rows"], info["width"]), dtype=np.float32)
            _lib.check(self._lib.bhr_kerr_raymap_read(self._ctx, which, a.ctypes.data, a.nbytes))
            out[name] = a
        return out

    def kerr_line_resources(self, redshift: str = "model", emissivity: str = "powerlaw") -> dict:
        """Registers, static LDS bytes and scratch bytes of the Kerr line kernel of a redshift mode and emissivity
        (bhr_kerr_line_resources); the histogram itself is dynamic LDS, (n_bins + 4) * 8 bytes."""
        if redshift not in ("model", "exact"):
            raise ValueError(f"redshift mode {redshift!r}: 'model' or 'exact'")
        if emissivity not in ("powerlaw", "texture"):
            raise ValueError(f"emissivity {emissivity!r}: 'powerlaw' or 'texture'")
        out = (C.c_int32 * 3)()
        _lib.check(self._lib.bhr_kerr_line_resources(_lib.REDSHIFT_EXACT if redshift == "exact" else _lib.REDSHIFT_MODEL,
                                                     1 if emissivity == "texture" else 0, out))
        return {"vgprs": int(out[0]), "lds_bytes": int(out[1]), "scratch_bytes": int(out[2])}

    def sync(self) -> None:
        _lib.check(self._lib.bhr_sync(self._ctx))

    def set_outputs(self, outputs: str) -> None:
        """Layers the V pass of every later frame stores: "f32", "blur", "u8" joined by "+" (bhr_set_outputs)."""
        bits = {"f32": _lib.OUTPUT_F32, "blur": _lib.OUTPUT_BLUR, "u8": _lib.OUTPUT_U8}
        mask = 0
        for part in outputs.split("+"):
            if part not in bits:
                raise ValueError(f"outputs: 'f32', 'blur', 'u8' joined by '+', got {outputs!r}")
            mask |= bits[part]
        _lib.check(self._lib.bhr_set_outputs(self._ctx, mask))
        self._outputs = outputs

    @property
    def outputs(self) -> str:
        """The layers last chosen with set_outputs ("f32" on a new renderer)."""
        return self._outputs

    @property
    def supersample(self) -> int:
        """k: every pixel is the box filter of k x k rays (1: one ray per pixel)."""
        return self._supersample

    @property
    def supersample_threshold(self) -> Optional[float]:
        """T of adaptive supersampling: only pixels whose k = 1 neighbours differ by more than T get the k x k rays (None: all)."""
        return self._supersample_threshold

    def set_supersample(self, k: int, threshold: Optional[float] = None) -> None:
        """k x k rays per pixel for the frames rendered from now on (bhr_set_supersample): 1, 2, 4 or 8; whole-frame contexts
        only.  threshold=T: adaptive (bhr_set_adaptive_supersample; include/bhr.h states the function) -- one ray per pixel,
        k x k for the pixels whose largest difference to an edge neighbour in the k = 1 frame exceeds T."""
        _check_supersample(k)
        _check_threshold(threshold)
        if threshold is None:
            _lib.check(self._lib.bhr_set_supersample(self._ctx, int(k)))
        else:
            _lib.check(self._lib.bhr_set_adaptive_supersample(self._ctx, int(k), float(threshold)))
        self._supersample = int(k)
        self._supersample_threshold = None if threshold is None or int(k) == 1 else float(np.float32(threshold))

    def set_spin(self, a: float, force_kerr: bool = False) -> None:
        """A spinning (Kerr) hole for the frames rendered from now on (bhr_set_spin; include/bhr.h states the model): a is the
        dimensionless a / M, |a| <= 0.998, positive with the disk's orbital motion; 0 is the Schwarzschild hole.  force_kerr
        runs the Kerr kernel at spin 0 too (tests).  Refused (ValueError naming the combination) with a tilted disk,
        anti-aliasing, a Disk V2 source, adaptive supersampling or a row-block context."""
        from . import kerr
        a = kerr.check_spin(a)
        _lib.check(self._lib.bhr_set_spin(self._ctx, a, 1 if force_kerr else 0))
        self._spin, self._force_kerr = a, bool(force_kerr)
        self._redshift_forced = False

    @property
    def spin(self) -> float:
        return self._spin

    def set_redshift(self, mode: str) -> None:
        """The redshift of the disk for the frames rendered from now on (bhr_set_redshift; include/bhr.h states both): "model",
        the reference's g-factor model with Kerr's orbital frequency, or "exact", the g-factor of the Kerr metric -- frame
        dragging, the photon's own angular momentum, and gas that plunges inside the ISCO.  "exact" is a Kerr kernel's: at
        spin 0 it turns the forced Kerr march on itself (and "model" turns that off again), so a Schwarzschild hole gets the
        exact redshift too, and what a spin refuses (set_spin) is refused."""
        from . import kerr
        mode = kerr.check_redshift(mode)
        if mode == "exact":
            if self._spin == 0.0 and not self._force_kerr:
                self.set_spin(0.0, force_kerr=True)
                self._redshift_forced = True
            _lib.check(self._lib.bhr_set_redshift(self._ctx, _lib.REDSHIFT_EXACT))
        else:
            _lib.check(self._lib.bhr_set_redshift(self._ctx, _lib.REDSHIFT_MODEL))
            if self._redshift_forced:
                self.set_spin(0.0)
        self._redshift = mode

    @property
    def redshift(self) -> str:
        return self._redshift

    def set_kerr_anti_alias(self, on: bool = True, strength: float = 1.0) -> None:
        """Anti-aliasing of the disk around a spinning hole for the frames rendered from now on (bhr_set_kerr_anti_alias;
        include/bhr.h states the model): the Kerr march carries ray differentials and every disk crossing samples the mip level
        of its footprint, min(int(clamp(lod * strength, 0, 3)), last level).  It is the Kerr march's own switch
        (anti_alias="lod_radius" is the Schwarzschild march's and stays refused with a spin): AssertionError without a spin or
        the exact redshift, ValueError for a negative or non-finite strength.  While it is on, Kerr ray map builds, the Kerr
        camera (render_async(kerr_observer=...)) and a set_spin that switches the Kerr march off are refused."""
        _lib.check(self._lib.bhr_set_kerr_anti_alias(self._ctx, 1 if on else 0, float(strength)))
        self._kerr_anti_alias = float(np.float32(strength)) if on else None

    @property
    def kerr_anti_alias(self) -> Optional[float]:
        """The LOD strength of the Kerr anti-aliasing, None while it is off (set_kerr_anti_alias)."""
        return self._kerr_anti_alias

    def kerr_anti_alias_resources(self, supersampled: bool = False, redshift: str = "model") -> dict:
        """Registers per lane, LDS and scratch bytes of the anti-aliased Kerr march kernel of a redshift mode
        (bhr_kerr_anti_alias_resources)."""
        from . import kerr
        out = (C.c_int32 * 3)()
        mode = _lib.REDSHIFT_EXACT if kerr.check_redshift(redshift) == "exact" else _lib.REDSHIFT_MODEL
        _lib.check(self._lib.bhr_kerr_anti_alias_resources(mode, 1 if supersampled else 0, out))
        return dict(vgprs=int(out[0]), lds_bytes=int(out[1]), scratch_bytes=int(out[2]))

    def kerr_info(self) -> dict:
        """Radii of the hole of the current spin, in r_s: a, r_plus, r_isco_prograde, r_isco_retrograde, r_photon_pro,
        r_photon_retro (prograde: turning with the hole)."""
        from . import kerr
        return kerr.kerr_info(self._spin)

    def kerr_resources(self, supersampled: bool = False, redshift: str = "model") -> dict:
        """Registers per lane, LDS and scratch bytes of the Kerr march kernel of a redshift mode (bhr_kerr_resources,
        bhr_kerr_redshift_resources)."""
        from . import kerr
        out = (C.c_int32 * 3)()
        if kerr.check_redshift(redshift) == "model":
            _lib.check(self._lib.bhr_kerr_resources(1 if supersampled else 0, out))
        else:
            _lib.check(self._lib.bhr_kerr_redshift_resources(_lib.REDSHIFT_EXACT, 1 if supersampled else 0, out))
        return dict(vgprs=int(out[0]), lds_bytes=int(out[1]), scratch_bytes=int(out[2]))

    def delayed_resources(self, supersampled: bool = False) -> dict:
        """Registers per lane, LDS and scratch bytes of the delayed march kernel (bhr_delayed_resources)."""
        out = (C.c_int32 * 3)()
        _lib.check(self._lib.bhr_delayed_resources(1 if supersampled else 0, out))
        return dict(vgprs=int(out[0]), lds_bytes=int(out[1]), scratch_bytes=int(out[2]))

    def observer_resources(self, supersampled: bool = False) -> dict:
        """Registers per lane, LDS and scratch bytes of the observer march kernel (bhr_observer_resources)."""
        out = (C.c_int32 * 3)()
        _lib.check(self._lib.bhr_observer_resources(1 if supersampled else 0, out))
        return dict(vgprs=int(out[0]), lds_bytes=int(out[1]), scratch_bytes=int(out[2]))

    def projected_resources(self, supersampled: bool = False) -> dict:
        """Registers per lane, LDS and scratch bytes of the projected march kernel (bhr_projected_resources)."""
        out = (C.c_int32 * 3)()
        _lib.check(self._lib.bhr_projected_resources(1 if supersampled else 0, out))
        return dict(vgprs=int(out[0]), lds_bytes=int(out[1]), scratch_bytes=int(out[2]))

    def kerr_view_resources(self, exact: bool = False, supersampled: bool = False) -> dict:
        """Registers per lane, LDS and scratch bytes of the Kerr camera's march kernel of a redshift mode (bhr_kerr_view_resources)."""
        out = (C.c_int32 * 3)()
        _lib.check(self._lib.bhr_kerr_view_resources(_lib.REDSHIFT_EXACT if exact else _lib.REDSHIFT_MODEL, 1 if supersampled else 0, out))
        return dict(vgprs=int(out[0]), lds_bytes=int(out[1]), scratch_bytes=int(out[2]))

    def adaptive_info(self) -> dict:
        """The last adaptively supersampled frame: pixels refined, how many of them were marched strict, pixels of the frame
        (bhr_adaptive_info; synchronises)."""
        out = (C.c_int64 * 3)()
        _lib.check(self._lib.bhr_adaptive_info(self._ctx, out))
        return dict(refined=int(out[0]), strict=int(out[1]), pixels=int(out[2]))

    def set_option(self, name: str, value) -> None:
        """One of the library's switches for this context (bhr_set_option; include/bhr.h lists them)."""
        _lib.check(self._lib.bhr_set_option(self._ctx, name.encode(), float(value)))

    def read_layer(self, layer: int) -> np.ndarray:
        out = np.empty((self.rows, self.width, 3), dtype=np.float32)
        _lib.check(self._lib.bhr_read_layer(self._ctx, layer, _lib.fptr(out)))
        return out

    def write_layer(self, layer: int, data: np.ndarray) -> None:
        data = np.ascontiguousarray(data, dtype=np.float32)
        if data.shape != (self.rows, self.width, 3):
            raise ValueError(f"layer must be {(self.rows, self.width, 3)}, got {data.shape}")
        _lib.check(self._lib.bhr_write_layer(self._ctx, layer, _lib.fptr(data)))

    def bloom_only(self) -> None:
        """BLUR <- bloom(DISK), FINAL <- clip(BG + DISK + BLUR, 0, 1) on the layers in the context
        (_bloom_kernel + combine, render.py:3914-3918)."""
        _lib.check(self._lib.bhr_bloom(self._ctx))

    def apply_lens_flare(self) -> None:
        """FINAL <- clip(FINAL + flare(DISK), 0, 1) on the device (_apply_lens_flare, render.py:3925-4028)."""
        _lib.check(self._lib.bhr_lens_flare(self._ctx))

    def lens_flare_sums(self) -> np.ndarray:
        """(sum glow, sum x glow, sum y glow) of the disk layer, in NumPy's summation order."""
        out = (C.c_double * 3)()
        _lib.check(self._lib.bhr_lens_flare_sums(self._ctx, out))
        return np.array(out[:], dtype=np.float64)

    def mip_lds_level(self) -> int:
        """First mip level the last anti-aliased fast march staged in LDS (option "mip_lds" / environment BHR_MIP_LDS=1), -1 if none."""
        return int(self._lib.bhr_mip_lds_level(self._ctx))

    def row_costs(self, cam_pos, fov: float, split: bool = False):
        """Ray-steps per band of 8 rows for this view (one march with BHR_ROW_COSTS, no bloom).  split=True: the pair
        (steps taken by the fast arithmetic, steps taken by the strict arithmetic) -- a hybrid frame has both."""
        cam = self.camera_uniforms(cam_pos, fov, 0)
        flags = self._flags(True, True) | _lib.ROW_COSTS
        _lib.check(self._lib.bhr_render(self._ctx, C.byref(cam), flags))
        n = (self.rows + 7) // 8
        u64p = C.POINTER(C.c_uint64)
        if split:
            fast, strict = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
            _lib.check(self._lib.bhr_get_row_costs_split(self._ctx, fast.ctypes.data_as(u64p), strict.ctypes.data_as(u64p), n))
            return fast, strict
        out = np.zeros(n, dtype=np.uint64)
        _lib.check(self._lib.bhr_get_row_costs(self._ctx, out.ctypes.data_as(u64p), n))
        return out

    def read_final_u8(self) -> np.ndarray:
        out = np.empty((self.rows, self.width, 3), dtype=np.uint8)
        _lib.check(self._lib.bhr_read_final_u8(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def read_final_u16(self) -> np.ndarray:
        """The last frame at 16 bits per sample, (rows, width, 3) uint16: (uint16)(clip(x, 0, 1) * 65535), truncated
        (bhr_read_final_u16; output.quantize16 restates it)."""
        out = np.empty((self.rows, self.width, 3), dtype=np.uint16)
        _lib.check(self._lib.bhr_read_final_u16(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint16))))
        return out

    def set_dither(self, mode) -> None:
        """Quantisation of the u8 rows: "none" / 0 (default: truncation) or "blue" / 1 (blue-noise dither, bhr_set_dither).
        Every consumer of the u8 rows -- read_final_u8, the PNG and JPEG encoders, the sinks, the y4m stream -- follows."""
        names = {"none": 0, "blue": 1, 0: 0, 1: 1}
        if isinstance(mode, bool) or mode not in names:
            raise ValueError(f"dither must be 'none' (0) or 'blue' (1), got {mode!r}")
        _lib.check(self._lib.bhr_set_dither(self._ctx, names[mode]))
        self._dither = ("none", "blue")[names[mode]]

    @property
    def dither(self) -> str:
        """"none" or "blue": the mode last chosen with set_dither."""
        return getattr(self, "_dither", "none")

    def set_grade(self, tonemap=None, exposure: float = 0.0, white: float = 2.5, transfer: str = "linear",
                  keep_hdr: bool = False) -> None:
        """The grading stage of the frames rendered from now on (bhr_set_grade; include/bhr.h states the formulas).
        ``tonemap``: None (default: off, the frame is clip(bg + disk + blur, 0, 1) as ever), "clip", "reinhard" or "aces";
        ``exposure`` in stops (-16 .. 16); ``white``: the value "reinhard" maps to 1 (2.5: bg <= 0.5, disk <= 1, blur <= 1);
        ``transfer``: "linear" or "srgb"; ``keep_hdr``: the frame keeps its scene-linear plane for read_hdr().  Every consumer
        of the frame -- read_layer, read_final_u8 / _u16, the dither, the PNG and JPEG encoders, the sinks, the y4m stream --
        follows."""
        if tonemap is None:
            _lib.check(self._lib.bhr_set_grade(self._ctx, None))
            self._grade = None
            return
        grade = check_grade(dict(tonemap=tonemap, exposure=exposure, white=white, transfer=transfer, keep_hdr=keep_hdr))
        g = _lib.Grade(TONEMAPS.index(grade["tonemap"]), TRANSFERS.index(grade["transfer"]), grade["exposure"], grade["white"],
                       int(grade["keep_hdr"]))
        _lib.check(self._lib.bhr_set_grade(self._ctx, C.byref(g)))
        self._grade = grade

    @property
    def grade(self) -> Optional[dict]:
        """The grade last chosen with set_grade: None (off) or dict(tonemap, exposure, white, transfer, keep_hdr)."""
        g = getattr(self, "_grade", None)
        return None if g is None else dict(g)

    def grade_frame(self) -> None:
        """FINAL <- grade((BG + DISK) + BLUR) on the layers in the context, without flare (bhr_grade_frame)."""
        _lib.check(self._lib.bhr_grade_frame(self._ctx))

    def read_hdr(self) -> np.ndarray:
        """The scene-linear plane of the last frame rendered or graded under set_grade(..., keep_hdr=True): (rows, width, 3)
        float32 in [0, 65504], before exposure, with the lens flare if the frame had one."""
        return self.read_layer(_lib.LAYER_HDR)

    def render(self, cam_pos: List[float], fov: float, frame: int = 0,
               skip_differentials: bool = False, skip_bloom: bool = False, observer=None, observer_sky: bool = True,
               projection=None, projection_fov=None, light_delay=None, kerr_observer=None, kerr_observer_sky: bool = True,
               kerr_projection=None, kerr_projection_fov=None) -> np.ndarray:
        """One frame -> (rows, width, 3) float32 in [0, 1]  (render.py:3865-3923).  ``observer``, ``observer_sky``: a moving
        camera, ``projection``, ``projection_fov``: an equirect or fisheye camera, ``light_delay``: the scale of the light
        delay, ``kerr_observer``, ``kerr_observer_sky``, ``kerr_projection``, ``kerr_projection_fov``: the Kerr camera, as
        render_async takes them."""
        if self.lens_flare and self.rows != self.height:
            raise ValueError("lens flare needs whole-frame sums; render row blocks through "
                             "bhr_amd.multigpu.group_render(..., lens_flare=True)")
        self.render_async(cam_pos, fov, frame, skip_differentials, skip_bloom, observer=observer, observer_sky=observer_sky,
                          projection=projection, projection_fov=projection_fov, light_delay=light_delay, kerr_observer=kerr_observer,
                          kerr_observer_sky=kerr_observer_sky, kerr_projection=kerr_projection, kerr_projection_fov=kerr_projection_fov)
        return self.read_layer(_lib.LAYER_FINAL)

    def selftest(self) -> dict:
        """Device check of the strict march's exact sqrt / divide sequences (bhr_selftest)."""
        out = (C.c_uint64 * 4)()
        _lib.check(self._lib.bhr_selftest(self._ctx, out))
        return {"bad_sqrt": out[0], "bad_div": out[1], "bad_div6": out[2], "checked": out[3]}

    def stream_map(self) -> dict:
        """Which of the context's streams share a hardware queue (bhr_debug_read, which = 3: a probe of two one-lane kernels
        per pair).  Keys "a+b" over scene / slot0 / slot1 / aux0 / aux1; True = one queue.  Diagnostics."""
        geom = (C.c_int32 * 10)()
        _lib.check(self._lib.bhr_debug_read(self._ctx, 3, None, 0, geom))
        names = ["scene", "slot0", "slot1", "aux0", "aux1"]
        out, q = {}, 0
        for i in range(5):
            for j in range(i + 1, 5):
                if geom[q] >= 0:
                    out[f"{names[i]}+{names[j]}"] = bool(geom[q])
                q += 1
        return out

    def stream_calibration(self) -> dict:
        """What the context's choice of slot 1's stream was made from (bhr_debug_read, which = 4): the candidates' frame
        rates and the one kept; "done" False until the ninth two-slot frame."""
        geom = (C.c_int32 * 10)()
        _lib.check(self._lib.bhr_debug_read(self._ctx, 4, None, 0, geom))
        return {"done": bool(geom[0]), "kept": int(geom[1]), "candidates_fps": [int(geom[2 + c]) for c in range(6)]}

    def shutter_timing(self) -> dict:
        """The accumulation launches of the last shutter frame rendered under option "shutter_timing" 1 (bhr_debug_read, which
        = 5): how many were bracketed with HIP events and the sum of their times in ms.  Synchronises."""
        geom = (C.c_int32 * 10)()
        _lib.check(self._lib.bhr_debug_read(self._ctx, 5, None, 0, geom))
        return {"launches": int(geom[0]), "ms": int(geom[1]) * 1e-6}

    def grade_timing(self) -> dict:
        """The launches of the last graded frame's grade stage under option "grade_timing" 1 (bhr_debug_read, which = 6): how
        many were bracketed with HIP events and the sum of their times in ms.  Synchronises."""
        geom = (C.c_int32 * 10)()
        _lib.check(self._lib.bhr_debug_read(self._ctx, 6, None, 0, geom))
        return {"launches": int(geom[0]), "ms": int(geom[1]) * 1e-6}

    def hybrid_launch_order(self) -> np.ndarray:
        """The partitioned launch order of the last math="hybrid" march: tile indices, the strict tiles first
        (bhr_debug_read, which = 2).  Diagnostics."""
        geom = (C.c_int32 * 10)()
        _lib.check(self._lib.bhr_debug_read(self._ctx, 2, None, 0, geom))
        out = np.empty(int(geom[0]), dtype=np.int32)
        _lib.check(self._lib.bhr_debug_read(self._ctx, 2, out.ctypes.data, out.nbytes, None))
        return out

    def hybrid_info(self) -> dict:
        """Tile split and band of the last math="hybrid" march (bhr_hybrid_info)."""
        t, b = (C.c_int32 * 2)(), (C.c_double * 2)()
        _lib.check(self._lib.bhr_hybrid_info(self._ctx, t, b))
        rep = (C.c_int32 * 2)()
        _lib.check(self._lib.bhr_hybrid_repairs(self._ctx, rep))
        return {"strict_tiles": int(t[0]), "tiles": int(t[1]), "band_below": float(b[0]), "band_above": float(b[1]),
                "repaired_pixels": int(rep[0]), "repair_capacity": int(rep[1])}

    def timing_reset(self) -> None:
        _lib.check(self._lib.bhr_timing_reset(self._ctx))

    def frame_times(self, n: int) -> np.ndarray:
        """(n, 3) march start / march end / frame end of the last n timed frames, ms after the oldest one's start."""
        out = np.empty((n, 3), dtype=np.float32)
        _lib.check(self._lib.bhr_timing_dump(self._ctx, _lib.fptr(out), n))
        return out

    def counters(self) -> dict:
        c = _lib.Counters()
        _lib.check(self._lib.bhr_get_counters(self._ctx, C.byref(c)))
        return {name: getattr(c, name) for name, _ in c._fields_}
