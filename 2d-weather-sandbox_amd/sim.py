"""Host-side mirror of the reference's simulation seam.

The reference has no class for this: ``mainScript(base, water, wall, drops)`` (app.js:1495) creates
module-scope GL objects, ``draw()`` (app.js:5686) runs ``guiControls.IterPerFrame`` iterations per frame
(app.js:5830-6005), consumers call ``gl.readPixels`` and ``prepareDownload()`` writes a save
(app.js:6575-6628). ``WeatherSim`` restates exactly that surface on top of the C ABI (engine.py).
"""
from __future__ import annotations

import datetime as _dt
import sys
from typing import Any, Dict, Optional, Sequence

import numpy as np

from . import codec, params
from .engine import Handle

TIME_PER_ITERATION = 0.00008  # hours of simulated time per iteration (app.js:449)
_EPOCH = _dt.datetime(1970, 1, 1)


def _js_date(year: int, month_index: int, day: int, hour: int = 0, minute: int = 0, second: int = 0) -> _dt.datetime:
    """``new Date(year, monthIndex, day, h, m, s)`` with JavaScript's roll-over rules (month index 12 = January of the
    next year, day 0 = last day of the previous month); the arguments are already truncated to integers."""
    year += month_index // 12
    return _dt.datetime(year, month_index % 12 + 1, 1) + _dt.timedelta(days=day - 1, hours=hour, minutes=minute, seconds=second)


def initial_sim_datetime(month: float, time_of_day: float, day_night_cycle: bool) -> _dt.datetime:
    """startSimulation()'s clock (app.js:3902-3910): ``new Date(2000, floor(month) - 1, (month % 1) * 30.417)`` -- the
    Date constructor truncates the fractional day -- and, with the day/night cycle on, ``onUpdateTimeOfDaySlider`` /
    ``onUpdateMonthSlider`` (app.js:6494-6507): ``setHours(timeOfDay, (timeOfDay % 1) * 60)`` then
    ``setMonth(month - 0.96, ((month - 0.96) % 1) * 30)``, every argument truncated toward zero."""
    import math
    t = _js_date(2000, math.floor(month) - 1, int((month % 1) * 30.417))
    if day_night_cycle:
        t = t.replace(hour=0, minute=0) + _dt.timedelta(hours=int(time_of_day), minutes=int((time_of_day % 1) * 60))
        m = month - 0.96
        t = _js_date(t.year, int(m), int((m % 1) * 30), t.hour, t.minute, t.second)
    return t


def advance_sim_datetime(t: _dt.datetime, delta_hours: float):
    """The clock part of ``updateSunlight(deltaT_hours)`` (app.js:6513-6516): ``new Date(getTime() + deltaT_hours * 3600 * 1000)`` -- a
    Date holds whole milliseconds, the sum is truncated -- and the two sliders recomputed from it. Returns (t, timeOfDay, month)."""
    ms = int((t - _EPOCH) / _dt.timedelta(milliseconds=1) + delta_hours * 3600 * 1000)
    t = _EPOCH + _dt.timedelta(milliseconds=ms)
    return t, t.hour + t.minute / 60.0 + t.second / 3600.0, t.month + t.day / 30.5 + t.hour / 720.0


class WeatherSim:
    def __init__(self, X: int, Y: int, base, water, wall, droplets=None, settings: Optional[Dict[str, Any]] = None, *,
                 sun_angle_deg: Optional[float] = None, quad_scale: int = 0, pass_mask: int = params.PASS_ALL, columns=None,
                 handle: Optional[Handle] = None):
        """``mainScript``: take the four initial arrays + saved settings (app.js:1495, 3375-3399, 5189-5317), or -- for a
        new simulation -- the 1-D setup descriptors ``columns`` (synth.terrain_columns) that the device expands.
        ``handle``: an engine handle somebody else owns (a member of a ``WeatherEnsemble``) instead of a new one."""
        self.X, self.Y = int(X), int(Y)
        self.gui = params.merge_settings(settings)
        n_drops = 0 if droplets is None else int(np.asarray(droplets).size // 5)
        self._h = handle if handle is not None else Handle(self.X, self.Y, n_drops)
        if columns is not None:
            self._h.setup_columns(columns, droplets)
        else:
            self._h.upload(base, water, wall, droplets)
        self._quad_scale = int(quad_scale)
        self._pass_mask = int(pass_mask)
        self._manual_sun = sun_angle_deg
        self._inactive_pushed = False
        self._placement_told = False
        self.verbose = True
        # startSimulation(): clock from the saved month / time of day (app.js:3902-3910)
        self.sim_datetime = initial_sim_datetime(float(self.gui["month"]), float(self.gui["timeOfDay"]), bool(self.gui.get("dayNightCycle")))
        self.brush = {"userInputType": -1, "userInputValues": (0.0, 0.0, 0.0, 0.0), "userInputMove": (0.0, 0.0)}
        self.airplane = (0.0, 0.0, 0.0, 0.0)
        self._push_uniforms()

    # ---- construction helpers ----
    @classmethod
    def new_simulation(cls, X: int, Y: int, settings: Optional[Dict[str, Any]] = None, *, n_droplets: Optional[int] = None,
                       seed: float = 0.5, height_mult: float = 0.3, **kw) -> "WeatherSim":
        """Start-up without a save file: the setup pass (setupShader.frag:36-92) + ``initRainDrops`` (app.js:4901-4913),
        one droplet per 25 cells like the reference (the save format relies on that count)."""
        from . import synth
        gui = params.merge_settings(settings)
        n = codec.num_droplets(X, Y) if n_droplets is None else int(n_droplets)
        cols = synth.terrain_columns(X, Y, gui, seed=seed, height_mult=height_mult)
        return cls(X, Y, None, None, None, synth.init_rain_drops(n) if n else None, settings, columns=cols, **kw)

    @classmethod
    def from_save(cls, sf: "codec.SaveFile | str", **kw) -> "WeatherSim":
        """``loadData()`` (app.js:1256-1366)."""
        if isinstance(sf, str):
            sf = codec.load(sf)
        return cls(sf.X, sf.Y, sf.base, sf.water, sf.wall, sf.droplets, sf.settings, **kw)

    @classmethod
    def _on_cloned_handle(cls, handle: Handle, other: "WeatherSim") -> "WeatherSim":
        """A ``WeatherSim`` on ``handle`` (a member of a ``WeatherEnsemble``) whose engine state ALREADY is a device-side clone of
        ``other``'s: no upload, no host arrays -- only the host state is taken over."""
        self = cls.__new__(cls)
        self.X, self.Y = other.X, other.Y
        self._h = handle
        self.verbose = False
        self._placement_told = True  # (members never search for a placement)
        self._take_host_state(other)
        return self

    def _take_host_state(self, other: "WeatherSim"):
        """What a ``WeatherSim`` keeps on the host next to its engine handle: gui, sounding, clock, sun, brush."""
        self.gui = dict(other.gui)
        self._quad_scale, self._pass_mask, self._manual_sun = other._quad_scale, other._pass_mask, other._manual_sun
        self._inactive_pushed = other._inactive_pushed
        self._sounding = getattr(other, "_sounding", None)
        self.sim_datetime = other.sim_datetime
        self.brush = dict(other.brush)
        self.airplane = tuple(other.airplane)

    def copy_from(self, other: "WeatherSim"):
        """This simulation becomes ``other``'s: the engine state on the device (``Handle.copy_from``: fields, droplets, iteration counter,
        parameters -- not the engine options) and the host state that goes with it (gui, sounding, clock, sun, brush). Both go on
        independently afterwards."""
        if other is self:
            return
        if (self.X, self.Y) != (other.X, other.Y):
            raise ValueError(f"copy_from: {other.X} x {other.Y} into {self.X} x {self.Y}")
        self._h.copy_from(other._h)
        self._take_host_state(other)

    # ---- parameters ----
    def uniforms(self) -> Dict[str, Any]:
        u = params.uniforms_from_gui(self.gui, self.Y, sun_angle_deg=self._manual_sun, quad_scale=self._quad_scale,
                                     pass_mask=self._pass_mask)
        u.update(self.brush)
        u["airplaneValues"] = self.airplane
        # keep the engine's own 600-iteration measurement after the first push (app.js:5957-5966)
        u["inactiveDroplets"] = -1.0 if self._inactive_pushed else 0.0
        if getattr(self, "_sounding", None) is not None:
            u["sounding_T"], u["sounding_W"], u["sounding_Vel"] = self._sounding
        return u

    def _push_uniforms(self):
        u = self.uniforms()
        p = params.fill_struct(params.WxParams(), u)
        self._h.set_params(p, u["initial_T"], u.get("sounding_T"), u.get("sounding_W"), u.get("sounding_Vel"))
        self._inactive_pushed = True

    def set_sounding(self, raw_sounding):
        """Load a real sounding for the ``soundingForcing`` slider (app.js:5444-5463); ``raw_sounding`` as in
        ``params.sounding_arrays`` (scraper order: top of the sounding first)."""
        sim_h = float(self.gui["simHeight"])
        self._sounding = params.sounding_arrays(raw_sounding, self.Y, sim_h, sim_h * float(self.gui["dryLapseRate"]) / 1000.0)
        self._push_uniforms()

    def set_gui(self, **changes):
        """Change guiControls entries and push the uniforms (dat.GUI onChange + setGuiUniforms, app.js:3401-3443)."""
        for k in changes:
            if k not in params.GUI_DEFAULTS:
                raise KeyError(k)
        self.gui.update(changes)
        self._push_uniforms()

    def set_brush(self, input_type: int, x: float, y: float, intensity: float, brush_size: float, move=(0.0, 0.0)):
        """Per-frame brush uniforms (app.js:5749-5808); input_type -1 = mouse released."""
        self.brush = {"userInputType": int(input_type), "userInputValues": (x, y, intensity, brush_size * 0.5),
                      "userInputMove": tuple(move)}
        self._push_uniforms()

    def update_sunlight(self, delta_hours: Optional[float]):
        """``updateSunlight(deltaT_hours)`` (app.js:6510-6561): advance the clock, recompute the sun."""
        if delta_hours is not None:
            self.sim_datetime, self.gui["timeOfDay"], self.gui["month"] = advance_sim_datetime(self.sim_datetime, delta_hours)
        self.gui["sunAngle"] = params.sun_angle_from_time(self.gui["timeOfDay"], self.gui["month"], self.gui["latitude"])
        self._manual_sun = None
        self._push_uniforms()

    # ---- the frame loop ----
    def step(self, n_iter: Optional[int] = None):
        """Simulation part of ``draw()``: sun update for the frame, then n iterations (app.js:5814-6005)."""
        n = int(self.gui["IterPerFrame"]) if n_iter is None else int(n_iter)
        if self.gui.get("dayNightCycle") and self._manual_sun is None:
            self.update_sunlight(TIME_PER_ITERATION * n)
        self._h.step(n)
        if not self._placement_told:  # the engine looked for a fast placement of its planes inside the first step of a big grid: say so once
            self._placement_told = True
            pi = self._h.placement_info()
            if pi is not None and self.verbose:
                print(f"[wxsim] placement search: {pi[0]:.4f} ms / iteration on the first allocations, {pi[1]:.4f} kept", file=sys.stderr)

    def sync(self):
        self._h.sync()

    @property
    def iter_num(self) -> int:
        return self._h.iter

    @iter_num.setter
    def iter_num(self, v: int):
        self._h.iter = v

    # ---- readback (gl.readPixels / getBufferSubData call sites) ----
    def read_rect(self, field: str, x=0, y=0, w=None, h=None, **kw):
        return self._h.read_rect(field, x, y, w, h, **kw)

    def read_particles(self, first=0, count=None):
        return self._h.read_particles(first, count)

    def diagnostics(self) -> dict:
        """Conservation sums (exact), extremes and the non-finite census of the current state, from one device pass (Handle.diagnostics)."""
        return self._h.diagnostics()

    def measure_station(self, x: int, y: int):
        """Weatherstation.measure (app.js:1084-1092): FB0 base 1x3 and water 1x2 starting at (x, y-1)."""
        return self.read_rect("BASE_CUR", x, y - 1, 1, 3), self.read_rect("WATER_0", x, y - 1, 1, 2)

    def sounding_column(self, x: int):
        """soundingGraph.draw (app.js:3931-3943): FB1 column reads; wall as Int32."""
        return (self.read_rect("BASE_DISP", x, 0, 1, self.Y), self.read_rect("WATER_CUR", x, 0, 1, self.Y),
                self.read_rect("WALL_DISP", x, 0, 1, self.Y, int32=True))

    def inactive_droplets(self) -> float:
        """readPixels(0,0) of the feedback texture (app.js:5958-5961)."""
        return float(self.read_rect("PRECIP_FB", 0, 0, 1, 1)[0, 0, 0])

    def lightning(self):
        return self.read_rect("LIGHTNING")

    def to_save(self) -> codec.SaveFile:
        """``prepareDownload()`` (app.js:6584-6613): FB0 = base_0, water_0 (post-boundary!), wall_0 + particles.
        Deviation: the reference always stores particle buffer 0; this stores the current buffer."""
        gui = {k: v for k, v in self.gui.items()}
        return codec.SaveFile(self.X, self.Y, self.read_rect("BASE_CUR"), self.read_rect("WATER_0"), self.read_rect("WALL_CUR"),
                              self.read_particles() if self._h.n_droplets else np.zeros((0, 5), np.float32), [], gui)

    # ---- profiling ----
    def profile(self, enable: bool):
        self._h.profile(enable)

    def profile_read(self):
        return self._h.profile_read()

    @property
    def handle(self) -> Handle:
        return self._h


class WeatherEnsemble:
    """B ``WeatherSim`` members of one size on one ``engine.Ensemble``: one scene (arrays, a save file or a synthetic terrain) plus
    per-member setting overrides -- a sweep over the sliders, a perturbed ensemble. Every member is a full ``WeatherSim`` (``set_gui``,
    ``set_brush``, ``read_rect``, ``read_particles`` ...); ``step`` advances all of them in one marching launch per iteration, their
    droplets in one set of particle launches."""

    def __init__(self, n_members: int, X: int, Y: int, base, water, wall, settings: Optional[Dict[str, Any]] = None,
                 overrides: Optional[Sequence[Optional[Dict[str, Any]]]] = None, *, perturb=None, columns=None, droplets=None, **kw):
        """``overrides[i]``: guiControls entries of member i on top of ``settings``; ``perturb(i, base, water, wall)`` may return member
        i's own copies of the arrays -- three, or four with the member's own droplet pool; ``droplets``: one pool (n x 5) that every
        member starts from (all members hold the same number of droplets)."""
        from .engine import Ensemble
        if overrides is not None and len(overrides) != n_members:
            raise ValueError("one overrides entry per member")
        for o in overrides or ():
            for k in o or ():  # (as set_gui: an unknown name would be merged and never reach a uniform)
                if k not in params.GUI_DEFAULTS:
                    raise KeyError(k)
        n_drops = 0 if droplets is None else int(np.asarray(droplets).size // 5)
        self._e = Ensemble(n_members, X, Y, n_drops)
        self.members = []
        for i in range(n_members):
            st = dict(settings or {})
            st.update((overrides[i] if overrides is not None else None) or {})
            arrays = (base, water, wall) if perturb is None or columns is not None else tuple(perturb(i, base, water, wall))
            b, w, wl = arrays[:3]
            d = arrays[3] if len(arrays) > 3 else droplets
            m = WeatherSim(X, Y, b, w, wl, d if n_drops else None, st, columns=columns, handle=self._e[i], **kw)
            m.verbose = False
            m._placement_told = True  # (members never search for a placement)
            self.members.append(m)

    @classmethod
    def from_save(cls, n_members: int, sf: "codec.SaveFile | str", overrides=None, **kw) -> "WeatherEnsemble":
        if isinstance(sf, str):
            sf = codec.load(sf)
        drops = sf.droplets if sf.droplets is not None and len(sf.droplets) else None
        return cls(n_members, sf.X, sf.Y, sf.base, sf.water, sf.wall, sf.settings, overrides, droplets=drops, **kw)

    @classmethod
    def new_simulation(cls, n_members: int, X: int, Y: int, settings: Optional[Dict[str, Any]] = None, overrides=None, *, seed: float = 0.5,
                       height_mult: float = 0.3, n_droplets: int = 0, droplet_seed: int = 1, **kw) -> "WeatherEnsemble":
        """``n_droplets`` per member, initialised on the device (wx_init_droplets; member i with seed ``droplet_seed + i``)."""
        from . import synth
        cols = synth.terrain_columns(X, Y, params.merge_settings(settings), seed=seed, height_mult=height_mult)
        n = int(n_droplets)
        ens = cls(n_members, X, Y, None, None, None, settings, overrides, columns=cols, droplets=synth.init_rain_drops(n) if n else None, **kw)
        for i, m in enumerate(ens.members if n else ()):
            m.handle.init_droplets(int(droplet_seed) + i)
        return ens

    @classmethod
    def from_sim(cls, sim: WeatherSim, n_members: int, overrides: Optional[Sequence[Optional[Dict[str, Any]]]] = None) -> "WeatherEnsemble":
        """``n_members`` members cloned ON THE DEVICE from a running ``WeatherSim`` (its spun-up state: light, curl, feedback textures,
        lightning, droplets, iteration counter -- what an upload cannot carry), no host arrays; ``overrides[i]``: guiControls entries of
        member i on top of the simulation's. Follow with ``perturb`` to make the members differ."""
        from .engine import Ensemble
        if overrides is not None and len(overrides) != n_members:
            raise ValueError("one overrides entry per member")
        for o in overrides or ():
            for k in o or ():
                if k not in params.GUI_DEFAULTS:
                    raise KeyError(k)
        self = cls.__new__(cls)
        self._e = Ensemble(n_members, sim.X, sim.Y, sim.handle.n_droplets)
        self._e[0].copy_from(sim.handle)
        self._e.broadcast(0)
        self.members = []
        for i in range(n_members):
            m = WeatherSim._on_cloned_handle(self._e[i], sim)
            if overrides is not None and overrides[i]:
                m.set_gui(**overrides[i])
            self.members.append(m)
        return self

    def broadcast(self, i: int, members=None):
        """Every selected member (None: all others) becomes member ``i``: its engine state on the device (``engine.Ensemble.broadcast``)
        and its host state (gui, sounding, clock, sun, brush)."""
        self._e.broadcast(i, members)
        from .engine import _member_mask
        mask = _member_mask(len(self.members), members)
        src = self.members[i]
        for k, m in enumerate(self.members):
            if k != i and (mask is None or mask[k]):
                m._take_host_state(src)

    def perturb(self, field: str, amplitude, **kw):
        """``engine.Ensemble.perturb``: smooth device-side noise on one field of the selected members (mode, scale, seed, wrap_x, rect,
        members, lo, hi)."""
        self._e.perturb(field, amplitude, **kw)

    def assimilate(self, observations, *, loc=(0.0, 0.0), rect=None, members=None, wrap_x=None, **kw) -> list:
        """``engine.Ensemble.assimilate``: the selected members pulled towards point observations -- ``(field, x, y, channel, value,
        error_var)`` tuples, e.g. a nature run's values at its weather stations -- by a serial ensemble square-root filter on the
        device (loc, rect, members, gain_base, gain_water, lo_* / hi_*). ``wrap_x`` defaults to the members' ``wrapHorizontally``.
        Returns one dict per observation (applied, prior_mean, prior_var, innovation, alpha)."""
        if wrap_x is None:
            wrap_x = bool(self.members[0].gui.get("wrapHorizontally", True))
        return self._e.assimilate(observations, loc=loc, rect=rect, members=members, wrap_x=wrap_x, **kw)

    def save_prior(self, field: str, rect=None, members=None):
        """``engine.Ensemble.save_prior``: the device-side snapshot of one field that ``inflate`` relaxes to in the modes "rtps" / "rtpp"."""
        self._e.save_prior(field, rect, members)

    def drop_prior(self, field: str):
        """``engine.Ensemble.drop_prior``: frees that field's snapshot."""
        self._e.drop_prior(field)

    def inflate(self, field: str, coef, **kw):
        """``engine.Ensemble.inflate``: covariance inflation about the ensemble mean (mode "const") or relaxation to the saved prior
        ("rtps", "rtpp") of one field of the selected members (mode, rect, members, lambda_bounds, lo, hi, want_lambda)."""
        return self._e.inflate(field, coef, **kw)

    def covariance(self, field: str, predictors, **kw) -> dict:
        """``engine.Ensemble.covariance``: the sample covariance, correlation and regression slope, over the selected members, between
        every cell-channel of one field and up to 8 scalar predictors, in one pass on the device (source, rect, members, want)."""
        return self._e.covariance(field, predictors, **kw)

    def correlation(self, field: str, point, *, source="current", rect=None, members=None) -> np.ndarray:
        """The ensemble correlation of ``field`` with the members' current value at ``point`` = (field name, x, y, channel), as one
        (h, w, 4) plane: where it sinks into the sampling noise of about 1 / sqrt(n - 1) is where a localization half-width belongs."""
        return self._e.covariance(field, [tuple(point)], source=source, rect=rect, members=members, want=("corr",))["corr"][0]

    def sensitivity(self, metric, field: str, *, rect=None, members=None) -> dict:
        """Ensemble sensitivity analysis (Torn and Hakim 2008): the regression of a per-member forecast metric J_k onto the prior that
        ``save_prior`` took of ``field``. ``metric``: one number per member, or a callable that is given the list of the members'
        ``diagnostics`` entries and returns them. Returns ``slope`` = dJ/dx and ``corr``, (h, w, 4) each, and ``result`` (the metric's
        mean and variance over the members). Without a saved prior the library's WX_E_STATE message comes through."""
        values = metric(self.diagnostics()) if callable(metric) else metric
        out = self._e.covariance(field, [np.asarray(values, np.float64)], source="prior", rect=rect, members=members, want=("slope", "corr"))
        return {"slope": out["slope"][0], "corr": out["corr"][0], "result": out["results"][0]}

    def gram(self, field: str, rect=None, members=None, center="mean") -> dict:
        """``engine.Ensemble.gram``: the selected members (at most 64) in member space -- per channel the n x n matrix of the exact
        inner products, over the cells of ``rect``, of the members' deviations from their mean (``center`` "mean") or of their raw
        values ("none"): ``gram`` (4, n, n) float64, the counts ``n_entered`` / ``n_excluded`` / ``n_overflow`` and ``members``."""
        return self._e.gram(field, rect, members, center)

    def distances(self, field: str, weights=(1, 1, 1, 1), *, rect=None, members=None, center="mean") -> np.ndarray:
        """How far the selected members are from one another over ``rect``: the n x n matrix of sqrt(sum_c w_c (G_aa + G_bb - 2 G_ab))
        from ``gram``, clipped at 0; ``weights`` put the channels on one scale (e.g. one over their variances). The distance between
        two members does not depend on the centre; "mean" keeps the matrix entries small. The difference cancels: it costs about
        2^-24 of G_aa -- the rounding of the float terms the sums are made of -- which two nearly equal members feel and which is
        harmless for clustering."""
        g = self.gram(field, rect, members, center)["gram"]
        w = np.asarray(weights, np.float64).reshape(4)
        m = np.tensordot(w, g, axes=(0, 0))
        d = np.diag(m)
        return np.sqrt(np.maximum(d[:, None] + d[None, :] - 2.0 * m, 0.0))

    def medoid(self, field: str, weights=(1, 1, 1, 1), *, rect=None, members=None) -> int:
        """The most representative member: the index of the selected member whose summed ``distances`` to the others is smallest
        (the first of them if several are)."""
        from .engine import _selected
        d = self.distances(field, weights, rect=rect, members=members)
        return int(_selected(len(self.members), members)[int(np.argmin(d.sum(axis=1)))])

    def eofs(self, field: str, k: int = 3, weights=(1, 1, 1, 1), *, rect=None, members=None) -> dict:
        """The leading ``k`` empirical orthogonal functions of ``field`` over ``rect``, by the member-space route: M = sum_c w_c G_c /
        (n - 1) from ``gram`` has the non-zero eigenvalues of the (channel-weighted) spatial covariance, ``numpy.linalg.eigh`` of that
        n x n matrix gives them, and ONE ``covariance`` call with the unit-variance principal-component scores as predictors turns
        them into patterns -- so k <= 8. Returns ``eigenvalues`` (n, descending), ``explained`` (their fractions of the trace),
        ``pcs`` (n, k: unit sample variance, the members in ascending index) and ``patterns`` (k, h, w, 4): the covariance of every
        cell-channel with PC j, in the field's own units (the EOF times sqrt(eigenvalue), unweighted); NaN where a cell does not
        enter. The sign of a pattern and its PC is eigh's."""
        from .engine import ENS_COV_MAX, _selected
        k = int(k)
        if k < 1 or k > ENS_COV_MAX:
            raise ValueError(f"eofs: k = {k}: 1 .. {ENS_COV_MAX} (WX_ENS_COV_MAX: the patterns come from one covariance call)")
        out = self.gram(field, rect, members, "mean")
        sel = _selected(len(self.members), members)
        n = len(sel)
        if k > n:
            raise ValueError(f"eofs: k = {k} patterns from {n} members")
        w = np.asarray(weights, np.float64).reshape(4)
        lam, vec = np.linalg.eigh(np.tensordot(w, out["gram"], axes=(0, 0)) / (n - 1))
        lam, vec = lam[::-1], vec[:, ::-1]
        total = lam.sum()
        pcs = vec[:, :k] * np.sqrt(n - 1.0)
        values = np.zeros((k, len(self.members)), np.float64)
        values[:, sel] = pcs.T
        patterns = self._e.covariance(field, list(values), rect=rect, members=members, want=("cov",))["cov"]
        return {"eigenvalues": lam, "explained": lam / total if total > 0 else np.full_like(lam, np.nan), "pcs": pcs, "patterns": patterns, "members": out["members"]}

    def analysis(self, observations, *, relax=None, inflate=None, **assimilate_kw) -> list:
        """One analysis step of a cycling filter: ``save_prior`` of the state fields with a non-zero gain (only with ``relax``), then
        ``assimilate(observations, **assimilate_kw)``, then the inflation -- ``relax`` = ("rtps", alpha) or ("rtpp", alpha): relaxation
        to the prior just saved; ``inflate`` = lambda: constant inflation about the analysis mean (after the relaxation if both are
        given). alpha / lambda: one value or one per channel; they act on the channels the analysis updates (gain != 0), inside its
        ``rect`` and on its ``members``. The clamps of the analysis (lo_* / hi_*) hold for the inflation too. Returns the
        per-observation results of ``assimilate``."""
        from .engine import _four
        gains = {"BASE_CUR": _four(assimilate_kw.get("gain_base", (0, 0, 0, 1)), 0.0), "WATER_CUR": _four(assimilate_kw.get("gain_water", 0.0), 0.0)}
        fields = [f for f, g in gains.items() if any(v != 0.0 for v in g)]
        rect, members = assimilate_kw.get("rect"), assimilate_kw.get("members")
        if relax is not None:
            mode, alpha = relax
            if mode not in ("rtps", "rtpp"):
                raise ValueError('relax: ("rtps", alpha) or ("rtpp", alpha)')
            for f in fields:
                self.save_prior(f, rect, members)
        res = self.assimilate(observations, **assimilate_kw)
        for f in fields:
            suffix = "base" if f == "BASE_CUR" else "water"
            clamp = dict(lo=assimilate_kw.get("lo_" + suffix), hi=assimilate_kw.get("hi_" + suffix))
            if relax is not None:
                self.inflate(f, [a if g != 0.0 else 0.0 for a, g in zip(_four(alpha, 0.0), gains[f])], mode=mode, rect=rect, members=members, **clamp)
            if inflate is not None:
                self.inflate(f, [l if g != 0.0 else 1.0 for l, g in zip(_four(inflate, 1.0), gains[f])], mode="const", rect=rect, members=members, **clamp)
        return res

    def __len__(self):
        return len(self.members)

    def __getitem__(self, i: int) -> WeatherSim:
        return self.members[i]

    def step(self, n_iter: Optional[int] = None):
        """One frame for every member: the members' own sun updates, then n iterations of all of them together (``IterPerFrame`` of
        member 0 by default)."""
        n = int(self.members[0].gui["IterPerFrame"]) if n_iter is None else int(n_iter)
        for m in self.members:
            if m.gui.get("dayNightCycle") and m._manual_sun is None:
                m.update_sunlight(TIME_PER_ITERATION * n)
        self._e.step(n)

    def sync(self):
        self._e.sync()

    def diagnostics(self) -> list:
        return self._e.diagnostics()

    def stats(self) -> dict:
        return self._e.stats()

    def particle_stats(self) -> dict:
        return self._e.particle_stats()

    def statistics(self, field: str, x: int = 0, y: int = 0, w: Optional[int] = None, h: Optional[int] = None, *, members=None,
                   threshold=(0, 0, 0, 0), want=None) -> dict:
        """``engine.Ensemble.statistics`` over the members (mean, variance, extremes and who holds them, counts), plus
        ``probability`` = n_above / count in float64 -- the fraction of the entered values above ``threshold`` -- NaN where no value
        entered. ``want`` (default: every plane) always gains ``count`` and ``n_above``."""
        from .engine import ENS_STAT_ALL
        want = tuple(ENS_STAT_ALL if want is None else want)
        out = self._e.statistics(field, x, y, w, h, members=members, threshold=threshold, want=want + tuple(k for k in ("count", "n_above") if k not in want))
        n = out["count"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["probability"] = np.where(n > 0, out["n_above"].astype(np.float64) / n, np.nan)
        return out

    def quantiles(self, field: str, p, x: int = 0, y: int = 0, w: Optional[int] = None, h: Optional[int] = None, **kw) -> dict:
        """``engine.Ensemble.quantiles`` over the members: ``q`` (n_q, h, w, 4), ``count``, ``n_wall`` and, with ``rank_of``, ``n_below`` /
        ``n_equal`` (members, interp, rank_of, want)."""
        return self._e.quantiles(field, p, x, y, w, h, **kw)

    def median(self, field: str, x: int = 0, y: int = 0, w: Optional[int] = None, h: Optional[int] = None, **kw) -> np.ndarray:
        """The per-cell median over the members, (h, w, 4): ``quantiles(field, (0.5,))["q"][0]``."""
        return self.quantiles(field, (0.5,), x, y, w, h, **kw)["q"][0]

    def scores(self, field: str, truth, x: int = 0, y: int = 0, w: Optional[int] = None, h: Optional[int] = None, **kw) -> dict:
        """``engine.Ensemble.scores``: the members scored against ``truth`` -- a ``WeatherSim`` (a nature run, a member of this or
        another ensemble) or an ``engine.Handle`` -- on the device (members, want). On top of the exact sums, counts and rank histograms
        the derived numbers per channel in plain float64, NaN where nothing was scored: ``bias`` = sum_error / n_scored, ``mae``,
        ``rmse`` = sqrt(sum_sq_error / n_scored), ``spread`` = sqrt(sum_variance / n_scored), ``crps``, and ``rank_histogram`` =
        (rank_low + rank_high) / 2 -- tied cells split evenly between the two ends of their tie. The maps asked for with ``want``
        (error, variance, crps) come back under ``maps``."""
        from .engine import ENS_SCORE_MAPS
        out = self._e.scores(field, getattr(truth, "handle", truth), x, y, w, h, **kw)
        out["maps"] = {k: out.pop(k) for k in ENS_SCORE_MAPS if k in out}
        n = out["n_scored"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["bias"] = out["sum_error"] / n
            out["mae"] = out["sum_abs_error"] / n
            out["rmse"] = np.sqrt(out["sum_sq_error"] / n)
            out["spread"] = np.sqrt(out["sum_variance"] / n)
            out["crps"] = out["sum_crps"] / n
        out["rank_histogram"] = (out["rank_low"] + out["rank_high"]).astype(np.float64) / 2.0
        return out

    def neighbourhood(self, field: str, channel: int, threshold: float, scales, truth=None, *, wrap_x=None, **kw) -> dict:
        """``engine.Ensemble.neighbourhood``: neighbourhood ensemble probabilities of the event "channel of ``field`` above
        ``threshold``" at the ``scales`` ((rx, ry) half-widths in cells) and, against ``truth`` -- a ``WeatherSim`` or an
        ``engine.Handle`` --, the fractions skill score (Roberts and Lean 2008), on the device (above, rect, members, want). On top of
        the raw sums, in plain float64: ``fss`` = 1 - sum_d2 / (sum_f2 + sum_o2) per scale, NaN where the denominator is 0;
        ``base_rate`` = ev_o / n_o; ``frequency_bias`` = (ev_f / n_f) / base_rate; ``fss_useful`` = 0.5 + base_rate / 2, the FSS above
        which a forecast is useful at that scale. ``wrap_x`` defaults to the members' ``wrapHorizontally``. The maps asked for with
        ``want`` (nep, obs_fraction) come back under ``maps``."""
        from .engine import ENS_NBHD_MAPS
        if wrap_x is None:
            wrap_x = bool(self.members[0].gui.get("wrapHorizontally", True))
        out = self._e.neighbourhood(field, channel, threshold, scales, None if truth is None else getattr(truth, "handle", truth), wrap_x=wrap_x, **kw)
        out["maps"] = {k: out.pop(k) for k in ENS_NBHD_MAPS if k in out}
        with np.errstate(invalid="ignore", divide="ignore"):
            den = out["sum_f2"] + out["sum_o2"]
            out["fss"] = np.where(den > 0, 1.0 - out["sum_d2"] / den, np.nan)
            out["base_rate"] = np.float64(out["ev_o"]) / np.float64(out["n_o"])
            out["frequency_bias"] = (np.float64(out["ev_f"]) / np.float64(out["n_f"])) / out["base_rate"]
            out["fss_useful"] = 0.5 + out["base_rate"] / 2.0
        return out

    def fss(self, field: str, channel: int, threshold: float, scales, truth, **kw) -> list:
        """The fractions skill score of the members against ``truth`` at each of the ``scales``: ``neighbourhood(...)["fss"]`` as a list."""
        return [float(v) for v in self.neighbourhood(field, channel, threshold, scales, truth, want=(), **kw)["fss"]]

    @property
    def engine(self):
        return self._e

    def close(self):
        self._e.close()
