"""One engine's whole state and one substep of everything, composed from the restatements (imported like the other *_ref.py modules).

Mirror holds what an engine holds -- records, members, scalar channels with their coefficients, buoyancy and sources, bodies with their
dynamics records and volume bindings, tracers with their history ring, the fountain, the fp64 books as lists of terms -- and has one
method per public call that the random feature sequences draw.  It restates no arithmetic: substep() calls the oracle and the *_ref.py
modules in the order DESIGN.md and include/sph_abi.h give for one substep,

    grid of the entry state -> tracers -> scalar step (both on the entry state) -> SPH pass + container -> obstacles (volumes where bound)
    -> body step (kinematic advance, dynamic step) -> sources, then buoyancy, with the poses after the body step -> fountain,

and a paused substep does nothing at all.  A dynamic body's step takes the substep's impulse sums; the caller passes the device's own
(their last bit depends on the device's summation order) or lets the mirror use the restatement's correctly rounded ones.

sequence() is the seeded generator of the call sequences: it holds no engine and returns plain (op, args) tuples, so that the CPU tests
of the mirror and both GPU families replay the same calls.  apply() plays one tuple on a mirror, play() one on an engine.
"""
from __future__ import annotations

import ctypes as C
import math
import types

import numpy as np

from conftest import to_oracle_params
import body_ref as B
import body_scenes as S
import coupling_ref as CR
import obstacle_ref as R
import sample_ref
import scalar_ref as SR
import stats_ref
import surface_ref
import tracer_ref as TR
import volume_ref as VR
from support import fluid_block, random_scene

F = np.float32
STAGES = ("grid", "tracers", "scalars", "sph", "obstacles", "bodies", "couple", "fountain")
FEATURES = ("tracers", "scalars", "sources", "buoyancy", "kinematic", "dynamic", "volume", "fountain")


class Refused(Exception):
    """The call is one the engine refuses with SPH_ERR_STATE; nothing has changed."""


def order_bound(terms):
    """2 (n - 1) 2^-53 sum |t| of n fp64 terms: obstacle_ref.impulse_bound and coupling_ref.books_bound for terms collected over several
    substeps (any two summation trees of the same terms differ by no more)."""
    t = np.asarray(terms, np.float64)
    n = t.shape[0]
    return 2.0 * max(n - 1, 0) * 2.0 ** -53 * np.abs(t).sum(axis=0)


def _copy_params(sp):
    return type(sp).from_buffer_copy(sp)


class Mirror:
    ORDER = STAGES

    def __init__(self, pkg, oracle, rec, sp, seed=1):
        self.pkg, self.o = pkg, oracle
        self.rec = np.ascontiguousarray(rec).copy()
        self.sp = _copy_params(sp)
        self.op = to_oracle_params(oracle, self.sp)
        self.requested, self.seed = len(rec), seed
        fd = pkg.SphFountain()
        pkg.load_library().sph_fountain_default(C.byref(fd))
        self.of = oracle.default_fountain(mode=0, seed=int(fd.fountainSeed))
        self.grid_build = 0
        self.substeps = 0                                  # non-paused substeps since creation
        self._drop_scalars()
        self.bodies, self.dyn, self.dyn_raw, self.bind = [], [], [], []
        self.vols = {}
        self._zero_impulses()
        self._drop_tracers()

    # ---- members, options, records -------------------------------------------------------------------
    def set_member(self, name, value):
        cur = getattr(self.sp, name)
        if hasattr(cur, "__len__"):
            for i, x in enumerate(value):
                cur[i] = x
        else:
            setattr(self.sp, name, value)
        self.op = to_oracle_params(self.o, self.sp)

    def set_option(self, name, value):
        if name == "grid_build":
            self.grid_build = int(value)                   # (pass, record mode, graph replay and the sweep variant change no result)

    def upload(self, rec):
        self.rec = np.ascontiguousarray(rec).copy()        # (tracers, scalars, bodies: untouched; a value stays with its index)

    def reset(self):
        """sph_reset: a fresh spawn; tracers and scalars are dropped, the obstacle set stays and its sums restart."""
        self.rec, mass = self.o.spawn(self.op, self.requested, self.seed)
        self.set_member("param_mass", mass)
        self._drop_tracers()
        self._drop_scalars()
        self._zero_impulses()

    def wave(self, *a):
        self.rec = self.o.wave_impulse(self.rec, *a)

    def vortex(self, *a):
        self.rec = self.o.vortex_impulse(self.rec, self.op, *a)

    def set_fountain(self, on, offset=None, rate=None, level=None):
        self.of.mode = int(on)
        if on:
            self.of.drainPerSec, self.of.drainLevel = rate, level
            for a in range(3):
                self.of.offset[a] = offset[a]

    # ---- scalars ------------------------------------------------------------------------------------------
    def _drop_scalars(self):
        self.values, self.D, self.lam = None, None, None
        self.sc_steps, self.sc_number = 0, F(0)
        self.beta, self.ref = None, None
        self.sources = np.zeros(0, CR.SOURCE_DTYPE)
        self._zero_books()

    def _zero_books(self):
        self.src_terms = [[] for _ in range(len(self.sources))]
        self.src_time, self.src_steps = np.float64(0), 0

    @property
    def K(self):
        return 0 if self.values is None else self.values.shape[1]

    def set_scalars(self, values, diffusivity, decay):
        self._drop_scalars()                               # (a new set starts without buoyancy, without sources, with zeroed books)
        self.values = np.ascontiguousarray(values, F).reshape(len(self.rec), -1).copy()
        self.set_coefficients(diffusivity, decay)

    def clear_scalars(self):
        self._drop_scalars()

    def set_coefficients(self, diffusivity, decay):
        self.D = np.broadcast_to(np.asarray(diffusivity, F), (self.K,)).astype(F)
        self.lam = np.broadcast_to(np.asarray(decay, F), (self.K,)).astype(F)

    def paint(self, center, radius, value, channel, mode):
        self.values = SR.paint(self.rec, self.values, center, radius, channel, value, mode)

    def set_buoyancy(self, beta, ref):
        if beta is None:
            self.beta, self.ref = None, None
        else:
            self.beta = np.broadcast_to(np.asarray(beta, F), (self.K,)).astype(F)
            self.ref = np.broadcast_to(np.asarray(ref, F), (self.K,)).astype(F)

    def set_sources(self, sources):
        arr = np.ascontiguousarray(sources).view(CR.SOURCE_DTYPE).reshape(-1).copy()
        other = len(arr) != len(self.sources)
        self.sources = arr
        if other:                                          # (another count zeroes the books, the same count keeps them)
            self._zero_books()

    def injected(self, reset=False):
        """(sums, hits, time, substeps, bound) with the sums correctly rounded over every term since the last zeroing."""
        S_ = len(self.sources)
        sums, hits, bound = np.zeros(S_), np.zeros(S_, np.uint64), np.zeros(S_)
        for i, ts in enumerate(self.src_terms):
            t = np.concatenate(ts) if ts else np.zeros(0)
            sums[i], hits[i], bound[i] = math.fsum(t), len(t), order_bound(t)
        out = (sums, hits, float(self.src_time), self.src_steps, bound)
        if reset:
            self._zero_books()
        return out

    # ---- bodies, dynamics, volumes --------------------------------------------------------------------
    def _zero_impulses(self):
        self.imp_terms = [[] for _ in range(len(self.bodies))]
        self.imp_time, self.imp_steps = np.float64(0), 0

    def set_obstacles(self, arr):
        arr = np.asarray(arr, R.OBSTACLE_DTYPE).reshape(-1)
        other = len(arr) != len(self.bodies)
        self.bodies = R.bodies(arr, normalise=True)        # (a set replaces the set: dynamics records and bindings go with it)
        self.dyn = [None] * len(arr)
        self.dyn_raw = [None] * len(arr)
        self.bind = [None] * len(arr)
        if other:
            self._zero_impulses()

    def set_motion(self, index, vel, omega):
        self.bodies[index] = dict(self.bodies[index], v=np.asarray(vel, F), w=np.asarray(omega, F))

    def set_dynamics(self, index, record):
        self.dyn_raw[index] = None if record is None else np.frombuffer(bytes(record), B.DYNAMICS_DTYPE)[0].copy()
        self.dyn[index] = None if record is None else B.record(self.dyn_raw[index])

    def create_volume(self, handle, values, spacing):
        self.vols[handle] = VR.volume(values, spacing)

    def bind_volume(self, index, handle):
        self.bind[index] = handle

    def destroy_volume(self, handle):
        if handle in self.bind:
            raise Refused("the volume is bound")
        del self.vols[handle]

    def impulses(self, reset=False):
        """(J (K, 6) correctly rounded over every term since the last zeroing, time, substeps, bound (K, 6))."""
        Kb = len(self.bodies)
        J, bound = np.zeros((Kb, 6)), np.zeros((Kb, 6))
        for i, ts in enumerate(self.imp_terms):
            t = np.concatenate(ts) if ts else np.zeros((0, 6))
            J[i] = [math.fsum(t[:, a]) for a in range(6)]
            bound[i] = order_bound(t)
        out = (J, float(self.imp_time), self.imp_steps, bound)
        if reset:
            self._zero_impulses()
        return out

    def poses(self):
        return R.to_array(self.bodies)

    @property
    def any_dynamic(self):
        return any(d is not None for d in self.dyn)

    # ---- tracers ------------------------------------------------------------------------------------------
    def _drop_tracers(self):
        self.tr, self.tr_integrator, self.tr_K, self.tr_S, self.tr_steps, self.tr_ring = None, 0, 0, 1, 0, {}

    def set_tracers(self, points, integrator, history, stride):
        self._drop_tracers()
        if len(points):
            self.tr = TR.seed(points)
            self.tr_integrator, self.tr_K, self.tr_S = integrator, history, stride
            if history:
                self.tr_ring[TR.history_slot(0, history)] = TR.snapshot_of(self.tr)

    def clear_tracers(self):
        self._drop_tracers()

    def tracer_info(self):
        count, first = TR.history_stored(self.tr_steps, self.tr_S, self.tr_K) if self.tr is not None else (0, 0)
        return self.tr_steps if self.tr is not None else 0, count, first

    def tracer_history(self):
        _, count, first = self.tracer_info()
        return first, np.stack([self.tr_ring[TR.history_slot(q, self.tr_K)] for q in range(first, first + count)]) if count else None

    # ---- one substep --------------------------------------------------------------------------------------
    def refusal(self):
        """Why the next non-paused dispatch fails with SPH_ERR_STATE, or None."""
        if self.grid_build == 1 and self.tr is not None:
            return "tracers need the counting-sort grid build"
        if self.grid_build == 1 and self.values is not None:
            return "scalars need the counting-sort grid build"
        for s in self.sources:
            if int(s["body"]) >= len(self.bodies):
                return f"rides on obstacle {int(s['body'])}"
        return None

    def substep(self, dt=-1.0, impulses=None):
        """One DispatchCompute(dt).  impulses: the device's (K, 6) sums of this substep for the body step (None: the restatement's own)."""
        if self.sp.param_pause:
            return
        why = self.refusal()
        if why:
            raise Refused(why)
        c = types.SimpleNamespace(override=float(dt), dt=F(dt if dt > 0 else self.sp.param_timeStep), entry=self.rec, out=None, given=impulses,
                                  J=None, info=None, poses_before=self.bodies)
        for stage in self.ORDER:
            getattr(self, "stage_" + stage)(c)
        self.rec = c.out
        self.substeps += 1

    def _grid_of(self, rec):
        b = self.o.build_grid(rec, self.op)
        return b["grid"], b["cell_start"], b["order"]

    def stage_grid(self, c):
        c.grid = self._grid_of(c.entry)

    def stage_tracers(self, c, rec=None, grid=None):
        if self.tr is None:
            return
        self.tr = TR.advect(self.tr, c.entry if rec is None else rec, self.sp.param_h, self.sp.param_mass, *(c.grid if grid is None else grid), c.dt,
                            self.tr_integrator)
        self.tr_steps += 1
        slot = TR.history_write_slot(self.tr_steps, self.tr_S, self.tr_K)
        if slot is not None:
            self.tr_ring[slot] = TR.snapshot_of(self.tr)

    def stage_scalars(self, c, rec=None, grid=None):
        if self.values is None:
            return
        self.values, self.sc_number = SR.step32(c.entry if rec is None else rec, self.values, self.sp.param_h, self.sp.param_mass, self.D, self.lam, c.dt,
                                                *(c.grid if grid is None else grid))
        self.sc_steps += 1

    def stage_sph(self, c):
        c.out = self.o.obb(self.o.sph_pass(c.entry, self.op, dt=c.override), self.op)

    def stage_obstacles(self, c):
        if not self.bodies:
            return
        if any(h is not None for h in self.bind):
            names = sorted(self.vols)
            c.out, c.J, c.info = VR.apply(self.bodies, [self.vols[h] for h in names], [-1 if h is None else names.index(h) for h in self.bind],
                                          F(self.op.mass), c.out)
        else:
            c.out, c.J, c.info = R.apply(self.bodies, F(self.op.mass), c.out)
        for i, t in enumerate(c.info["terms"]):
            self.imp_terms[i].append(t)
        self.imp_time = self.imp_time + np.float64(c.dt)
        self.imp_steps += 1

    def stage_bodies(self, c):
        if not self.bodies:
            return
        J = c.J if c.given is None else np.asarray(c.given, np.float64).reshape(len(self.bodies), 6)
        self.bodies = B.step_all(self.bodies, self.dyn, J, S.world_of(self.pkg, self.sp), c.dt)

    def stage_couple(self, c, bodies=None):
        if self.values is None or (self.beta is None and not len(self.sources)):
            return
        g = (self.sp.param_gravityX, self.sp.param_gravityY, self.sp.param_gravityZ)
        c.out, self.values, books = CR.couple(c.out, self.values, c.dt, g, beta=self.beta, ref=self.ref, sources=self.sources,
                                              bodies=self.bodies if bodies is None else bodies)
        if len(self.sources):
            for i, t in enumerate(books["terms"]):
                self.src_terms[i].append(np.asarray(t, np.float64))
            self.src_time = self.src_time + np.float64(c.dt)
            self.src_steps += 1

    def stage_fountain(self, c):
        if self.of.mode:
            c.out = self.o.fountain_recycle(c.out, self.op, self.of, float(c.dt), int(self.of.seed))
            self.of.seed = (int(self.of.seed) + 1) & 0xFFFFFFFF

    # ---- read-only queries, from the restatements on the current state -----------------------------------
    def cells(self):
        b = self.o.build_grid(self.rec, self.op)
        return np.diff(b["cell_start"]).astype(np.int32), b["particle_cell"]

    def sample(self, points):
        """(density, fraction, count, velocity) of sph_sample_points."""
        grid = self._grid_of(self.rec)
        dens, frac, cnt = sample_ref.emulate(self.rec, points, self.sp.param_h, self.sp.param_mass, *grid)
        u, phi, _, _ = TR.field(self.rec, points, self.sp.param_h, self.sp.param_mass, *grid)
        return dens, frac, cnt, u, phi

    def sample_lattice(self, origin, spacing, dims, field="fraction"):
        pts = VR.lattice_points(origin, spacing, dims)
        dens, frac, _, _, _ = self.sample(pts)
        return (frac if field == "fraction" else dens).reshape(dims[2], dims[1], dims[0])

    def surface(self, origin, spacing, dims, iso):
        return surface_ref.extract(self.sample_lattice(origin, spacing, dims), origin, spacing, iso)

    def statistics(self, specs):
        _, pc = self.cells()
        return stats_ref.statistics(self.rec, self.sp, self.pkg.compute_grid_extents(self.sp), pc, specs)

    def scalar_moments(self):
        _, pc = self.cells()
        return SR.moments(self.values, SR.targets(self.rec), pc)

    def sample_scalar(self, points, channel):
        return SR.shepard32(self.rec, self.values, channel, points, self.sp.param_h, *self._grid_of(self.rec))

    # ---- the whole state, for comparisons between two mirrors -----------------------------------------------
    def state_bytes(self):
        parts = [self.rec.tobytes(), b"" if self.values is None else self.values.tobytes(), self.poses().tobytes(),
                 b"" if self.tr is None else self.tr.tobytes(), repr((self.tracer_info(), self.sc_steps, int(self.of.seed), self.K)).encode()]
        if self.tr is not None and self.tr_K:
            parts.append(self.tracer_history()[1].tobytes())
        parts.append(self.injected()[0].tobytes() + self.injected()[1].tobytes() + self.impulses()[0].tobytes())
        return b"|".join(parts)


# ---- the generator -----------------------------------------------------------------------------------------------
def feature_scene(pkg, seed):
    """A random_scene whose grid has at least 5 cells per axis, cut down to what the numpy restatements (whose cost is particles times
    candidates) step in a few seconds: at most 4096 records, 2048 from 2 and 1024 from 6 particles per cell on, and at most 64 records of
    a clump in one cell.  Crowded cells (occupancy 64), dense rows (the scalar sweep's staged rows overflow), ghosts, particles outside the
    grid and both instances of the walk stay.  Returns (records, params, what, centre, extent of the fluid inside the container)."""
    j = 0
    while True:
        rec, sp, _, what = random_scene(pkg, 2000 + 16 * seed + j)
        if min(what["dims"]) >= 5:
            break
        j += 1
    rec = rec[:4096 if what["per_cell"] < 2.0 else 2048 if what["per_cell"] < 6.0 else 1024]
    g = pkg.compute_grid_extents(sp)
    cx, cy, cz = sample_ref.cell_of(rec["pos"][:, :3], g)
    cell = (cz * g.dims[1] + cy) * g.dims[0] + cx
    rank = np.zeros(len(rec), np.int64)                    # the record's number among the records of its cell, in index order
    order = np.argsort(cell, kind="stable")
    start = np.r_[0, np.nonzero(np.diff(cell[order]))[0] + 1]
    rank[order] = np.arange(len(rec)) - np.repeat(start, np.diff(np.r_[start, len(rec)]))
    rec = rec[rank < 64].copy()
    half = np.array(list(sp.param_boxHalf), F)
    inside = (np.abs(rec["pos"][:, :3]) <= half * F(1.5)).all(axis=1) & (rec["isGhost"] == 0)
    c, E = fluid_block(rec[inside] if inside.any() else rec)
    what = dict(what, n=len(rec), scene_seed=2000 + 16 * seed + j, cells=int(g.numCells))
    return rec, sp, what, c, E


def _body(rng, c, E, shape=None):
    shape = int(rng.choice([R.SPHERE, R.BOX, R.BOX, R.CAPSULE])) if shape is None else shape
    size = [float(rng.uniform(0.08, 0.2) * E) for _ in range(3)]
    q = rng.normal(0, 1, 4)
    return dict(shape=shape, center=[float(c[a] + rng.uniform(-0.25, 0.25) * E) for a in range(3)], size=size, rotation=[float(x) for x in q / np.linalg.norm(q)],
                vel=[float(rng.uniform(-2, 2) * E) for _ in range(3)], omega=[float(rng.uniform(-6, 6)) for _ in range(3)],
                restitution=float(rng.uniform(0, 0.6)), friction=float(rng.uniform(0, 0.3)))


def _source(rng, c, E, K, nbodies):
    body = int(rng.integers(0, nbodies)) if nbodies and rng.random() < 0.5 else -1
    center = [float(rng.uniform(-0.05, 0.05) * E) for _ in range(3)] if body >= 0 else [float(c[a] + rng.uniform(-0.2, 0.2) * E) for a in range(3)]
    return dict(shape=int(rng.integers(0, 2)), center=center, size=[float(rng.uniform(0.2, 0.45) * E) for _ in range(3)], channel=int(rng.integers(0, K)),
                mode=int(rng.integers(0, 2)), rate=float(rng.choice([5.0, 60.0, 2000.0])), target=float(rng.uniform(-1, 3)), body=body)


def _tracer_points(rng, c, E, m, far):
    pts = np.zeros((m, 4), F)
    pts[:, :3] = c + rng.uniform(-0.45, 0.45, (m, 3)).astype(F) * F(E)
    pts[:, 3] = rng.uniform(0, 1, m).astype(F)
    pts[::7, 1] += F(3.0 * E)                              # dry ones, above the fluid
    if m > 2:
        pts[1, :3] = far                                   # outside the grid
        pts[2, 0] = np.nan
    return pts


def _probe_points(rng, c, E, m, far):
    pts = (c + rng.uniform(-0.6, 0.6, (m, 3)).astype(F) * F(E)).astype(F)
    pts[0] = far
    pts[1, 1] = np.nan
    return pts


SETUP = ("set_scalars", "set_obstacles", "set_tracers", "sources", "buoyancy", "dynamics", "volume", "fountain", "dispatch", "paint")
WISHES = ("refuse_destroy", "param:param_viscosity", "param:param_gravityY", "param:param_timeStep", "param:param_pause", "container:half",
          "container:euler", "container:shape", "option:neighbor", "option:aos", "option:graph", "option:sweep", "clear_tracers", "clear_scalars",
          "clear_obstacles", "reset", "coefficients", "injected", "impulses", "volume", "destroy", "wave", "vortex", "upload", "motion", "refuse_dangling",
          "refuse_grid_build", "dynamics", "sources", "paint", "sandwich:container", "sandwich:set_scalars", "sandwich:clear_obstacles", "sandwich:bind",
          "sandwich:first_sources", "sandwich:buoyancy", "sandwich:sources")
QUERIES = ("download", "scalars", "obstacles", "tracers", "tracer_history", "download_grid", "sample", "sample_lattice", "statistics",
           "scalar_moments", "sample_scalar", "surface", "mesh_distance")


def make_query(rng, name, c, E, far, K, rho0):
    if name in ("sample", "sample_scalar"):
        return dict(name=name, points=_probe_points(rng, c, E, 40, far), channel=int(rng.integers(0, max(K, 1))))
    if name in ("sample_lattice", "surface"):
        nn = 8 if name == "sample_lattice" else 14
        dims = tuple(int(rng.integers(nn - 3, nn + 1)) for _ in range(3))
        spacing = tuple(float(1.1 * E / d) for d in dims)
        return dict(name=name, origin=tuple(float(c[a] - 0.55 * E) for a in range(3)), spacing=spacing, dims=dims, iso=0.5)
    if name == "statistics":
        return dict(name=name, specs=[(stats_ref.DENSITY, 64, 0.0, 4.0 * rho0)])
    if name == "mesh_distance":
        r = float(rng.uniform(0.2, 0.4))
        return dict(name=name, radius=r, origin=(-0.5, -0.45, -0.55), spacing=float(rng.uniform(0.15, 0.2)), dims=(6, 7, 5))
    return dict(name=name)


def sequence(pkg, seed, family="A"):
    """(records, params, what, ops) of one random feature sequence.  ops is a list of (op, args) with args a dict of plain values.
    family "A": while a body is dynamic only single dispatches, each followed by ("impulses", reset); family "B": DispatchN and graph
    runs with dynamic bodies too, and no read-only queries (the busy run adds its own)."""
    rng = np.random.default_rng((4000 if family == "A" else 6000) + seed)
    rec, sp0, what, c, E = feature_scene(pkg, seed + (0 if family == "A" else 40))
    sp = _copy_params(sp0)
    h, rho0 = float(sp.param_h), float(sp.param_restDensity)
    far = (c + F(40.0 * E)).astype(F)
    ops = []
    st = types.SimpleNamespace(K=0, nsrc=0, buoy=False, bodies=[], dyn=set(), bound={}, vols=[], tracers=False, fountain=False, graph=0, pause=0,
                               reset=False, substeps=0, src_bodies=[], first_sources=True, nvol=0, queries=0, forced=None)

    def alive():
        a = set()
        if st.tracers: a.add("tracers")
        if st.K: a.add("scalars")
        if st.nsrc: a.add("sources")
        if st.buoy: a.add("buoyancy")
        if any(i not in st.dyn for i in range(len(st.bodies))): a.add("kinematic")
        if st.dyn: a.add("dynamic")
        if st.bound: a.add("volume")
        if st.fountain: a.add("fountain")
        return tuple(sorted(a))

    def emit(op, **args):
        ops.append((op, args))

    def dispatch(dt):
        emit("dispatch", dt=dt, alive=alive(), paused=st.pause)
        st.substeps += 1
        if st.dyn and family == "A":
            emit("impulses", reset=True)

    def dispatch_n(k, times=1):
        for _ in range(times):
            if st.dyn and family == "A":
                for _ in range(k):
                    dispatch(-1.0)
            else:
                emit("dispatch_n", k=k, alive=alive(), paused=st.pause, graph=st.graph and not st.fountain and not st.pause)
                st.substeps += k

    def set_scalars(K):
        emit("set_scalars", K=K, seed=int(rng.integers(0, 1 << 30)), diffusivity=[float(rng.uniform(50, 400) * h * h) for _ in range(K)],
             decay=[float(rng.choice([0.0, 2.0])) for _ in range(K)])
        st.K, st.nsrc, st.buoy, st.src_bodies, st.first_sources = K, 0, False, [], True

    def set_sources(count):
        srcs = [_source(rng, c, E, st.K, len(st.bodies)) for _ in range(count)]
        emit("sources", sources=srcs, first=st.first_sources and count > 0)
        if count:
            st.first_sources = False
        st.nsrc, st.src_bodies = count, [s["body"] for s in srcs]

    def set_obstacles(count, box=False):
        bodies = [_body(rng, c, E, R.BOX if i == 0 and (box or rng.random() < 0.7) else None) for i in range(count)]
        emit("set_obstacles", bodies=bodies)
        st.bodies, st.dyn, st.bound = [b["shape"] for b in bodies], set(), {}
        st.body_sizes = [b["size"] for b in bodies]

    def fix_dangling():
        if any(b >= len(st.bodies) for b in st.src_bodies):
            emit("dispatch_refused", dt=-1.0, match="obstacle")
            keep = [s for s in ops_sources() if s["body"] < len(st.bodies)]
            emit("sources", sources=keep, first=False)
            st.nsrc, st.src_bodies = len(keep), [s["body"] for s in keep]

    def ops_sources():
        for op, a in reversed(ops):
            if op == "sources":
                return a["sources"]
        return []

    def create_volume():
        boxes = [i for i, s in enumerate(st.bodies) if s == R.BOX]
        i = int(rng.choice(boxes))
        m = min(st.body_sizes[i])
        handle = f"v{st.nvol}"
        st.nvol += 1
        kind = str(rng.choice(["sphere", "box"]))
        emit("create_volume", handle=handle, kind=kind, radius=0.9 * m, half=[0.8 * m, 0.6 * m, 0.7 * m], spacing=m / 3.0)
        st.vols.append(handle)
        return i, handle

    def quiet_for_graphs():
        if st.fountain:
            emit("fountain", on=0); st.fountain = False
        if st.pause:
            emit("param", name="param_pause", value=0); st.pause = 0
        if not st.graph:
            emit("option", name="graph", value=1); st.graph = 1

    def pick(kind, choices):
        """One of the choices, the wished one if a wish names it."""
        if st.forced in choices:
            return st.forced
        return str(rng.choice(choices))

    def edit_container():
        which = pick("container", ["half", "euler", "shape"])
        if which == "half":
            value = tuple(float(x) * float(rng.uniform(0.9, 1.15)) for x in sp.param_boxHalf)
            name = "param_boxHalf"
        elif which == "euler":
            value, name = tuple(float(rng.uniform(-30, 30)) for _ in range(3)), "param_boxEulerDeg"
        else:
            value, name = int(rng.integers(0, 15)), "param_shapeType"
        emit("container", name=name, value=value)
        cur = getattr(sp, name)
        if hasattr(cur, "__len__"):
            for a in range(3):
                cur[a] = value[a]
        else:
            setattr(sp, name, value)

    def between_runs(what_):
        """One key-changing call between two graph runs."""
        if what_ == "container":
            edit_container()
        elif what_ == "set_scalars":
            set_scalars(int(rng.choice([k for k in (1, 2, 4) if k != st.K])))
        elif what_ == "clear_obstacles":
            emit("clear_obstacles"); st.bodies, st.dyn, st.bound = [], set(), {}
            fix_dangling()
        elif what_ == "bind":
            if st.bound:
                i = next(iter(st.bound))
                emit("unbind", index=i); del st.bound[i]
            else:
                i, handle = create_volume()
                emit("bind", index=i, handle=handle); st.bound[i] = handle
        elif what_ == "first_sources":
            set_sources(int(rng.integers(1, 5)))
        elif what_ == "sources":                           # (on or off with the buffers in place: only which kernels run changes)
            set_sources(0 if st.nsrc else int(rng.integers(1, 5)))
        elif what_ == "buoyancy":
            if st.buoy:
                emit("buoyancy", beta=None, ref=None); st.buoy = False
            else:
                ensure("buoyancy")

    def sandwich():
        k = 2
        if st.substeps + 6 * k > 30:
            return False
        if st.forced:
            for need in {"set_scalars": ["scalars"], "clear_obstacles": ["kinematic"], "bind": ["box"], "first_sources": ["scalars"], "buoyancy": ["scalars"],
                         "sources": ["scalars"]}.get(st.forced, []):
                ensure(need)
            if st.forced == "first_sources" and not st.first_sources:
                set_scalars(int(rng.choice([k for k in (1, 2, 4) if k != st.K])))
        options = ["container"]
        if st.K:
            options += ["set_scalars", "buoyancy", "sources"]
            if st.first_sources:
                options = ["first_sources"]
        if st.bodies:
            options.append("clear_obstacles")
        if R.BOX in st.bodies:
            options += ["bind", "bind"]
        quiet_for_graphs()
        dispatch_n(k, 3)
        between_runs(pick("between", options))
        dispatch_n(k, 3)
        return True

    def ensure(feature):
        """Makes a feature alive, if it is not, with the calls a host would make."""
        if feature in ("scalars", "sources", "buoyancy") and not st.K:
            set_scalars(int(rng.choice([1, 2, 4])))
        if feature == "sources" and not st.nsrc:
            set_sources(int(rng.integers(1, 5)))
        if feature == "buoyancy" and not st.buoy:
            emit("buoyancy", beta=[float(rng.uniform(0.2, 0.8)) for _ in range(st.K)], ref=[float(rng.uniform(0, 0.5)) for _ in range(st.K)]); st.buoy = True
        if feature == "tracers" and not st.tracers:
            set_tracers()
        if feature in ("kinematic", "dynamic", "volume", "box") and (not st.bodies or (feature in ("volume", "box") and R.BOX not in st.bodies)):
            set_obstacles(int(rng.integers(2, 4)), box=True)
            fix_dangling()
        if feature == "kinematic" and len(st.dyn) == len(st.bodies):
            i = next(iter(st.dyn))
            emit("dynamics", index=i, on=0); st.dyn.discard(i)
        if feature == "dynamic" and not st.dyn:
            set_dynamic(int(rng.integers(0, len(st.bodies))))
        if feature == "volume" and not st.bound:
            i, handle = create_volume()
            emit("bind", index=i, handle=handle); st.bound[i] = handle
        if feature == "fountain" and not st.fountain:
            fountain_on()
        if feature == "unpaused" and st.pause:
            emit("param", name="param_pause", value=0); st.pause = 0

    def set_dynamic(i):
        if family == "A":
            emit("impulses", reset=True)                   # (the sums of a dynamic body's substep are read one dispatch at a time)
        emit("dynamics", index=i, on=1, density=float(rng.choice([0.3, 0.8, 2.5])), shape=st.bodies[i], size=st.body_sizes[i]); st.dyn.add(i)

    def set_tracers():
        m = int(rng.choice([1, 63, 64, 65, 200]))
        emit("set_tracers", points=_tracer_points(rng, c, E, m, far), integrator=int(rng.integers(0, 2)), history=int(rng.choice([0, 3])), stride=int(rng.choice([1, 2])))
        st.tracers = True

    def fountain_on():
        emit("fountain", on=1, offset=(float(rng.uniform(-h, h)), float(rng.uniform(-6 * h, 0.0)), float(rng.uniform(-h, h))),
             rate=float(rng.uniform(50, 600)), level=float(rng.uniform(0.5 * h, 6 * h)))
        st.fountain = True

    NEEDS = {"refuse_destroy": ["volume"], "clear_tracers": ["tracers"], "clear_scalars": ["scalars"], "clear_obstacles": ["kinematic"], "coefficients": ["scalars"],
             "injected": ["sources"], "impulses": ["kinematic"], "volume": ["box"], "motion": ["kinematic"], "refuse_dangling": ["scalars", "kinematic", "unpaused"],
             "refuse_grid_build": ["scalars", "unpaused"], "dynamics": ["kinematic"], "sources": ["scalars"], "destroy": ["volume"], "paint": ["scalars"],
             "query:scalars": ["scalars"], "query:scalar_moments": ["scalars"], "query:sample_scalar": ["scalars"], "query:tracers": ["tracers"],
             "query:tracer_history": ["tracers"], "query:obstacles": ["kinematic"]}
    n_ops = int(rng.integers(14, 23))
    drawn = 0
    # features come alive early, so that the later calls meet them together
    menu = ["dispatch"] * 12 + ["dispatch_n"] * 4 + ["sandwich"] * 2 + ["wave", "vortex", "param", "param", "container", "option", "option", "upload", "fountain",
            "reset", "set_scalars", "set_scalars", "clear_scalars", "coefficients", "paint", "paint", "buoyancy", "buoyancy", "sources", "sources", "sources", "injected",
            "set_obstacles", "set_obstacles", "clear_obstacles", "motion", "dynamics", "dynamics", "volume", "volume", "impulses", "set_tracers", "set_tracers",
            "clear_tracers", "refuse_grid_build", "refuse_dangling", "refuse_destroy"] + (["query"] * 16 if family == "A" else [])
    setup = [x for x in SETUP if x != "sources" or seed % 4 != 1]        # (some seeds meet their first sources between two graph runs)
    # every sequence is given a pair of features to have alive in one substep and four calls by turns, so that the seeds together reach
    # the whole alphabet and every pair whatever the dice say
    turn = seed if family == "A" else 16 + seed
    pair = [(x, y) for i, x in enumerate(FEATURES) for y in FEATURES[i + 1:]][turn % 28]
    if family == "A":
        wishes = ["query:" + QUERIES[(2 * seed + j) % len(QUERIES)] for j in range(2)] + [WISHES[(2 * seed + j) % len(WISHES)] for j in range(2)]
    else:
        wishes = [WISHES[(4 * seed + j + 2) % len(WISHES)] for j in range(4)]
    wishes = ["pair"] + wishes
    guard = 0
    while drawn < n_ops and guard < 400:
        guard += 1
        opn, st.forced, wished = str(rng.choice(setup if drawn < 5 else menu)), None, False
        if drawn >= 3 and wishes and rng.random() < 0.5:
            for need in NEEDS.get(wishes[0], []):
                ensure(need)
            opn, _, st.forced = wishes[0].partition(":")
            wished = True
            wishes.append(wishes.pop(0))                   # (a wish that the state does not allow yet comes round again)
        before = len(ops)
        if opn == "pair":
            if st.substeps + 1 > 30: continue
            for need in pair + ("unpaused",):
                ensure(need)
            for need in pair:                              # (making one alive may have replaced the other's set)
                ensure(need)
            dispatch(-1.0)
        elif opn == "destroy":
            i = next(iter(st.bound))
            emit("unbind", index=i); handle = st.bound.pop(i)
            emit("destroy_volume", handle=handle); st.vols.remove(handle)
            opn = "done"
        if opn in ("pair", "done"):
            pass
        elif opn == "dispatch":
            if st.substeps + 1 > 30: continue
            dispatch(float(rng.choice([-1.0, -1.0, 5e-4, 1.5e-3])))
        elif opn == "dispatch_n":
            k = int(rng.integers(2, 5))
            times = int(rng.integers(3, 5)) if rng.random() < 0.3 else 1
            if st.substeps + k * times > 30: continue
            if times > 1:
                quiet_for_graphs()
            dispatch_n(k, times)
        elif opn == "sandwich":
            if not sandwich(): continue
        elif opn == "wave":
            emit("wave", args=(float(rng.uniform(0.2, 2.0) * h / 0.28), float(rng.uniform(1.0, 4.0)), float(rng.uniform(0, 6.0)), (0.3, 1.0, -0.2), -1e9, 1e9))
        elif opn == "vortex":
            emit("vortex", args=(float(rng.uniform(-1, 1) * h / 0.28), float(rng.uniform(-0.3, 0.3) * h / 0.28)))
        elif opn == "param":
            which = pick("param", ["param_viscosity", "param_gravityY", "param_timeStep", "param_pause"])
            if which == "param_pause":
                st.pause = 1 - st.pause
                value = st.pause
            else:
                value = {"param_viscosity": float(rng.uniform(1, 8)), "param_gravityY": float(rng.uniform(-1500, 200) * h / 0.28),
                         "param_timeStep": float(rng.choice([5e-4, 1e-3, 2e-3]))}[which]
            emit("param", name=which, value=value)
        elif opn == "container":
            edit_container()
        elif opn == "option":
            which = pick("option", ["neighbor", "aos", "graph", "sweep"])
            value = int(rng.choice([1, 2, 3, 3, 3])) if which == "neighbor" else int(rng.integers(0, 2))
            if which == "graph":
                st.graph = value
            emit("option", name=which, value=value)
        elif opn == "upload":
            emit("upload", seed=int(rng.integers(0, 1 << 30)))
        elif opn == "fountain":
            if st.fountain and rng.random() < 0.4:
                emit("fountain", on=0); st.fountain = False
            else:
                fountain_on()
        elif opn == "reset":
            if st.reset or drawn < 6: continue
            emit("reset"); st.reset = True
            st.K, st.nsrc, st.buoy, st.src_bodies, st.tracers = 0, 0, False, [], False
        elif opn == "set_scalars":
            if st.K and rng.random() < 0.6: continue
            set_scalars(int(rng.choice([1, 2, 4])))
        elif opn == "clear_scalars":
            if not st.K or rng.random() < 0.3: continue
            emit("clear_scalars"); st.K, st.nsrc, st.buoy, st.src_bodies = 0, 0, False, []
        elif opn == "coefficients":
            if not st.K: continue
            emit("coefficients", diffusivity=[float(rng.uniform(50, 400) * h * h) for _ in range(st.K)], decay=[float(rng.choice([0.0, 5.0])) for _ in range(st.K)])
        elif opn == "paint":
            if not st.K: continue
            emit("paint", center=[float(c[a] + rng.uniform(-0.3, 0.3) * E) for a in range(3)], radius=float(rng.uniform(0.15, 0.4) * E),
                 value=float(rng.uniform(-2, 4)), channel=int(rng.integers(0, st.K)), mode=int(rng.integers(0, 2)))
        elif opn == "buoyancy":
            if not st.K: continue
            if st.buoy and rng.random() < 0.3:
                zero = rng.random() < 0.5
                emit("buoyancy", beta=[0.0] * st.K if zero else None, ref=[1.0] * st.K if zero else None); st.buoy = False
            else:
                emit("buoyancy", beta=[float(rng.uniform(-0.8, 0.8)) for _ in range(st.K)], ref=[float(rng.uniform(0, 0.5)) for _ in range(st.K)]); st.buoy = True
        elif opn == "sources":
            if not st.K: continue
            set_sources(int(rng.integers(0, 5)) if st.nsrc else int(rng.integers(1, 5)))
        elif opn == "injected":
            if not st.K: continue
            emit("injected", reset=bool(rng.random() < 0.5))
        elif opn == "set_obstacles":
            if st.bodies and rng.random() < 0.6: continue
            set_obstacles(int(rng.integers(1, 4)))
            fix_dangling()
        elif opn == "clear_obstacles":
            if not st.bodies or rng.random() < 0.3: continue
            emit("clear_obstacles"); st.bodies, st.dyn, st.bound = [], set(), {}
            fix_dangling()
        elif opn == "motion":
            if not st.bodies: continue
            emit("motion", index=int(rng.integers(0, len(st.bodies))), vel=[float(rng.uniform(-2, 2) * E) for _ in range(3)], omega=[float(rng.uniform(-6, 6)) for _ in range(3)])
        elif opn == "dynamics":
            if not st.bodies: continue
            i = int(rng.integers(0, len(st.bodies)))
            if i in st.dyn:
                if rng.random() < 0.6: continue
                emit("dynamics", index=i, on=0); st.dyn.discard(i)
            else:
                set_dynamic(i)
        elif opn == "volume":
            if st.bound and rng.random() < 0.5:
                i = next(iter(st.bound))
                emit("unbind", index=i); handle = st.bound.pop(i)
                if rng.random() < 0.5:
                    emit("destroy_volume", handle=handle); st.vols.remove(handle)
            elif R.BOX in st.bodies and len(st.vols) < 4:
                i, handle = create_volume()
                emit("bind", index=i, handle=handle); st.bound[i] = handle
            else:
                continue
        elif opn == "impulses":
            if not st.bodies: continue
            emit("impulses", reset=bool(rng.random() < 0.5) or (bool(st.dyn) and family == "A"))
        elif opn == "set_tracers":
            if st.tracers and rng.random() < 0.6: continue
            set_tracers()
        elif opn == "clear_tracers":
            if not st.tracers or rng.random() < 0.3: continue
            emit("clear_tracers"); st.tracers = False
        elif opn == "refuse_grid_build":
            if not (st.tracers or st.K) or st.pause: continue
            emit("option", name="grid_build", value=1)
            emit("dispatch_refused", dt=-1.0, match="counting-sort")
            emit("option", name="grid_build", value=0)
        elif opn == "refuse_dangling":
            if len(st.bodies) < 1 or not st.K or st.pause: continue
            count = int(rng.integers(1, 4))
            srcs = [_source(rng, c, E, st.K, len(st.bodies)) for _ in range(count)]
            srcs[0]["body"], srcs[0]["center"] = len(st.bodies) - 1, [0.0, 0.0, 0.0]
            emit("sources", sources=srcs, first=st.first_sources)
            st.first_sources = False
            st.nsrc, st.src_bodies = count, [s["body"] for s in srcs]
            if len(st.bodies) > 1 and rng.random() < 0.5:
                set_obstacles(len(st.bodies) - 1)
            else:
                emit("clear_obstacles"); st.bodies, st.dyn, st.bound = [], set(), {}
            fix_dangling()
        elif opn == "refuse_destroy":
            if not st.bound: continue
            emit("destroy_refused", handle=next(iter(st.bound.values())))
        elif opn == "query":
            pool = [q for q in QUERIES if not ((q in ("scalars", "scalar_moments", "sample_scalar") and not st.K) or
                                               (q in ("tracers", "tracer_history") and not st.tracers) or (q == "obstacles" and not st.bodies))]
            pool += [q for q in pool if q in ("scalars", "scalar_moments", "sample_scalar", "tracers", "tracer_history", "obstacles")]
            name = str(rng.choice(pool))                   # (the queries of a feature that is set come up twice as often)
            if st.forced:
                if st.forced not in pool: continue
                name = st.forced
            emit("query", **make_query(rng, name, c, E, far, st.K, rho0))
        if len(ops) > before:
            drawn += 1
            if wished:
                wishes.pop()
    what = dict(what, family=family, substeps=st.substeps, center=[float(x) for x in c], extent=float(E))
    return rec, sp0, what, ops


def log_line(op, a):
    keys = ("dt", "k", "name", "value", "K", "index", "handle", "reset", "on", "match", "integrator", "history", "stride")
    return op + "".join(f" {k}={a[k]}" for k in keys if k in a and not isinstance(a[k], (list, np.ndarray)))


# ---- argument builders shared by both sides -------------------------------------------------------------------
def scalar_values(n, K, seed):
    return np.random.default_rng(seed).uniform(-1.0, 2.0, (n, K)).astype(F)


def edited_records(rec, seed):
    """What a host does between a download and an upload: kicks, new ghosts, switched-off records."""
    rng = np.random.default_rng(seed)
    cur = rec.copy()
    pick = rng.choice(len(cur), size=max(1, len(cur) // 10), replace=False)
    cur["vel"][pick, :3] += rng.normal(0, 5, (len(pick), 3)).astype(F)
    cur["isGhost"][pick[: len(pick) // 4]] = 1
    cur["isActive"][pick[: len(pick) // 8]] = 0
    return cur


def obstacle_records(pkg, bodies):
    return pkg.obstacle_array([pkg.obstacle(b["shape"], b["center"], b["size"], rotation=b["rotation"], vel=b["vel"], omega=b["omega"],
                                            restitution=b["restitution"], friction=b["friction"]) for b in bodies])


def source_records(pkg, sources):
    return pkg.source_array([pkg.scalar_source(s["shape"], s["center"], s["size"], channel=s["channel"], mode=s["mode"], rate=s["rate"], target=s["target"],
                                               body=s["body"]) for s in sources])


def dynamics_record(pkg, a, rho0):
    make = {R.SPHERE: pkg.dynamics_sphere, R.BOX: pkg.dynamics_box, R.CAPSULE: pkg.dynamics_capsule}[a["shape"]]
    size = a["size"][0] if a["shape"] == R.SPHERE else a["size"]
    return make(a["density"] * rho0, size)


def lattice(a):
    if a["kind"] == "sphere":
        return VR.sphere_lattice(a["radius"], a["spacing"]), a["spacing"]
    return VR.box_lattice(a["half"], a["spacing"]), a["spacing"]


def apply(m, op, a, impulses=None):
    """One (op, args) of a sequence on a Mirror (a query changes nothing)."""
    pkg = m.pkg
    if op == "dispatch":
        m.substep(a["dt"], impulses)
    elif op == "dispatch_n":
        for _ in range(a["k"]):
            m.substep(-1.0)
    elif op == "dispatch_refused":
        try:
            m.substep(a["dt"])
        except Refused as why:
            assert a["match"] in str(why), (a, str(why))
        else:
            raise AssertionError(f"the mirror does not refuse {a}")
    elif op == "wave": m.wave(*a["args"])
    elif op == "vortex": m.vortex(*a["args"])
    elif op in ("param", "container"): m.set_member(a["name"], a["value"])
    elif op == "option": m.set_option(a["name"], a["value"])
    elif op == "upload": m.upload(edited_records(m.rec, a["seed"]))
    elif op == "fountain": m.set_fountain(a["on"], a.get("offset"), a.get("rate"), a.get("level"))
    elif op == "reset": m.reset()
    elif op == "set_scalars": m.set_scalars(scalar_values(len(m.rec), a["K"], a["seed"]), a["diffusivity"], a["decay"])
    elif op == "clear_scalars": m.clear_scalars()
    elif op == "coefficients": m.set_coefficients(a["diffusivity"], a["decay"])
    elif op == "paint": m.paint(a["center"], a["radius"], a["value"], a["channel"], a["mode"])
    elif op == "buoyancy": m.set_buoyancy(a["beta"], a["ref"])
    elif op == "sources": m.set_sources(source_records(pkg, a["sources"]))
    elif op == "injected": m.injected(a["reset"])
    elif op == "set_obstacles": m.set_obstacles(obstacle_records(pkg, a["bodies"]))
    elif op == "clear_obstacles": m.set_obstacles(np.zeros(0, R.OBSTACLE_DTYPE))
    elif op == "motion": m.set_motion(a["index"], a["vel"], a["omega"])
    elif op == "dynamics": m.set_dynamics(a["index"], dynamics_record(pkg, a, float(m.sp.param_restDensity)) if a["on"] else None)
    elif op == "create_volume": m.create_volume(a["handle"], *lattice(a))
    elif op == "bind": m.bind_volume(a["index"], a["handle"])
    elif op == "unbind": m.bind_volume(a["index"], None)
    elif op == "destroy_volume": m.destroy_volume(a["handle"])
    elif op == "destroy_refused":
        try:
            m.destroy_volume(a["handle"])
        except Refused:
            pass
        else:
            raise AssertionError("the mirror does not refuse to destroy a bound volume")
    elif op == "impulses": m.impulses(a["reset"])
    elif op == "set_tracers": m.set_tracers(a["points"], a["integrator"], a["history"], a["stride"])
    elif op == "clear_tracers": m.clear_tracers()
    elif op == "query": pass
    else:
        raise KeyError(op)


OPTIONS = dict(neighbor="SPH_OPT_NEIGHBOR_KERNEL", aos="SPH_OPT_AOS_MODE", graph="SPH_OPT_GRAPH", sweep="SPH_OPT_SCALAR_SWEEP", grid_build="SPH_OPT_GRID_BUILD")


def play(f, pkg, op, a, handles, split_n=False, flip_aos=False, force_graph=None):
    """The same (op, args) on an engine.  handles: the volume ids of this engine by the sequence's handle.  split_n issues a DispatchN(k) as
    k single calls, flip_aos sets the opposite record mode, force_graph overrides every graph switch (the two ways of family B)."""
    import pytest
    if op == "dispatch": f.DispatchCompute(a["dt"])
    elif op == "dispatch_n":
        if split_n:
            for _ in range(a["k"]):
                f.DispatchCompute()
        else:
            f.DispatchN(a["k"])
    elif op == "dispatch_refused":
        with pytest.raises(pkg.SphError, match="error -3:.*" + a["match"]):
            f.DispatchCompute(a["dt"])
        with pytest.raises(pkg.SphError, match="error -3:.*" + a["match"]):
            f.DispatchN(2)
    elif op == "wave": f.ApplyWaveImpulse(*a["args"])
    elif op == "vortex": f.ApplyVortexImpulse(*a["args"])
    elif op in ("param", "container"): setattr(f, a["name"], a["value"])
    elif op == "option":
        value = a["value"]
        if a["name"] == "aos" and flip_aos: value = 1 - value
        if a["name"] == "graph" and force_graph is not None: value = force_graph
        f.set_option(getattr(pkg, OPTIONS[a["name"]]), value)
    elif op == "upload": f.upload(edited_records(f.download(), a["seed"]))
    elif op == "fountain":
        f.fountainMode = a["on"]
        if a["on"]:
            f.fountainOffset, f.fountainDrainPerSec, f.fountainDrainLevel = a["offset"], a["rate"], a["level"]
    elif op == "reset": f.ResetSimulation()
    elif op == "set_scalars": f.set_scalars(scalar_values(f.GetNumFluids(), a["K"], a["seed"]), diffusivity=a["diffusivity"], decay=a["decay"])
    elif op == "clear_scalars": f.clear_scalars()
    elif op == "coefficients": f.set_scalar_coefficients(a["diffusivity"], a["decay"])
    elif op == "paint": f.paint_scalar(a["center"], a["radius"], a["value"], channel=a["channel"], mode=a["mode"])
    elif op == "buoyancy": f.set_scalar_buoyancy(a["beta"], a["ref"] if a["ref"] is not None else 0.0)
    elif op == "sources": f.set_scalar_sources(source_records(pkg, a["sources"]))
    elif op == "injected": return f.scalar_injected(a["reset"])
    elif op == "set_obstacles": f.set_obstacles(obstacle_records(pkg, a["bodies"]))
    elif op == "clear_obstacles": f.clear_obstacles()
    elif op == "motion": f.set_obstacle_motion(a["index"], a["vel"], a["omega"])
    elif op == "dynamics": f.set_obstacle_dynamics(a["index"], dynamics_record(pkg, a, float(f.param_restDensity)) if a["on"] else None)
    elif op == "create_volume": handles[a["handle"]] = f.create_volume(*lattice(a))
    elif op == "bind": f.bind_obstacle_volume(a["index"], handles[a["handle"]])
    elif op == "unbind": f.bind_obstacle_volume(a["index"], -1)
    elif op == "destroy_volume": f.destroy_volume(handles.pop(a["handle"]))
    elif op == "destroy_refused":
        with pytest.raises(pkg.SphError, match="error -3:"):
            f.destroy_volume(handles[a["handle"]])
    elif op == "impulses": return f.obstacle_impulses(a["reset"])
    elif op == "set_tracers": f.set_tracers(a["points"], a["integrator"], a["history"], a["stride"])
    elif op == "clear_tracers": f.clear_tracers()
    elif op == "query": pass
    else:
        raise KeyError(op)
    return None
