"""Helpers shared by the test modules (imported like the *_ref.py modules): building and running the C++ examples, the C99 layout
program behind the ctypes mirrors, the bitwise and impulse comparisons, the engine set-ups several GPU test files use, and what the
GPU tests of every spatial query repeat (same_info, after_dispatches, the two refusing engines)."""
import os
import subprocess
from contextlib import contextmanager
from importlib import import_module

import numpy as np

from conftest import PKG_NAME, ROOT, small_scene
import obstacle_ref as R

F = np.float32
INCLUDE = os.path.join(ROOT, "include")
LIB_DIR = os.path.join(ROOT, PKG_NAME)                                   # where build() leaves libsph_hip.so
G = os.path.join(ROOT, "tests", "golden")


# ---- C and C++ against include/ ---------------------------------------------------------------------
def build_example(pkg, name, out_dir, werror=False):
    """Compile examples/<name>.cpp against libsph_hip.so into out_dir; returns the executable's path."""
    pkg.load_library()
    exe = os.path.join(str(out_dir), name)
    cmd = ["g++", "-std=c++17", "-Wall", *(["-Werror"] if werror else []), "-I", INCLUDE, os.path.join(ROOT, "examples", name + ".cpp"),
           "-L", LIB_DIR, "-lsph_hip", "-Wl,-rpath," + LIB_DIR, "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0 or not os.path.exists(exe):
        raise RuntimeError(f"{' '.join(cmd)} failed ({res.returncode}):\n{res.stderr}")
    return exe


def run_example(exe, args, timeout):
    """Run a built example with the library's folder on LD_LIBRARY_PATH; prints what it wrote and returns the completed process."""
    env = dict(os.environ, LD_LIBRARY_PATH=LIB_DIR + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    res = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, env=env, timeout=timeout)
    print(res.stdout, res.stderr)
    return res


def check_shim_syntax(source=None):
    """g++ -fsyntax-only over include/SPHFluidGPU_hip.hpp, or over a source file that includes it."""
    what = ["-x", "c++", os.path.join(INCLUDE, "SPHFluidGPU_hip.hpp")] if source is None else [str(source)]
    res = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", INCLUDE, *what], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def c_layout(record_name, ctypes_struct, extra_printf_lines, tmp_path):
    """Print sizeof and every offsetof of a record of include/sph_abi.h from C99, followed by the caller's own printf statements.
    Returns (sizeof, [(field, offset), ...] in the order of the mirror's _fields_, the extra output lines)."""
    fields = [fname for fname, _ in ctypes_struct._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sph_abi.h"', 'int main(void) {',
             f'    printf("sizeof %zu\\n", sizeof({record_name}));']
    lines += [f'    printf("{fname} %zu\\n", offsetof({record_name}, {fname}));' for fname in fields]
    lines += ["    " + ln for ln in extra_printf_lines]
    lines += ['    return 0;', '}']
    src = tmp_path / f"layout_{record_name}.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / f"layout_{record_name}")
    res = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", INCLUDE, str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    head, size = out[0].split()
    assert head == "sizeof", out[0]
    offsets = [(name, int(val)) for name, val in (ln.split() for ln in out[1:1 + len(fields)])]
    return int(size), offsets, out[1 + len(fields):]


# ---- comparisons ------------------------------------------------------------------------------------
def same_bits(a, b, what):
    assert a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"{what}:\n{a}\nvs\n{b}"


def check_impulses(got, want, info, what):
    """Impulses against the restatement's correctly rounded sums, within obstacle_ref.impulse_bound (a re-ordered fp64 sum)."""
    bound = R.impulse_bound(info)
    err = np.abs(got - want)
    print(f"{what}: touched {info['touched'].tolist()} u_n<0 {info['negative'].tolist()} max err {err.max():.3g} max bound {bound.max():.3g}")
    assert (err <= bound).all(), f"{what}: |got - reference| {err} above {bound}"


# ---- engines and scenes -----------------------------------------------------------------------------
def engine(pkg, rec, sp, kern=3, aos=1, graph=0):
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.set_option(pkg.SPH_OPT_NEIGHBOR_KERNEL, kern)
    f.set_option(pkg.SPH_OPT_AOS_MODE, aos)
    f.set_option(pkg.SPH_OPT_GRAPH, graph)
    return f


def records(pkg, pos, vel, ghost=None):
    """Particle records at rest density from positions, velocities and an optional ghost mask."""
    rec = np.zeros(len(pos), pkg.PARTICLE_DTYPE)
    rec["pos"][:, :3] = pos
    rec["pos"][:, 3] = 1.0
    rec["vel"][:, :3] = vel
    rec["density"] = 1000.0
    if ghost is not None:
        rec["isGhost"] = ghost
    return rec


def fluid_block(rec):
    """Centre and largest extent of the fluid block."""
    p = rec["pos"][rec["isGhost"] == 0][:, :3].astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    return (0.5 * (lo + hi)).astype(F), float((hi - lo).max())


def random_scene(pkg, seed):
    """A seeded random scene for the fuzz tests: (records, params, substeps, what).  It varies the kernel length h (h^2 > 1 selects the
    walk's other template instance), non-cubic grids down to three cells, 0.3 .. 20 particles per cell, speeds up to the velocity cap,
    clumps, ghosts, particles outside the grid, rotated containers of every shape and the time step."""
    rng = np.random.default_rng(1000 + seed)
    h = float(rng.choice([0.1, 0.28, 0.28, 0.6, 1.25, 2.0]))
    dims = [int(rng.integers(3, 22)) for _ in range(3)]
    half = [(g / 2.0 - 1.0) * h - 0.01 * h for g in dims]
    lam = float(rng.choice([0.3, 1.0, 2.0, 2.0, 6.0, 20.0]))
    fill = float(rng.uniform(0.3, 1.0))                       # fraction of the box height that holds particles
    cells = max(1, (dims[0] - 2) * (dims[2] - 2) * max(1, int((dims[1] - 2) * fill)))
    n = int(min(14000, max(1, lam * cells)))
    dt = float(rng.choice([1e-3, 5e-4, 2e-3]))
    s = 0.8 * h
    sp = pkg.default_params(
        param_h=h, param_mass=float(np.float32(1000.0 * s ** 3)), param_restDensity=1000.0, param_gasConstant=2000.0,
        param_viscosity=3.5, param_gravityX=0.0, param_gravityY=-980.0 * h / 0.28, param_gravityZ=0.0, param_surfaceTension=0.0728,
        param_timeStep=dt, param_foamGen=1.0, param_foamVelRef=8.0, param_boxCenter=(0.0, 0.0, 0.0), param_boxHalf=tuple(half),
        param_boxEulerDeg=(0.0, 0.0, 0.0), param_shapeType=0, param_wallRestitution=0.15, param_wallFriction=0.02, grid_cap=160)
    if rng.random() < 0.5:
        sp.param_shapeType = int(rng.integers(0, 15))
        for a in range(3):
            sp.param_shapeAux[a] = float(rng.uniform(0.2, 1.0))
    if rng.random() < 0.4:
        for a in range(3):
            sp.param_boxEulerDeg[a] = float(rng.uniform(-40, 40))
    rec = np.zeros(n, pkg.PARTICLE_DTYPE)
    lo = np.array([-half[0], -half[1], -half[2]], np.float32)
    ext = np.array([2 * half[0], 2 * half[1] * fill, 2 * half[2]], np.float32)
    rec["pos"][:, :3] = lo + rng.random((n, 3)).astype(np.float32) * ext
    rec["pos"][:, 3] = 1.0
    vcap = 0.4 * h / dt
    sigma = float(rng.choice([0.0, 0.02, 0.1, 0.5])) * vcap
    rec["vel"][:, :3] = rng.normal(0, 1, (n, 3)).astype(np.float32) * np.float32(sigma)
    rec["isActive"][:] = 1
    if n > 200 and rng.random() < 0.4:                         # a clump: hundreds of particles inside one cell
        k = int(rng.integers(50, min(n, 1500)))
        rec["pos"][:k, :3] = rec["pos"][0, :3] + rng.normal(0, 0.2 * h, (k, 3)).astype(np.float32)
    if n > 100 and rng.random() < 0.4:                         # ghosts of every kind, some inactive particles
        g = rng.choice(n, size=n // 20, replace=False)
        rec["isGhost"][g] = rng.choice([1, 1, 3], size=len(g))
        rec["isActive"][g[: len(g) // 2]] = 0
    if n > 100 and rng.random() < 0.3:                         # particles outside the grid
        rec["pos"][rng.choice(n, size=n // 50 + 1, replace=False), 0] += np.float32(4.0 * half[0] + 3 * h)
    steps = int(rng.integers(1, 4))
    return rec, sp, steps, dict(h=h, dims=dims, n=n, per_cell=lam, sigma_over_cap=sigma / vcap, dt=dt, steps=steps, shape=int(sp.param_shapeType))


def identity_states(pkg):
    """(name, records, params) of the states the sampling identities are checked on."""
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=7)
    yield "scene4096", np.load(os.path.join(G, "scene4096.npz"))["after_10"], sp
    z = np.load(os.path.join(G, "cylinder2000.npz"))
    sp = pkg.default_params(param_shapeType=2, param_boxHalf=(2.2, 1.6, 0.9), param_boxEulerDeg=(10.0, -25.0, 40.0),
                            param_boxCenter=(0.2, -0.1, 0.3), param_mass=float(z["mass"]))
    yield "cylinder2000", z["after"], sp
    fx = np.load(os.path.join(G, "settled_pool.npz"))
    yield "settled_pool", fx["settled"], pkg.default_params(param_mass=float(fx["mass"]))
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3)
    yield "small_scene", rec, sp


def undisturbed_run(pkg, rec, sp, probe, aos=1, graph=0):
    """The "a read-only feature does not change the simulation" scenario: eager or graph dispatches, an impulse, download, upload,
    download, dispatch, with probe(engine) called between all of them (probe None: the same run without the feature).
    Returns (records after the upload, records at the end, graph launches)."""
    f = pkg.SPHFluidGPU.from_particles(rec, sp)
    f.set_option(pkg.SPH_OPT_AOS_MODE, aos)
    f.set_option(pkg.SPH_OPT_GRAPH, graph)

    def look():
        if probe is not None:
            probe(f)
    look()
    if graph:
        for _ in range(4):
            f.DispatchN(3)
            look()
    else:
        for _ in range(3):
            f.DispatchCompute()
            look()
        f.DispatchN(4)
        look()
        f.ApplyWaveImpulse(1.5, 3.0, 0.25, (0.0, 1.0, 0.0))
        look()
        f.DispatchN(3)
    mid = f.download()
    look()
    f.upload(mid)
    look()
    after_upload = f.download()
    look()
    f.DispatchN(2)
    out = f.download()
    launches = f.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES)
    f.close()
    return after_upload, out, launches


# ---- the spatial queries: what every family's GPU tests repeat --------------------------------------
def same_info(info, want, fields, what):
    """The named fields of two info structs are equal."""
    assert [getattr(info, a) for a in fields] == [getattr(want, a) for a in fields], what


def after_dispatches(pkg, kern, aos, graph, check, unchanged, scene=None):
    """The "a query on a state the engine produced" scenario: an engine for (kern, aos, graph) on `scene` (records, params; None: the
    small scene of 4096), four DispatchN(3) (a graph is captured once a call repeats, then replayed), the download, the family's
    check(engine, records now, params, what), one more DispatchN(3) and the family's unchanged(engine, what check returned): a result
    describes the state it was built from."""
    rec, sp = small_scene(pkg, n=4096, grid=16, seed=3) if scene is None else scene
    f = engine(pkg, rec, sp, kern, aos, graph)
    for _ in range(4):
        f.DispatchN(3)
    if graph:
        assert f.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) >= 1
    now = f.download()
    held = check(f, now, sp, f"kernel {kern} aos {aos} graph {graph}")
    f.DispatchN(3)
    unchanged(f, held)
    f.close()


@contextmanager
def slab_engine(pkg, rec, sp):
    """The first of the two engines every query refuses with -3: a slab engine (here one slab over the whole grid), closed on exit."""
    halo = import_module(pkg.__name__ + ".halo")
    g = pkg.compute_grid_extents(sp)
    slab = halo.HipSlabEngine(rec, np.arange(len(rec), dtype=np.uint32), sp, 0, g.dims[2], False, False, int(len(rec) * 1.2) + 8192)
    try:
        yield slab
    finally:
        slab.close()


@contextmanager
def linked_list_grid(pkg, f):
    """The second: the caller's engine while its grid is built as linked lists (SPH_OPT_GRID_BUILD 1), the option put back on exit."""
    f.set_option(pkg.SPH_OPT_GRID_BUILD, 1)
    try:
        yield f
    finally:
        f.set_option(pkg.SPH_OPT_GRID_BUILD, 0)
