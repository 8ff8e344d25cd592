"""Scenes shared by the free-surface tests (test_shell_cpu.py, test_gpu_shell.py): jittered lattices at h = 0.28 with spacing
dx = h / 2.4 and a jitter of +-0.2 dx per axis from a seeded generator, all well inside the default container (half-extent 7): a block
of 20^3, balls of radius 10 dx and 5 dx, and a block of 24^3 with a spherical hole of radius 5 dx.  Every scene is (records, params,
nominal): nominal holds the lattice positions before the jitter in units of dx, which is what the geometric statements select by."""
import numpy as np

from support import records

F = np.float32
H = 0.28
DX = H / 2.4
JITTER = 0.2


def params(pkg):
    return pkg.default_params(param_h=H)


def _scene(pkg, nominal, seed):
    rng = np.random.default_rng(seed)
    pos = ((nominal + (rng.random(nominal.shape) * 2.0 - 1.0) * JITTER) * DX).astype(F)
    return records(pkg, pos, np.zeros_like(pos)), params(pkg), nominal


def _lattice(side, half_integers):
    ax = np.arange(side, dtype=np.float64) - (side - 1) / 2.0 if half_integers else np.arange(-side, side + 1, dtype=np.float64)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)


def block(pkg, side=20, seed=102):
    """side^3 particles; the outermost lattice planes are at +-(side - 1) / 2 dx.  (The seed: see test_shell_cpu.test_what_the_shell_is_block.)"""
    return _scene(pkg, _lattice(side, True), seed)


def ball(pkg, radius, seed=102):
    """The lattice points (a particle at the centre) within `radius` spacings of the centre."""
    g = _lattice(int(np.ceil(radius)), False)
    return _scene(pkg, g[(g * g).sum(axis=1) <= radius * radius], seed + int(radius))


def hole(pkg, side=24, radius=5.0, seed=103):
    """A block of side^3 without the lattice points closer than `radius` spacings to its centre."""
    g = _lattice(side, True)
    return _scene(pkg, g[(g * g).sum(axis=1) >= radius * radius], seed)


def depth(nominal_or_pos, side):
    """Distance (in dx) below the nearest nominal face plane of a block of side^3, per particle, and the axis / sign of that face."""
    p = np.asarray(nominal_or_pos, np.float64)
    d = (side - 1) / 2.0 - np.abs(p)
    ax = d.argmin(axis=1)
    return d.min(axis=1), ax, np.sign(p[np.arange(len(p)), ax])
