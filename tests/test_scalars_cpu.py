"""Diffusing scalar channels without a GPU: the host twin sph_scalars_step_host against the numpy restatement
of tests/scalar_ref.py bit for bit, and the operator's properties (conservation, maximum principle, consistency with D k^2) against
the restatement's float64 evaluation, with rounding bounds derived in scalar_ref."""
import os

import numpy as np
import pytest

from conftest import to_oracle_params
import scalar_ref as R
import support
from support import same_bits

F = np.float32
DT = 0.004


def _grid(oracle, rec, sp):
    b = oracle.build_grid(rec, to_oracle_params(oracle, sp))
    return b["grid"], b["cell_start"], b["order"]


def _values(n, K, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 2.0, (n, K)).astype(F)


def _ghost_scene(pkg):
    rec, sp = support.small_scene(pkg, n=1200, grid=12, seed=5)
    rec = rec.copy()
    rec["density"] = 1000.0
    mask = np.zeros(len(rec), np.int32)
    mask[::7] = 1
    mask[3::11] = 2
    out = support.records(pkg, rec["pos"][:, :3], rec["vel"][:, :3], ghost=mask)
    out["isActive"] = 1
    return out, sp


def _states(pkg):
    yield from support.identity_states(pkg)
    rec, sp = _ghost_scene(pkg)
    yield "ghost_scene", rec, sp


def _unit_number_diffusivity(pkg, rec, sp, target, dt=DT):
    """D with which the twin reports the diffusion number `target` on this state (the number is linear in D)."""
    _, s1 = pkg.scalars_step_host(rec, sp, np.zeros(len(rec), F), diffusivity=1.0, dt=dt)
    return F(target / float(s1)) if s1 > 0 else F(1.0)                 # (records before their first substep: 1/rho = 0, nothing diffuses)


@pytest.fixture(scope="module")
def pool(pkg, oracle):
    """settled_pool with D chosen for a diffusion number of 0.5, a step-plus-noise field, and the float64 evaluation of one substep."""
    fx = np.load(os.path.join(support.G, "settled_pool.npz"))
    rec, sp = fx["settled"], pkg.default_params(param_mass=float(fx["mass"]))
    D = _unit_number_diffusivity(pkg, rec, sp, 0.5)
    rng = np.random.default_rng(11)
    y = rec["pos"][:, 1]
    c0 = ((y > np.median(y)).astype(F) + rng.uniform(0.0, 0.25, len(rec)).astype(F)).astype(F).reshape(-1, 1)
    grid = _grid(oracle, rec, sp)
    ref = R.step64(rec, c0, sp.param_h, sp.param_mass, D, 0.0, DT, *grid)
    return dict(rec=rec, sp=sp, D=D, c0=c0, grid=grid, ref=ref)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_restatement_matches_the_host_twin_bit_for_bit(pkg, oracle, K):
    for name, rec, sp in _states(pkg):
        c = _values(len(rec), K, 3 + K)
        D = np.linspace(2.0, 0.5, K).astype(F) * _unit_number_diffusivity(pkg, rec, sp, 0.4)
        lam = np.linspace(0.0, 3.0, K).astype(F)
        got, s = pkg.scalars_step_host(rec, sp, c, diffusivity=D, decay=lam, dt=DT)
        want, s_want = R.step32(rec, c, sp.param_h, sp.param_mass, D, lam, DT, *_grid(oracle, rec, sp))
        same_bits(got, want, f"{name} K={K}")
        assert F(s).tobytes() == F(s_want).tobytes(), (name, K, s, s_want)
        if name == "small_scene":                                        # spawned records, density 0: no targets
            same_bits(got, c, name)
            assert s == 0
        else:
            assert (got != c).any() and s > 0


def test_sum_is_conserved_within_the_rounding_bound(pkg, pool):
    got, s = pkg.scalars_step_host(pool["rec"], pool["sp"], pool["c0"], diffusivity=pool["D"], dt=DT)
    tgt = pool["ref"]["targets"]
    before = pool["c0"][tgt, 0].astype(np.float64).sum()
    after = got[tgt, 0].astype(np.float64).sum()
    bound = R.rounding_bound(pool["ref"], pool["c0"]).sum()
    ref_drift = abs(pool["ref"]["values"][tgt, 0].sum() - before)
    print(f"sum {before:.9g} -> {after:.9g}: drift {abs(after - before):.3g}, bound {bound:.3g}, float64 evaluation drifts {ref_drift:.3g}; number {s}")
    assert ref_drift <= 1e-9 * max(abs(before), 1.0)                    # the formula itself conserves (symmetric weights)
    assert abs(after - before) <= bound


def test_maximum_principle_and_variance_at_number_one_half(pkg, pool):
    rec, sp, D, c = pool["rec"], pool["sp"], pool["D"], pool["c0"]
    tgt = pool["ref"]["targets"]
    lo, hi = float(c[tgt].min()), float(c[tgt].max())
    # one substep moves a value by rounding at most rounding_bound beyond a convex combination of values in [lo, hi]; the spread of
    # any later field is at most W (hi - lo)
    ref = pool["ref"]
    per_step = ((ref["pairs"] + 4.0) * R.EPS32 * (max(abs(lo), abs(hi)) + ref["scale"][0, 0] * ref["W"] * (hi - lo)))[tgt].max()
    var = [c[tgt, 0].astype(np.float64).var()]
    for step in range(20):
        c, s = pkg.scalars_step_host(rec, sp, c, diffusivity=D, dt=DT)
        assert abs(float(s) - 0.5) < 1e-5
        var.append(c[tgt, 0].astype(np.float64).var())
        assert c[tgt].min() >= lo - (step + 1) * per_step and c[tgt].max() <= hi + (step + 1) * per_step
    slack = 2.0 * (hi - lo) * per_step
    print(f"variance {var[0]:.6g} -> {var[-1]:.6g}; per-step bound {per_step:.3g}")
    assert all(b <= a + slack for a, b in zip(var, var[1:]))
    assert var[-1] < 0.9 * var[0]


def _mode_fraction(pkg, oracle, spacing_over_h, m, steps=1, twin=False):
    """Decay rate of cos(k x), k = 2 pi / (16 h), at the centre particle (density rho) of an m^3 lattice, as a fraction of
    (D / rho) k^2 (the operator carries 1 / (rho_i rho_j): D is Cleary-Monaghan's coefficient, rho times a diffusivity); float64
    restatement, or the host twin.  rate = (1 - (c_n / c_0)^(1 / n)) / dt: exact for an eigenfunction of the lattice operator."""
    rec, sp = R.cubic_lattice(pkg, oracle, m, spacing_over_h)
    h = float(F(sp.param_h))
    k = 2.0 * np.pi / (16.0 * h)
    c0 = np.cos(k * rec["pos"][:, 0].astype(np.float64)).astype(F).reshape(-1, 1)
    grid = _grid(oracle, rec, sp)
    one = R.step64(rec, c0, sp.param_h, sp.param_mass, 1.0, 0.0, DT, *grid)
    centre = len(rec) // 2
    assert np.allclose(rec["pos"][centre, :3], 0.0, atol=1e-6) and c0[centre, 0] == 1.0
    D = F(0.2 / one["number"][centre])
    c64, c32, tol = c0.astype(np.float64), c0, 0.0
    for _ in range(steps):
        ref = R.step64(rec, c64, sp.param_h, sp.param_mass, D, 0.0, DT, *grid)
        tol += R.value_bound(ref, c64).max()                             # (number <= 1: a substep does not amplify the error carried in)
        c64 = ref["values"]
        if twin:
            c32, _ = pkg.scalars_step_host(rec, sp, c32, diffusivity=D, dt=DT)
    unit = float(D) / float(rec["density"][centre]) * k * k
    rate = lambda c: (1.0 - (float(c[centre, 0]) / float(c0[centre, 0])) ** (1.0 / steps)) / DT
    if not twin:
        return rate(c64) / unit
    return rate(c32) / unit, rate(c64) / unit, abs(float(c32[centre, 0]) - float(c64[centre, 0])), tol


@pytest.fixture(scope="module")
def half_h_mode(pkg, oracle):
    return _mode_fraction(pkg, oracle, 0.5, 21, steps=10, twin=True)


def test_decay_of_a_sine_mode_matches_the_float64_evaluation(half_h_mode):
    """Ten substeps of the twin against ten of the float64 evaluation on a cubic lattice at spacing h / 2 (21^3 particles, the centre
    particle five supports from the faces): the values agree within the accumulated rounding bound of scalar_ref.value_bound."""
    got, want, err, tol = half_h_mode
    print(f"fraction of (D / rho) k^2 at spacing h/2: twin {got:.6f}, float64 {want:.6f}; |c_twin - c_64| {err:.3g} <= {tol:.3g}")
    assert err <= tol
    assert 0.5 < want < 1.0


def test_decay_rate_lies_between_the_fractions_of_coarser_and_finer_lattices(pkg, oracle, half_h_mode):
    """The rate at spacing 0.5 h lies between the fractions of (D / rho) k^2 that the float64 restatement gives at 0.6 h and at 0.4 h.
    The lattices carry the densities the engine's density sweep gives them (scalar_ref.cubic_lattice), rho being the centre particle's.
    Float64, k = 2 pi / (16 h): 0.3 h 0.9459 (170 pairs), 0.4 h 0.9189 (80), 0.45 h 0.9060 (32), 0.5 h 0.9176 (26), 0.55 h 0.8967 (26),
    0.6 h 0.8459 (18), 0.7 h 0.6267 (18), 0.85 h 0.3029 (6): the figures DESIGN.md section 3h quotes.  (With densities set by hand to
    m / a^3 the order of 0.4 h and 0.5 h is the other way round, 0.9147 and 0.9266: the fraction is not monotone in the spacing, whole
    shells of neighbours enter the support at once, and the bracket is 0.0013 wide at its upper end.)"""
    got, want, _, _ = half_h_mode
    coarse, fine = _mode_fraction(pkg, oracle, 0.6, 17), _mode_fraction(pkg, oracle, 0.4, 25)
    print(f"fraction at 0.5 h: twin {got:.6f}, float64 {want:.6f}; 0.6 h {coarse:.6f}, 0.4 h {fine:.6f}")
    assert min(coarse, fine) < got < max(coarse, fine)


def test_records_that_are_no_targets_keep_their_bits(pkg):
    rec, sp = _ghost_scene(pkg)
    rec = rec.copy()
    fluid = np.nonzero(rec["isGhost"] == 0)[0]
    nan, inf, fresh, lone = fluid[5], fluid[9], fluid[20:30], fluid[40]
    rec["pos"][nan, 1] = np.nan
    rec["pos"][inf, 0] = np.inf
    rec["density"][fresh] = 0.0
    rec["density"][fluid[31]] = -1.0
    rec["pos"][lone, :3] = (50.0, 50.0, 50.0)                            # outside the grid: the clamped corner cell, nobody within h
    c = _values(len(rec), 2, 9)
    got, s = pkg.scalars_step_host(rec, sp, c, diffusivity=_unit_number_diffusivity(pkg, rec, sp, 0.3), decay=0.0, dt=DT)
    keep = np.concatenate([np.nonzero(rec["isGhost"] != 0)[0], [nan, inf, fluid[31], lone], fresh])
    same_bits(got[keep], c[keep], "ghosts, non-finite positions, density <= 0 and a target without a pair")
    moved = np.setdiff1d(fluid, keep)
    assert (got[moved] != c[moved]).any(axis=1).mean() > 0.9
    # decay alone reaches the lone target (it is one), not the others
    got, _ = pkg.scalars_step_host(rec, sp, c, diffusivity=0.0, decay=2.0, dt=DT)
    want = (c[lone] + F(DT) * (F(0.0) - (F(2.0) * c[lone]).astype(F)).astype(F)).astype(F)
    same_bits(got[lone], want, "decay of a target without a pair")
    rest = np.setdiff1d(keep, [lone])
    same_bits(got[rest], c[rest], "no decay outside the targets")
    # a paused engine does not step
    paused = pkg.SphParams.from_buffer_copy(bytes(sp))
    paused.param_pause = 1
    got, s = pkg.scalars_step_host(rec, paused, c, diffusivity=1.0, dt=DT)
    same_bits(got, c, "param_pause")
    assert s == 0


def test_python_layer_errors_and_mixing_index(pkg):
    rec, sp = _ghost_scene(pkg)
    c = np.zeros(len(rec), F)
    for kw in (dict(diffusivity=-1.0), dict(diffusivity=np.nan), dict(decay=-0.5), dict(decay=np.inf)):
        with pytest.raises(pkg.SphError, match="sph C-ABI error -1"):
            pkg.scalars_step_host(rec, sp, c, **kw)
    with pytest.raises(pkg.SphError, match="-1"):
        pkg.scalars_step_host(rec, sp, np.zeros((len(rec), 5), F))
    with pytest.raises(pkg.SphError, match="shape"):
        pkg.scalars_step_host(rec, sp, np.zeros(len(rec) - 1, F))
    got, s = pkg.scalars_step_host(rec[:0], sp, np.zeros((0, 2), F), diffusivity=1.0)
    assert got.shape == (0, 2) and s == 0
    assert pkg.mixing_index(0.25, 1.0) == 0.75 and pkg.mixing_index(1.0, 1.0) == 0.0 and pkg.mixing_index(0.0, 2.0) == 1.0
    with pytest.raises(pkg.SphError):
        pkg.mixing_index(0.1, 0.0)
    m = pkg.SphScalarMoments()
    m.count, m.sum, m.sumSquares = 4, 6.0, 14.0                          # values 0, 1, 2, 3
    mom = pkg.ScalarMoments(m)
    assert mom.mean == 1.5 and mom.variance == 14.0 / 4 - 1.5 ** 2 and mom.mixing_index(2.5) == 1.0 - 1.25 / 2.5
    assert pkg.SPH_MAX_SCALAR_CHANNELS == 4 and (pkg.SPH_SCALAR_SET, pkg.SPH_SCALAR_ADD) == (0, 1)
    for sym in ("sph_scalars_set", "sph_scalars_paint", "sph_scalars_moments", "sph_scalars_sample_lattice", "sph_scalars_step_host"):
        assert sym in pkg.ABI_SYMBOLS
    support.check_shim_syntax()
