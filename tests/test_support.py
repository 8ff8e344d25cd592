"""The shared assertion helpers of tests/support.py can fail: several test files rest on one copy of each.  No GPU."""
import shutil

import numpy as np
import pytest

from conftest import small_scene, to_oracle_params
import obstacle_ref as R
from support import after_dispatches, build_example, check_impulses, fluid_block, same_bits, same_info

F = np.float32


def test_same_bits_accepts_a_non_contiguous_view_of_equal_content():
    a = np.arange(24, dtype=F).reshape(4, 6)
    view = np.ascontiguousarray(a.T).T
    assert not view.flags["C_CONTIGUOUS"]
    same_bits(a, view, "a view")
    same_bits(a[:, ::2], a[:, ::2].copy(), "a strided view")


def test_same_bits_tells_signed_zeros_apart():
    with pytest.raises(AssertionError, match="zeros"):
        same_bits(np.array([0.0], F), np.array([-0.0], F), "zeros")


def test_same_bits_tells_nan_payloads_apart():
    a = np.array([0x7fc00000], np.uint32).view(F)
    b = np.array([0x7fc00001], np.uint32).view(F)
    assert np.isnan(a).all() and np.isnan(b).all()
    same_bits(a, a.copy(), "the same NaN")
    with pytest.raises(AssertionError, match="payloads"):
        same_bits(a, b, "payloads")


def test_same_bits_compares_shapes():
    a = np.arange(6, dtype=F).reshape(2, 3)
    assert a.tobytes() == a.reshape(3, 2).tobytes()
    with pytest.raises(AssertionError, match="shapes"):
        same_bits(a, a.reshape(3, 2), "shapes")


def test_check_impulses_holds_at_the_bound_and_fails_one_ulp_above(pkg, oracle):
    """want + bound is rounded to fp64; where that rounding went away from want, the largest fp64 inside the bound is its neighbour
    towards want.  One ulp above fl(want + bound) is always outside: the exact want + bound is at most fl(want + bound) rounded up."""
    rec, sp = small_scene(pkg, n=4096, grid=16)
    c, E = fluid_block(rec)
    bs = R.bodies(pkg.obstacle_array([pkg.obstacle(R.SPHERE, c, 0.2 * E, vel=(0.5, 0.0, 0.0))]))
    _, _, want, info = R.step(oracle, rec, to_oracle_params(oracle, sp), bs)
    bound = R.impulse_bound(info)
    assert info["touched"][0] > 1 and (bound[0, :3] > 0).all()
    at = want + bound
    over = np.abs(at - want) > bound
    at[over] = np.nextafter(at[over], want[over])
    check_impulses(at, want, info, "at the bound")
    above = at.copy()
    above[0, 1] = np.nextafter(want[0, 1] + bound[0, 1], np.inf)
    with pytest.raises(AssertionError, match="one ulp above"):
        check_impulses(above, want, info, "one ulp above")


def test_same_info_compares_the_named_fields_only(pkg):
    a, b = pkg.SphKnnInfo(rows=5, total=7, k=8), pkg.SphKnnInfo(rows=5, total=9, k=8)
    same_info(a, b, ("rows", "k"), "rows and k")
    with pytest.raises(AssertionError, match="the total"):
        same_info(a, b, ("rows", "total", "k"), "the total")


class _NoDevice:
    """Stands in for the package and for its engine in after_dispatches: it notes what is called and replays no graph."""
    SPH_OPT_NEIGHBOR_KERNEL, SPH_OPT_AOS_MODE, SPH_OPT_GRAPH, SPH_OPT_GRAPH_LAUNCHES = "kern", "aos", "graph", "launches"

    def __init__(self, launches):
        self.SPHFluidGPU, self.options, self.seen = self, {"launches": launches}, []

    def from_particles(self, rec, sp):
        self.seen.append(("engine", rec, sp))
        return self

    def set_option(self, option, value):
        self.options[option] = value

    def get_option(self, option):
        return self.options[option]

    def DispatchN(self, n):
        self.seen.append(("dispatch", n))

    def download(self):
        return "now"

    def close(self):
        self.seen.append("close")


def test_after_dispatches_runs_the_scenario_in_order_and_wants_the_graph_replayed():
    def check(f, now, sp, what):
        f.seen.append(("check", now, sp, what))
        return "held"

    def unchanged(f, held):
        f.seen.append(("unchanged", held))

    fake = _NoDevice(launches=2)
    after_dispatches(fake, 1, 0, 1, check, unchanged, scene=("rec", "sp"))
    assert fake.options == {"kern": 1, "aos": 0, "graph": 1, "launches": 2}
    assert fake.seen == [("engine", "rec", "sp")] + [("dispatch", 3)] * 4 + [("check", "now", "sp", "kernel 1 aos 0 graph 1"), ("dispatch", 3),
                                                                              ("unchanged", "held"), "close"]
    with pytest.raises(AssertionError):
        after_dispatches(_NoDevice(launches=0), 3, 1, 1, check, unchanged, scene=("rec", "sp"))
    eager = _NoDevice(launches=0)                                                   # without a graph no launch is asked for
    after_dispatches(eager, 3, 1, 0, check, unchanged, scene=("rec", "sp"))
    assert eager.seen[-1] == "close"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_build_example_reports_the_compilers_words(pkg, tmp_path):
    with pytest.raises(RuntimeError, match="no_such_example.cpp: No such file"):
        build_example(pkg, "no_such_example", tmp_path)
