"""The shared assertion helpers of tests/support.py can fail: several test files rest on one copy of each.  No GPU."""
import shutil

import numpy as np
import pytest

from conftest import small_scene, to_oracle_params
import obstacle_ref as R
from support import build_example, check_impulses, fluid_block, same_bits

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


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_build_example_reports_the_compilers_words(pkg, tmp_path):
    with pytest.raises(RuntimeError, match="no_such_example.cpp: No such file"):
        build_example(pkg, "no_such_example", tmp_path)
