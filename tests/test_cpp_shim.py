"""The header-only C++ twin of the reference class (include/SPHFluidGPU_hip.hpp)."""
import os
import shutil

import pytest

from conftest import ROOT
from support import build_example, check_shim_syntax, run_example


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_shim_compiles_and_links_against_the_c_abi(pkg, tmp_path):
    check_shim_syntax()
    assert os.path.exists(build_example(pkg, "headless_scene", tmp_path))
    src = open(os.path.join(ROOT, "include", "SPHFluidGPU_hip.hpp")).read()
    for name in ("DispatchCompute", "ResetSimulation", "ApplyWaveImpulse", "EffectiveHalf", "ComputeGridExtents", "GetNumFluids",
                 "param_h", "param_mass", "param_restDensity", "param_gasConstant", "param_viscosity", "param_gravityY",
                 "param_surfaceTension", "param_timeStep", "param_pause", "param_boxCenter", "param_boxHalf", "param_boxEulerDeg",
                 "param_shapeType", "param_shapeAux", "param_wallRestitution", "param_wallFriction", "numParticles", "particles",
                 "gridSizeX", "numCells", "gridMinV", "cellSize", "GetFluidVBO", "ssbo", "riverMode"):
        assert name in src, name


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_headless_scene_runs_on_the_gpu(pkg, tmp_path):
    """Scene0p's call pattern (ctor, per-frame impulse, 16-substep frames, param edits, reset)
    through the C++ shim."""
    res = run_example(build_example(pkg, "headless_scene", tmp_path), ["50000"], timeout=300)
    assert res.returncode == 0 and "headless_scene OK" in res.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_slab_example_links_against_the_c_abi(pkg, tmp_path):
    assert os.path.exists(build_example(pkg, "slab_pair", tmp_path))


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_slab_pair_through_the_c_abi_only(pkg, tmp_path):
    """A C++ host drives two z-slab engines through include/sph_abi.h alone (device-side counts, no host round trip in
    the exchange) and gets the single-engine result bit for bit."""
    res = run_example(build_example(pkg, "slab_pair", tmp_path), ["60000", "24"], timeout=300)
    assert res.returncode == 0 and "slab_pair OK" in res.stdout
