"""Host-side mirror of the reference's `SPHFluidGPU` class over the C-ABI (include/sph_abi.h).

The reference boundary is the C++ class SPHFluidGPU
(ComponentFramework/SPHFluid3D.h:26-210): public methods plus public
`param_*` data members that the caller pokes directly (Scene0p.cpp:936-1056) and that are
re-read at every DispatchCompute (SPHFluid3D.cpp:458-506).  This module keeps those names:
`DispatchCompute`, `ResetSimulation`, `ApplyWaveImpulse`, `EffectiveHalf`, `GetNumFluids`,
`ComputeGridExtents`, `param_h` ... `param_wallFriction`, `numParticles`, `particles`,
`gridSizeX/Y/Z`, `numCells`, `gridMinV`, `cellSize`.  The C++ twin of this file is
include/SPHFluidGPU_hip.hpp.

There is no CPU fallback: if libsph_hip.so is missing or HIP has no device, construction
raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import build as _build

# ---- constants and structs, in the order of include/sph_abi.h ---------------------------------------------------------
FLT_MAX = 3.4028234663852886e38
SPH_ERR_TIMEOUT = -5

# 80-byte record, SPHFluid3D.h:12-24
PARTICLE_DTYPE = np.dtype(
    [
        ("pos", "<f4", (4,)), ("vel", "<f4", (4,)), ("acc", "<f4", (4,)),
        ("density", "<f4"), ("pressure", "<f4"), ("padA", "<f4"), ("padB", "<f4"),
        ("isGhost", "<i4"), ("isActive", "<i4"), ("padC", "<i4"), ("pad0", "<i4"),
    ]
)
assert PARTICLE_DTYPE.itemsize == 80


class SphParams(C.Structure):
    """struct SphParams of include/sph_abi.h (param_* members, SPHFluid3D.h:94-124)."""

    _fields_ = [
        ("param_h", C.c_float), ("param_mass", C.c_float), ("param_restDensity", C.c_float),
        ("param_gasConstant", C.c_float), ("param_viscosity", C.c_float),
        ("param_gravityY", C.c_float), ("param_gravityX", C.c_float), ("param_gravityZ", C.c_float),
        ("param_surfaceTension", C.c_float), ("param_timeStep", C.c_float),
        ("param_pause", C.c_int32),
        ("param_useJitter", C.c_int32), ("param_jitterAmp", C.c_float),
        ("param_foamGen", C.c_float), ("param_foamVelRef", C.c_float),
        ("param_boxCenter", C.c_float * 3), ("param_boxHalf", C.c_float * 3), ("param_boxEulerDeg", C.c_float * 3),
        ("param_shapeType", C.c_int32), ("param_shapeAux", C.c_float * 3),
        ("param_mixPattern", C.c_int32), ("param_dyePattern", C.c_int32),
        ("param_wallRestitution", C.c_float), ("param_wallFriction", C.c_float),
        ("grid_cap", C.c_int32),
    ]


class SphGridInfo(C.Structure):
    _fields_ = [("dims", C.c_int32 * 3), ("numCells", C.c_int32), ("gridMin", C.c_float * 3), ("cellSize", C.c_float)]


class SphFountain(C.Structure):
    """fountain* members of the reference class (SPHFluid3D.h:161-168), same names."""
    _fields_ = [("fountainMode", C.c_int32), ("fountainOffset", C.c_float * 3), ("fountainRadius", C.c_float),
                ("fountainSpread", C.c_float), ("fountainJetSpeedLive", C.c_float), ("fountainDrainLevel", C.c_float),
                ("fountainDrainPerSec", C.c_float), ("fountainSeed", C.c_uint32)]


class SphRiver(C.Structure):
    """river / terrain members of the reference class (SPHFluid3D.h:171-196), same names."""
    _fields_ = [("riverMode", C.c_int32), ("terrainW", C.c_int32), ("terrainH", C.c_int32),
                ("terrainWorldMinX", C.c_float), ("terrainWorldMinZ", C.c_float), ("terrainWorldSizeX", C.c_float), ("terrainWorldSizeZ", C.c_float),
                ("riverEmitterPos", C.c_float * 3), ("riverEmitterVel", C.c_float * 3), ("riverEmitterRadius", C.c_float),
                ("riverSinkY", C.c_float), ("riverSinkZMax", C.c_float), ("riverAmp", C.c_float), ("riverFreq", C.c_float),
                ("riverPhase", C.c_float), ("riverChannelWidth", C.c_float), ("riverChannelDepth", C.c_float), ("riverSlopeDrop", C.c_float)]


# option constants of sph_abi.h
SPH_OPT_NEIGHBOR_KERNEL, SPH_OPT_GRID_BUILD, SPH_OPT_AOS_MODE, SPH_OPT_TIMING, SPH_OPT_DEBUG = 1, 2, 3, 4, 100
SPH_OPT_GRAPH, SPH_OPT_GRAPH_LAUNCHES = 5, 6
SPH_OPT_MESH_SPLIT = 7
SPH_OPT_SCALAR_SWEEP = 8
SPH_OPT_DIFFUSE_TIMED = 9
SPH_OPT_NEIGHBORS_FILL = 10
SPH_OPT_COMPONENTS_VARIANT = 11
SPH_OPT_KNN_VARIANT = 12
SPH_OPT_RAYS_VARIANT = 13
SPH_OPT_RAY_SPANS_VARIANT = 15
SPH_OPT_SHELL_TIMED = 14
SPH_OPT_AGGREGATE_VARIANT = 16
# sph_debug_counters (SPH_OPT_DEBUG bit 3): diagnostics of k_sph_walk / k_sph_list, summed over launches:
# [0] candidate rows walked from global memory (window too large; k_sph_walk), [1] targets on an exact fallback sweep,
# [2] neighbour-list entries, [3] candidate rows (k_sph_walk), [4] lanes, [5] targets whose list overflowed, [6] targets that
# left the list's slack, [7] waves with at least one fallback target
STAMP_NAMES = ("rows_unstaged", "slow_targets", "list_entries", "rows", "lanes", "overflow_targets", "far_targets", "waves_with_fallback")


class SphSample(C.Structure):
    """struct SphSample of include/sph_abi.h: the fields of the fluid at one probe point (see SPHFluidGPU.sample)."""
    _fields_ = [("density", C.c_float), ("fraction", C.c_float), ("pressure", C.c_float), ("count", C.c_uint32),
                ("vel", C.c_float * 3), ("pad", C.c_float)]


assert C.sizeof(SphSample) == 32
SAMPLE_DTYPE = np.dtype(SphSample)
assert SAMPLE_DTYPE.itemsize == 32
SPH_FIELD_DENSITY, SPH_FIELD_FRACTION, SPH_FIELD_PRESSURE, SPH_FIELD_SPEED, SPH_FIELD_ALL = 0, 1, 2, 3, 4


SURFACE_VERTEX_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,))])     # struct SphSurfaceVertex
assert SURFACE_VERTEX_DTYPE.itemsize == 24


class SphSurface(C.Structure):
    """struct SphSurface of include/sph_abi.h: counts and borrowed device arrays of the last extracted surface."""
    _fields_ = [("numVertices", C.c_uint32), ("numTriangles", C.c_uint32), ("vertices", C.c_void_p), ("triangles", C.c_void_p)]


class SphStatExtremum(C.Structure):
    """struct SphStatExtremum of include/sph_abi.h: an extreme value and the particle id that attains it."""
    _fields_ = [("value", C.c_float), ("id", C.c_uint32)]


class SphStatistics(C.Structure):
    """struct SphStatistics of include/sph_abi.h: 832 bytes."""
    _fields_ = [
        ("numRecords", C.c_uint64), ("numFluid", C.c_uint64), ("numActiveGhosts", C.c_uint64), ("numInactiveGhosts", C.c_uint64),
        ("numOther", C.c_uint64), ("numNonFinite", C.c_uint64), ("numCounted", C.c_uint64), ("numEscaped", C.c_uint64),
        ("firstNonFiniteId", C.c_uint32), ("firstEscapedId", C.c_uint32),
        ("minPos", SphStatExtremum * 3), ("maxPos", SphStatExtremum * 3), ("minDensity", SphStatExtremum), ("maxDensity", SphStatExtremum),
        ("minPressure", SphStatExtremum), ("maxPressure", SphStatExtremum), ("maxFoam", SphStatExtremum), ("maxSpeed2", SphStatExtremum),
        ("maxSpeed", C.c_float), ("reserved0", C.c_uint32),
        ("sumPos", C.c_double * 3), ("sumVel", C.c_double * 3), ("sumSpeed2", C.c_double), ("sumDensity", C.c_double),
        ("sumDensity2", C.c_double), ("sumPressure", C.c_double), ("sumFoam", C.c_double), ("sumInvDensity", C.c_double),
        ("sumAngular", C.c_double * 3),
        ("occupiedCells", C.c_uint64), ("maxCellCount", C.c_uint32), ("maxCellIndex", C.c_uint32),
        ("occupancy", C.c_uint64 * 65),
    ]


assert C.sizeof(SphStatistics) == 832


class SphHistogramSpec(C.Structure):
    """struct SphHistogramSpec of include/sph_abi.h: field (SPH_STAT_*), bins (1 .. 1024), lo < hi."""
    _fields_ = [("field", C.c_int32), ("bins", C.c_uint32), ("lo", C.c_float), ("hi", C.c_float)]


SPH_STAT_DENSITY, SPH_STAT_PRESSURE, SPH_STAT_SPEED, SPH_STAT_POS_X, SPH_STAT_POS_Y, SPH_STAT_POS_Z, SPH_STAT_FOAM = range(7)
SPH_STAT_MAX_SPECS, SPH_STAT_MAX_BINS = 4, 1024


class SphTracer(C.Structure):
    """struct SphTracer of include/sph_abi.h: one passive tracer (see SPHFluidGPU.set_tracers)."""
    _fields_ = [("pos", C.c_float * 3), ("age", C.c_float), ("vel", C.c_float * 3), ("fraction", C.c_float)]


assert C.sizeof(SphTracer) == 32
TRACER_DTYPE = np.dtype(SphTracer)
assert TRACER_DTYPE.itemsize == 32
SPH_TRACER_EULER, SPH_TRACER_MIDPOINT = 0, 1


class SphDiffuse(C.Structure):
    """struct SphDiffuse of include/sph_abi.h: one spray, foam or bubble particle (see SPHFluidGPU.set_diffuse)."""
    _fields_ = [("pos", C.c_float * 3), ("life", C.c_float), ("vel", C.c_float * 3), ("age", C.c_float),
                ("parent", C.c_uint32), ("birth", C.c_uint32), ("kind", C.c_uint32), ("pad", C.c_uint32)]


class SphDiffuseConfig(C.Structure):
    """struct SphDiffuseConfig of include/sph_abi.h; diffuse_config() fills one."""
    _fields_ = [("capacity", C.c_uint32), ("seed", C.c_uint32), ("threshold", C.c_float), ("rate", C.c_float), ("lifeMin", C.c_float),
                ("lifeMax", C.c_float), ("spread", C.c_float), ("maxAge", C.c_float), ("sprayBelow", C.c_uint32), ("bubbleAbove", C.c_uint32),
                ("kb", C.c_float), ("kd", C.c_float), ("maxPerParent", C.c_uint32), ("pad", C.c_uint32 * 3)]


class SphDiffuseInfo(C.Structure):
    """struct SphDiffuseInfo of include/sph_abi.h: the device counter, the alive count and the running totals of the pool."""
    _fields_ = [("substeps", C.c_uint64), ("spawned", C.c_uint64), ("dropped", C.c_uint64), ("diedLife", C.c_uint64), ("diedAge", C.c_uint64),
                ("leftBox", C.c_uint64), ("nonFinite", C.c_uint64), ("seeded", C.c_uint64), ("alive", C.c_uint32), ("capacity", C.c_uint32),
                ("aliveByKind", C.c_uint32 * 3), ("pad", C.c_uint32)]


class SphDiffuseCrest(C.Structure):
    """struct SphDiffuseCrest of include/sph_abi.h: the pool's second birth term, at wave crests;
    diffuse_crest_config() fills one."""
    _fields_ = [("rate", C.c_float), ("radius", C.c_float), ("offset", C.c_float), ("minCount", C.c_uint32), ("flags", C.c_int32),
                ("crestMin", C.c_float), ("crestMax", C.c_float), ("speedMin", C.c_float), ("speedMax", C.c_float), ("align", C.c_float),
                ("every", C.c_uint32), ("pad", C.c_uint32)]


class SphDiffuseCrestInfo(C.Structure):
    """struct SphDiffuseCrestInfo of include/sph_abi.h: the books of the crest term."""
    _fields_ = [("acting", C.c_uint64), ("crestSpawned", C.c_uint64), ("shellSize", C.c_uint32), ("on", C.c_int32), ("radius", C.c_float),
                ("stencil", C.c_int32)]


assert C.sizeof(SphDiffuse) == 48 and C.sizeof(SphDiffuseConfig) == 64 and C.sizeof(SphDiffuseInfo) == 88
assert C.sizeof(SphDiffuseCrest) == 48 and C.sizeof(SphDiffuseCrestInfo) == 32
DIFFUSE_DTYPE = np.dtype(SphDiffuse)
assert DIFFUSE_DTYPE.itemsize == 48
SPH_DIFFUSE_SPRAY, SPH_DIFFUSE_FOAM, SPH_DIFFUSE_BUBBLE = 0, 1, 2


SPH_MAX_SCALAR_CHANNELS = 4
SPH_SCALAR_SET, SPH_SCALAR_ADD = 0, 1


class SphScalarMoments(C.Structure):
    """struct SphScalarMoments of include/sph_abi.h: count, fp64 sum and sum of squares, extrema of one scalar channel."""
    _fields_ = [("count", C.c_uint64), ("sum", C.c_double), ("sumSquares", C.c_double), ("min", SphStatExtremum), ("max", SphStatExtremum)]


assert C.sizeof(SphScalarMoments) == 40


class SphObstacle(C.Structure):
    """struct SphObstacle of include/sph_abi.h: one kinematic solid body (see obstacle() and SPHFluidGPU.set_obstacles)."""
    _fields_ = [("shape", C.c_int32), ("size", C.c_float * 3), ("center", C.c_float * 3), ("rotation", C.c_float * 4),
                ("vel", C.c_float * 3), ("omega", C.c_float * 3), ("restitution", C.c_float), ("friction", C.c_float)]


assert C.sizeof(SphObstacle) == 76
OBSTACLE_DTYPE = np.dtype(SphObstacle)
assert OBSTACLE_DTYPE.itemsize == 76
SPH_MAX_OBSTACLES = 16
SPH_OBSTACLE_SPHERE, SPH_OBSTACLE_BOX, SPH_OBSTACLE_CAPSULE = 0, 1, 2


class SphVolumeHost(C.Structure):
    """struct SphVolumeHost of include/sph_abi.h: one lattice of signed distances in host memory (see obstacles_apply_host_volumes)."""
    _fields_ = [("values", C.c_void_p), ("dims", C.c_int * 3), ("spacing", C.c_float * 3)]


SPH_MAX_VOLUMES = 16


class SphObstacleDynamics(C.Structure):
    """struct SphObstacleDynamics of include/sph_abi.h: what makes a body of the obstacle set dynamic (see dynamics() and
    SPHFluidGPU.set_obstacle_dynamics)."""
    _fields_ = [("mass", C.c_float), ("inertia", C.c_float * 6), ("com", C.c_float * 3), ("gravityScale", C.c_float),
                ("force", C.c_float * 3), ("torque", C.c_float * 3), ("linearDamping", C.c_float), ("angularDamping", C.c_float),
                ("flags", C.c_uint32)]


assert C.sizeof(SphObstacleDynamics) == 80
DYNAMICS_DTYPE = np.dtype(SphObstacleDynamics)
assert DYNAMICS_DTYPE.itemsize == 80
SPH_DYNAMICS_CONFINED = 1


class SphScalarSource(C.Structure):
    """struct SphScalarSource of include/sph_abi.h: one continuous source or sink of a scalar channel (see scalar_source() and
    SPHFluidGPU.set_scalar_sources)."""
    _fields_ = [("shape", C.c_int32), ("channel", C.c_int32), ("mode", C.c_int32), ("body", C.c_int32), ("center", C.c_float * 3),
                ("size", C.c_float * 3), ("rate", C.c_float), ("target", C.c_float), ("pad", C.c_float * 4)]


assert C.sizeof(SphScalarSource) == 64
SOURCE_DTYPE = np.dtype(SphScalarSource)
assert SOURCE_DTYPE.itemsize == 64
SPH_MAX_SCALAR_SOURCES = 8
SPH_SOURCE_SPHERE, SPH_SOURCE_BOX = 0, 1
SPH_SOURCE_RATE, SPH_SOURCE_RELAX = 0, 1


class SphGate(C.Structure):
    """struct SphGate of include/sph_abi.h: one flow gate, an oriented planar patch fixed in the world (see gate() and
    SPHFluidGPU.set_gates)."""
    _fields_ = [("shape", C.c_int32), ("flags", C.c_int32), ("center", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3),
                ("pad", C.c_float * 5)]


class SphGateBooks(C.Structure):
    """struct SphGateBooks: the cumulative books of one gate."""
    _fields_ = [("forward", C.c_uint64), ("backward", C.c_uint64), ("vel", C.c_double * 3), ("scalar", C.c_double * 4)]


assert C.sizeof(SphGate) == 64 and C.sizeof(SphGateBooks) == 72
GATE_DTYPE = np.dtype(SphGate)
GATE_BOOKS_DTYPE = np.dtype(SphGateBooks)
assert GATE_DTYPE.itemsize == 64 and GATE_BOOKS_DTYPE.itemsize == 72
SPH_MAX_GATES = 8
SPH_MAX_GATE_HISTORY = 4096
SPH_GATE_RECT, SPH_GATE_ELLIPSE = 0, 1
SPH_GATE_UNBOUNDED = 1


class SphMonitorConfig(C.Structure):
    """struct SphMonitorConfig of include/sph_abi.h: how a field monitor samples (monitor_config() fills one)."""
    _fields_ = [("every", C.c_uint32), ("wetFraction", C.c_float), ("history", C.c_uint32), ("stride", C.c_uint32), ("ringPoints", C.c_uint32),
                ("pad", C.c_uint32)]


class SphMonitorRow(C.Structure):
    """struct SphMonitorRow: the running sums of one monitor point."""
    _fields_ = [("samples", C.c_uint64), ("wet", C.c_uint64), ("sumFraction", C.c_double), ("sumFraction2", C.c_double), ("sumDensity", C.c_double),
                ("sumPressure", C.c_double), ("sumPressure2", C.c_double), ("sumVel", C.c_double * 3), ("sumVelVel", C.c_double * 6)]


class SphMonitorInfo(C.Structure):
    """struct SphMonitorInfo: what a monitor slot holds, with the device's counters (see SPHFluidGPU.monitor_info)."""
    _fields_ = [("kind", C.c_int32), ("dims", C.c_int32 * 3), ("points", C.c_uint64), ("config", SphMonitorConfig), ("substeps", C.c_uint64),
                ("acting", C.c_uint64), ("time", C.c_double), ("firstRow", C.c_uint64), ("ringRows", C.c_uint32), ("pad", C.c_uint32),
                ("origin", C.c_float * 3), ("spacing", C.c_float * 3)]


assert C.sizeof(SphMonitorConfig) == 24 and C.sizeof(SphMonitorRow) == 128 and C.sizeof(SphMonitorInfo) == 112
MONITOR_ROW_DTYPE = np.dtype(SphMonitorRow)
assert MONITOR_ROW_DTYPE.itemsize == 128
SPH_MAX_MONITORS = 4
SPH_MAX_MONITOR_POINTS = 4194304
SPH_MAX_MONITOR_HISTORY = 4096
SPH_MONITOR_NONE, SPH_MONITOR_POINTS, SPH_MONITOR_LATTICE = 0, 1, 2
(SPH_MONITOR_WET_SHARE, SPH_MONITOR_MEAN_FRACTION, SPH_MONITOR_VAR_FRACTION, SPH_MONITOR_MEAN_DENSITY, SPH_MONITOR_MEAN_PRESSURE,
 SPH_MONITOR_VAR_PRESSURE, SPH_MONITOR_MEAN_VEL_X, SPH_MONITOR_MEAN_VEL_Y, SPH_MONITOR_MEAN_VEL_Z, SPH_MONITOR_TKE) = range(10)
SPH_MONITOR_FIELDS = 10


class SphNeighborInfo(C.Structure):
    """struct SphNeighborInfo of include/sph_abi.h: what the engine's neighbour lists hold (see SPHFluidGPU.neighbors)."""
    _fields_ = [("rows", C.c_uint64), ("total", C.c_uint64), ("radius", C.c_float), ("stencil", C.c_int32), ("flags", C.c_int32),
                ("kind", C.c_int32), ("maxCount", C.c_uint32), ("pad", C.c_uint32)]


assert C.sizeof(SphNeighborInfo) == 40
SPH_NEIGHBORS_SELF, SPH_NEIGHBORS_HALF, SPH_NEIGHBORS_COUNT_ONLY = 1, 2, 4


class SphComponent(C.Structure):
    """struct SphComponent of include/sph_abi.h: one row of the table of connected bodies (see SPHFluidGPU.components)."""
    _fields_ = [("root", C.c_uint32), ("count", C.c_uint32), ("bbMin", C.c_float * 3), ("bbMax", C.c_float * 3), ("sumQ", C.c_int64 * 3),
                ("flags", C.c_uint32), ("pad", C.c_uint32)]


class SphComponentInfo(C.Structure):
    """struct SphComponentInfo of include/sph_abi.h: what the engine's components hold."""
    _fields_ = [("rows", C.c_uint64), ("numComponents", C.c_uint64), ("numExcluded", C.c_uint64), ("largestCount", C.c_uint64),
                ("largestRoot", C.c_uint32), ("numSingletons", C.c_uint32), ("radius", C.c_float), ("stencil", C.c_int32), ("flags", C.c_int32),
                ("rounds", C.c_uint32)]


assert C.sizeof(SphComponent) == 64 and C.sizeof(SphComponentInfo) == 56
COMPONENT_DTYPE = np.dtype(SphComponent)
assert COMPONENT_DTYPE.itemsize == 64
SPH_COMPONENTS_FLUID_ONLY = 1
SPH_COMPONENT_NONFINITE = 1


class SphKnnInfo(C.Structure):
    """struct SphKnnInfo of include/sph_abi.h: what the engine's k-nearest-neighbour rows hold (see SPHFluidGPU.knn)."""
    _fields_ = [("rows", C.c_uint64), ("total", C.c_uint64), ("rowsFull", C.c_uint64), ("radius", C.c_float), ("k", C.c_int32),
                ("stencil", C.c_int32), ("flags", C.c_int32), ("kind", C.c_int32), ("pad", C.c_int32)]


assert C.sizeof(SphKnnInfo) == 48
SPH_KNN_SELF, SPH_KNN_FLUID_ONLY, SPH_KNN_MAX_K = 1, 2, 64


class SphRayHit(C.Structure):
    """struct SphRayHit of include/sph_abi.h: what one ray met first (see SPHFluidGPU.raycast); a miss is (+inf, -1, zeros)."""
    _fields_ = [("t", C.c_float), ("id", C.c_int32), ("pos", C.c_float * 3), ("normal", C.c_float * 3)]


class SphRaysInfo(C.Structure):
    """struct SphRaysInfo of include/sph_abi.h: what the engine's ray hits hold."""
    _fields_ = [("rays", C.c_uint64), ("hits", C.c_uint64), ("voidRays", C.c_uint64), ("radius", C.c_float), ("flags", C.c_int32)]


assert C.sizeof(SphRayHit) == 32 and C.sizeof(SphRaysInfo) == 32
RAY_HIT_DTYPE = np.dtype(SphRayHit)
assert RAY_HIT_DTYPE.itemsize == 32
SPH_RAYS_FLUID_ONLY, SPH_RAYS_ANY_HIT = 1, 2


class SphRaySpan(C.Structure):
    """struct SphRaySpan of include/sph_abi.h: what one ray crosses in all (see SPHFluidGPU.ray_spans); nothing crossed is
    (+inf, -inf, -1, -1, 0)."""
    _fields_ = [("tEnter", C.c_float), ("tExit", C.c_float), ("idEnter", C.c_int32), ("idExit", C.c_int32), ("count", C.c_uint32),
                ("flags", C.c_uint32), ("length", C.c_uint64)]


class SphRaySpansInfo(C.Structure):
    """struct SphRaySpansInfo of include/sph_abi.h: what the engine's ray spans hold."""
    _fields_ = [("rays", C.c_uint64), ("crossed", C.c_uint64), ("voidRays", C.c_uint64), ("total", C.c_uint64), ("maxCount", C.c_uint32),
                ("radius", C.c_float), ("flags", C.c_int32), ("pad", C.c_uint32)]


assert C.sizeof(SphRaySpan) == 32 and C.sizeof(SphRaySpansInfo) == 48
RAY_SPAN_DTYPE = np.dtype(SphRaySpan)
assert RAY_SPAN_DTYPE.itemsize == 32


class SphShell(C.Structure):
    """struct SphShell of include/sph_abi.h: the free-surface record of one particle or query point (see SPHFluidGPU.shell)."""
    _fields_ = [("normal", C.c_float * 3), ("offsetRatio", C.c_float), ("crest", C.c_float), ("count", C.c_uint32), ("flags", C.c_uint32),
                ("pad", C.c_uint32)]


class SphShellConfig(C.Structure):
    """struct SphShellConfig of include/sph_abi.h: radius (<= 0: param_h), offset threshold, minCount, flags (see shell_config())."""
    _fields_ = [("radius", C.c_float), ("offset", C.c_float), ("minCount", C.c_uint32), ("flags", C.c_int32)]


class SphShellInfo(C.Structure):
    """struct SphShellInfo of include/sph_abi.h: what the engine's free-surface rows hold."""
    _fields_ = [("rows", C.c_uint64), ("numShell", C.c_uint64), ("numIsolated", C.c_uint64), ("maxCount", C.c_uint32), ("radius", C.c_float),
                ("stencil", C.c_int32), ("kind", C.c_int32), ("flags", C.c_int32), ("pad", C.c_uint32)]


assert C.sizeof(SphShell) == 32 and C.sizeof(SphShellConfig) == 16 and C.sizeof(SphShellInfo) == 48
SHELL_DTYPE = np.dtype(SphShell)
assert SHELL_DTYPE.itemsize == 32
SPH_SHELL_FLUID_ONLY = 1
SPH_SHELL_MEMBER, SPH_SHELL_ISOLATED = 1, 2


class SphAniso(C.Structure):
    """struct SphAniso of include/sph_abi.h: the smoothed centre and the ellipsoid of one particle (see SPHFluidGPU.anisotropy)."""
    _fields_ = [("center", C.c_float * 3), ("count", C.c_uint32), ("axis0", C.c_float * 3), ("flags", C.c_uint32), ("axis1", C.c_float * 3),
                ("reach", C.c_float), ("axis2", C.c_float * 3), ("amplitude", C.c_float)]


class SphAnisoConfig(C.Structure):
    """struct SphAnisoConfig of include/sph_abi.h: radius (<= 0: 2 param_h), support (<= 0: param_h), smoothing, maxRatio, maxStretch,
    sparseScale, minCount, flags (see aniso_config())."""
    _fields_ = [("radius", C.c_float), ("support", C.c_float), ("smoothing", C.c_float), ("maxRatio", C.c_float), ("maxStretch", C.c_float),
                ("sparseScale", C.c_float), ("minCount", C.c_uint32), ("flags", C.c_int32)]


class SphAnisoInfo(C.Structure):
    """struct SphAnisoInfo of include/sph_abi.h: what the engine's anisotropy rows hold."""
    _fields_ = [("rows", C.c_uint64), ("numSparse", C.c_uint64), ("numClamped", C.c_uint64), ("maxCount", C.c_uint32), ("radius", C.c_float),
                ("support", C.c_float), ("stencil", C.c_int32), ("maxReach", C.c_float), ("reachStencil", C.c_int32), ("kind", C.c_int32),
                ("flags", C.c_int32)]


assert C.sizeof(SphAniso) == 64 and C.sizeof(SphAnisoConfig) == 32 and C.sizeof(SphAnisoInfo) == 56
ANISO_DTYPE = np.dtype(SphAniso)
assert ANISO_DTYPE.itemsize == 64
SPH_ANISO_FLUID_ONLY = 1
SPH_ANISO_VALID, SPH_ANISO_SPARSE, SPH_ANISO_CLAMPED = 1, 2, 4


class SphAggregateConfig(C.Structure):
    """struct SphAggregateConfig of include/sph_abi.h: radius, op, weight, flags, channels, zero padding (see aggregate_config())."""
    _fields_ = [("radius", C.c_float), ("op", C.c_int32), ("weight", C.c_int32), ("flags", C.c_int32), ("channels", C.c_int32), ("pad", C.c_int32 * 3)]


class SphAggregateInfo(C.Structure):
    """struct SphAggregateInfo of include/sph_abi.h: what one neighbourhood reduction wrote."""
    _fields_ = [("rows", C.c_uint64), ("channels", C.c_int32), ("planes", C.c_int32), ("stencil", C.c_int32), ("flags", C.c_int32),
                ("radius", C.c_float), ("pad", C.c_int32)]


assert C.sizeof(SphAggregateConfig) == 32 and C.sizeof(SphAggregateInfo) == 32
SPH_AGGREGATE_SUM, SPH_AGGREGATE_MEAN, SPH_AGGREGATE_MAX, SPH_AGGREGATE_MIN = 0, 1, 2, 3
SPH_AGGREGATE_WEIGHT_ONE, SPH_AGGREGATE_WEIGHT_POLY6 = 0, 1
SPH_AGGREGATE_SELF, SPH_AGGREGATE_FLUID_ONLY, SPH_AGGREGATE_DELTA, SPH_AGGREGATE_MOMENTS = 1, 2, 4, 8
SPH_AGGREGATE_MAX_CHANNELS = 128
AGGREGATE_OPS = {"sum": SPH_AGGREGATE_SUM, "mean": SPH_AGGREGATE_MEAN, "max": SPH_AGGREGATE_MAX, "min": SPH_AGGREGATE_MIN}
AGGREGATE_WEIGHTS = {"one": SPH_AGGREGATE_WEIGHT_ONE, "poly6": SPH_AGGREGATE_WEIGHT_POLY6}


class SphBasisConfig(C.Structure):
    """struct SphBasisConfig of include/sph_abi.h: radius, weight, flags, channels, kind, size, zero padding (see basis_config())."""
    _fields_ = [("radius", C.c_float), ("weight", C.c_int32), ("flags", C.c_int32), ("channels", C.c_int32), ("kind", C.c_int32), ("size", C.c_int32),
                ("pad", C.c_int32 * 2)]


assert C.sizeof(SphBasisConfig) == 32
SPH_BASIS_GRID = 0


class SphSlabIntent(C.Structure):
    """The plan of one sized halo exchange (include/sph_abi.h SphSlabIntent): what both ends of a link must agree on before a record moves."""
    _fields_ = [("magic", C.c_uint32), ("exchangeNo", C.c_uint32), ("stepNo", C.c_uint32), ("faceCap", C.c_uint32),
                ("sendHalo", C.c_uint32 * 2), ("sendMig", C.c_uint32 * 2), ("recvHalo", C.c_uint32 * 2), ("recvMig", C.c_uint32 * 2),
                ("holdEvents", C.c_uint32), ("paramsHash", C.c_uint32), ("flags", C.c_uint32), ("zRange", C.c_uint32)]


assert C.sizeof(SphSlabIntent) == 64
# bits of the z-slab exchange's flag word (sph_slab_status out[4]); all but LAYER_JUMP, a notice, mean that records were lost
SPH_SLAB_FLAG_SEND_OVERFLOW, SPH_SLAB_FLAG_SLOT_OVERFLOW, SPH_SLAB_FLAG_BAD_HEADER, SPH_SLAB_FLAG_TRUNCATED = 1, 2, 4, 8
SPH_SLAB_FLAG_LAYER_JUMP, SPH_SLAB_FLAG_SIZE_MISMATCH = 16, 32
KERNEL_CLASSES = ("bin", "scan", "scatter", "sph", "writeback", "impulse", "other")     # SPH_K_* of "measurement"


# ---- checkpoints (include/sph_abi.h "checkpoints"): the records the library fills, and the blob's header and table entry -----
SPH_STATE_FORMAT = 1
SPH_STATE_CHECKSUM_MIX64 = 1
SPH_STATE_MAGIC = 0x4554415453485053                                       # "SPHSTATE"
STATE_SECTIONS = ("core", "particles", "tracers", "diffuse", "scalars", "obstacles", "gates", "monitors")   # the section with tag 1 << i


class SphStateInfo(C.Structure):
    _fields_ = [("formatVersion", C.c_uint32), ("abiVersion", C.c_uint32), ("checksumKind", C.c_uint32), ("sections", C.c_uint32),
                ("n", C.c_uint64), ("totalBytes", C.c_uint64), ("params", SphParams), ("pad", C.c_uint32),
                ("version", C.c_uint32 * len(STATE_SECTIONS)), ("offset", C.c_uint64 * len(STATE_SECTIONS)),
                ("bytes", C.c_uint64 * len(STATE_SECTIONS)), ("sum", (C.c_uint64 * 2) * len(STATE_SECTIONS)),
                ("terrainCount", C.c_uint64), ("terrainOffset", C.c_uint64), ("stencilCount", C.c_uint64)]


class SphStateDigest(C.Structure):
    _fields_ = [("sections", C.c_uint32), ("pad", C.c_uint32), ("sum", (C.c_uint64 * 2) * len(STATE_SECTIONS))]


class SphStateHeader(C.Structure):
    """The first 256 bytes of a blob."""
    _fields_ = [("magic", C.c_uint64), ("format", C.c_uint32), ("abi", C.c_uint32), ("checksumKind", C.c_uint32), ("sectionCount", C.c_uint32),
                ("n", C.c_uint64), ("totalBytes", C.c_uint64), ("sectionMask", C.c_uint32), ("headerBytes", C.c_uint32),
                ("params", SphParams), ("zero", C.c_ubyte * (240 - 48 - C.sizeof(SphParams))), ("sum", C.c_uint64 * 2)]


class SphStateEntry(C.Structure):
    """One entry of a blob's section table."""
    _fields_ = [("tag", C.c_uint32), ("version", C.c_uint32), ("offset", C.c_uint64), ("bytes", C.c_uint64), ("sum", C.c_uint64 * 2)]


class SphStateCore(C.Structure):
    """The record the core section opens with; the heightfield and the stencil targets follow it."""
    _fields_ = [("params", SphParams), ("lastDt", C.c_float), ("fountain", SphFountain), ("river", SphRiver),
                ("terrainCount", C.c_uint64), ("stencilCount", C.c_uint64)]


assert C.sizeof(SphStateCore) == 280
STATE_HEADER_DTYPE = np.dtype(SphStateHeader)
STATE_ENTRY_DTYPE = np.dtype(SphStateEntry)
assert STATE_HEADER_DTYPE.itemsize == 256 and STATE_ENTRY_DTYPE.itemsize == 40 and STATE_HEADER_DTYPE.fields["sum"][1] == 240


# ---- the C-ABI: every function include/sph_abi.h declares, in its order, as name -> (restype, argtypes) -------------------
# The one statement of the binding: ABI_SYMBOLS and load_library() derive from it, tests/test_abi.py holds it against the header's
# prototypes.  A record that only passes through (particles, samples, tracers, obstacles ...) crosses as c_void_p.
_int, _f, _d, _sz, _u32, _u64, _vp = C.c_int, C.c_float, C.c_double, C.c_size_t, C.c_uint32, C.c_uint64, C.c_void_p
_P = C.POINTER
_pf, _pi, _pp, _gp = _P(_f), _P(_int), _P(SphParams), _P(SphGridInfo)
_ABI = {
    # host-only helpers (no device needed)
    "sph_abi_version": (_int, []),
    "sph_params_default": (_int, [_pp]),
    "sph_rotation_mat3": (_int, [_pf, _pf]),
    "sph_effective_half": (_int, [_pp, _pf]),
    "sph_compute_grid_extents": (_int, [_pp, _gp]),
    "sph_spawn_particles": (_int, [_pp, _sz, _u32, _vp, _P(_sz), _pf]),
    "sph_last_error": (C.c_char_p, []),
    # lifetime
    "sph_create": (_int, [_P(_vp), _sz, _pp, _u32, _vp]),
    "sph_create_from_particles": (_int, [_P(_vp), _vp, _sz, _pp, _vp]),
    "sph_destroy": (_int, [_vp]),
    "sph_reset": (_int, [_vp, _sz, _u32]),
    # parameters
    "sph_set_params": (_int, [_vp, _pp]),
    "sph_get_params": (_int, [_vp, _pp]),
    "sph_set_option": (_int, [_vp, _int, _int]),
    "sph_get_option": (_int, [_vp, _int, _pi]),
    # the hot path
    "sph_dispatch": (_int, [_vp, _f]),
    "sph_dispatch_n": (_int, [_vp, _f, _int]),
    "sph_apply_wave_impulse": (_int, [_vp, _f, _f, _f, _pf, _f, _f]),
    "sph_apply_vortex_impulse": (_int, [_vp, _f, _f]),
    "sph_apply_attractor_impulse": (_int, [_vp, _pf, _f, _f]),
    "sph_set_stencil_targets": (_int, [_vp, _vp, _sz]),
    "sph_apply_stencil_attract": (_int, [_vp, _f, _f]),
    "sph_apply_curl_flow": (_int, [_vp, _f, _f, _f]),
    "sph_fountain_default": (None, [_P(SphFountain)]),
    "sph_set_fountain": (_int, [_vp, _P(SphFountain)]),
    "sph_get_fountain": (_int, [_vp, _P(SphFountain)]),
    "sph_river_default": (None, [_P(SphRiver)]),
    "sph_generate_river_terrain": (_int, [_pp, _int, _P(SphRiver), _vp]),
    "sph_spawn_river_particles": (_int, [_pp, _P(SphRiver), _vp, _sz, _u32, _vp, _P(_sz), _pf]),
    "sph_set_river": (_int, [_vp, _P(SphRiver), _vp]),
    "sph_get_river": (_int, [_vp, _P(SphRiver)]),
    # data
    "sph_num_particles": (_sz, [_vp]),
    "sph_grid_info": (_int, [_vp, _gp]),
    "sph_upload_particles": (_int, [_vp, _vp, _sz]),
    "sph_download_particles": (_int, [_vp, _vp, _sz]),
    "sph_device_particles": (_int, [_vp, _P(_vp)]),
    "sph_pack_render_buffer": (_int, [_vp, _vp, _sz, _int]),
    "sph_initial_particles": (_int, [_vp, _vp, _sz]),
    "sph_download_grid": (_int, [_vp, _vp, _sz, _vp, _sz]),
    "sph_sync": (_int, [_vp]),
    "sph_debug_counters": (_int, [_vp, _P(_u64), _int, _int]),
    # field sampling
    "sph_sample_points": (_int, [_vp, _vp, _sz, _vp]),
    "sph_sample_points_device": (_int, [_vp, _vp, _sz, _vp]),
    "sph_sample_lattice": (_int, [_vp, _pf, _pf, _pi, _int, _vp]),
    # iso-surface
    "sph_extract_surface": (_int, [_vp, _pf, _pf, _pi, _int, _f, _P(SphSurface)]),
    "sph_extract_surface_volume": (_int, [_vp, _vp, _pf, _pf, _pi, _f, _P(SphSurface)]),
    "sph_surface_download": (_int, [_vp, _vp, _sz, _vp, _sz]),
    # statistics
    "sph_statistics": (_int, [_vp, _vp, _vp, _int, _vp]),
    "sph_statistics_device": (_int, [_vp, _vp, _vp, _int, _vp]),
    # passive tracers
    "sph_tracers_set": (_int, [_vp, _vp, _sz, _int, _u32, _u32]),
    "sph_tracers_set_device": (_int, [_vp, _vp, _sz, _int, _u32, _u32]),
    "sph_tracers_count": (_sz, [_vp]),
    "sph_tracers_info": (_int, [_vp, _P(_u64), _P(_u32), _P(_u64)]),
    "sph_tracers_download": (_int, [_vp, _vp, _sz]),
    "sph_tracers_device": (_int, [_vp, _P(_vp)]),
    "sph_tracers_history": (_int, [_vp, _vp, _sz, _P(_u32), _P(_u64)]),
    # diffusing scalar fields
    "sph_scalars_set": (_int, [_vp, _vp, _sz, _int, _pf]),
    "sph_scalars_set_device": (_int, [_vp, _vp, _sz, _int, _pf]),
    "sph_scalars_set_coefficients": (_int, [_vp, _pf]),
    "sph_scalars_channels": (_int, [_vp]),
    "sph_scalars_download": (_int, [_vp, _vp, _sz]),
    "sph_scalars_device": (_int, [_vp, _P(_vp)]),
    "sph_scalars_paint": (_int, [_vp, _pf, _f, _int, _f, _int]),
    "sph_scalars_info": (_int, [_vp, _P(_u64), _pf]),
    "sph_scalars_moments": (_int, [_vp, _vp]),
    "sph_scalars_sample_points": (_int, [_vp, _vp, _sz, _int, _vp]),
    "sph_scalars_sample_points_device": (_int, [_vp, _vp, _sz, _int, _vp]),
    "sph_scalars_sample_lattice": (_int, [_vp, _pf, _pf, _pi, _int, _vp]),
    "sph_scalars_step_host": (_int, [_vp, _sz, _pp, _f, _vp, _int, _pf, _pf]),
    # kinematic solid obstacles
    "sph_obstacle_default": (None, [_vp]),
    "sph_obstacles_set": (_int, [_vp, _vp, _int]),
    "sph_obstacles_set_motion": (_int, [_vp, _int, _pf, _pf]),
    "sph_obstacles_get": (_int, [_vp, _vp, _int, _pi]),
    "sph_obstacles_impulses": (_int, [_vp, _vp, _int, _P(_d), _P(_u64), _int]),
    "sph_obstacles_apply_host": (_int, [_vp, _int, _f, _vp, _sz, _vp]),
    "sph_obstacles_advance_host": (_int, [_vp, _int, _f]),
    # triangle-mesh obstacles through signed distance lattices
    "sph_volume_create": (_int, [_vp, _vp, _pi, _pf, _int, _pi]),
    "sph_volume_destroy": (_int, [_vp, _int]),
    "sph_volume_info": (_int, [_vp, _int, _pi, _pf, _pf]),
    "sph_obstacles_bind_volume": (_int, [_vp, _int, _int]),
    "sph_obstacles_volume": (_int, [_vp, _int, _pi]),
    "sph_volume_sample_host": (_int, [_vp, _pi, _pf, _pf, _pf, _pf, _pi]),
    "sph_obstacles_apply_host_volumes": (_int, [_vp, _int, _vp, _int, _vp, _f, _vp, _sz, _vp]),
    "sph_mesh_distance": (_int, [_vp, _vp, _sz, _vp, _sz, _pf, _pf, _pi, _vp]),
    "sph_volume_from_mesh": (_int, [_vp, _vp, _sz, _vp, _sz, _pf, _pf, _pi, _pi]),
    "sph_mesh_distance_host": (_int, [_vp, _sz, _vp, _sz, _pf, _pf, _pi, _vp]),
    # dynamic rigid bodies
    "sph_obstacle_dynamics_default": (None, [_vp]),
    "sph_obstacles_set_dynamics": (_int, [_vp, _int, _vp]),
    "sph_obstacles_get_dynamics": (_int, [_vp, _int, _vp, _pi]),
    "sph_obstacles_step_host": (_int, [_vp, _vp, _int, _vp, _pp, _f]),
    "sph_volume_moments": (_int, [_vp, _int, _vp]),
    "sph_volume_moments_host": (_int, [_vp, _pi, _pf, _vp]),
    # active scalars: buoyancy and continuous sources
    "sph_scalars_set_buoyancy": (_int, [_vp, _pf, _pf]),
    "sph_scalars_get_buoyancy": (_int, [_vp, _pf, _pf]),
    "sph_scalar_source_default": (None, [_vp]),
    "sph_scalars_set_sources": (_int, [_vp, _vp, _int]),
    "sph_scalars_get_sources": (_int, [_vp, _vp, _int, _pi]),
    "sph_scalars_injected": (_int, [_vp, _vp, _vp, _int, _P(_d), _P(_u64), _int]),
    "sph_scalars_couple_host": (_int, [_vp, _sz, _pp, _f, _vp, _int, _pf, _pf, _vp, _int, _vp, _int, _vp, _vp]),
    # flow gates
    "sph_gates_set": (_int, [_vp, _vp, _int, _u32, _u32]),
    "sph_gates_get": (_int, [_vp, _vp, _int, _pi, _P(_u32), _P(_u32)]),
    "sph_gates_books": (_int, [_vp, _vp, _P(_d), _P(_u64), _int]),
    "sph_gates_history": (_int, [_vp, _P(_u64), _P(_u32), _vp, _vp]),
    "sph_gates_step_host": (_int, [_vp, _vp, _sz, _vp, _int, _vp, _int, _vp]),
    # field monitors
    "sph_monitor_config_default": (None, [_P(SphMonitorConfig)]),
    "sph_monitor_set": (_int, [_vp, _int, _vp, _sz, _P(SphMonitorConfig)]),
    "sph_monitor_set_device": (_int, [_vp, _int, _vp, _sz, _P(SphMonitorConfig)]),
    "sph_monitor_set_lattice": (_int, [_vp, _int, _pf, _pf, _pi, _P(SphMonitorConfig)]),
    "sph_monitor_info": (_int, [_vp, _int, _P(SphMonitorInfo)]),
    "sph_monitor_download": (_int, [_vp, _int, _vp, _sz]),
    "sph_monitor_device": (_int, [_vp, _int, _P(_vp)]),
    "sph_monitor_history": (_int, [_vp, _int, _P(_u64), _P(_u32), _vp, _vp, _sz]),
    "sph_monitor_field": (_int, [_vp, _int, _int, _vp]),
    "sph_monitor_reset": (_int, [_vp, _int]),
    "sph_monitor_clear": (_int, [_vp, _int]),
    "sph_monitor_accumulate_host": (_int, [_vp, _vp, _sz, _f]),
    "sph_monitor_field_host": (_int, [_vp, _sz, _int, _vp]),
    "sph_monitor_schedule_host": (_int, [_u32, _u32, _u32, _sz, _vp, _vp]),
    # spray, foam and bubbles
    "sph_diffuse_default": (None, [_P(SphDiffuseConfig)]),
    "sph_diffuse_set": (_int, [_vp, _P(SphDiffuseConfig)]),
    "sph_diffuse_get": (_int, [_vp, _P(SphDiffuseConfig)]),
    "sph_diffuse_info": (_int, [_vp, _P(SphDiffuseInfo)]),
    "sph_diffuse_download": (_int, [_vp, _vp, _sz, _P(_sz)]),
    "sph_diffuse_device": (_int, [_vp, _P(_vp), _P(_vp)]),
    "sph_diffuse_seed": (_int, [_vp, _vp, _sz]),
    "sph_diffuse_step_host": (_int, [_P(SphDiffuseConfig), _pp, _f, _u64, _vp, _sz, _vp, _vp, _sz, _vp, _P(_sz), _P(SphDiffuseInfo)]),
    "sph_diffuse_crest_default": (None, [_P(SphDiffuseCrest)]),
    "sph_diffuse_set_crest": (_int, [_vp, _P(SphDiffuseCrest)]),
    "sph_diffuse_get_crest": (_int, [_vp, _P(SphDiffuseCrest)]),
    "sph_diffuse_crest_info": (_int, [_vp, _P(SphDiffuseCrestInfo)]),
    "sph_diffuse_step_host_crest": (_int, [_P(SphDiffuseConfig), _P(SphDiffuseCrest), _pp, _f, _u64, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _P(_sz),
                                           _P(SphDiffuseInfo), _P(SphDiffuseCrestInfo)]),
    # neighbour lists
    "sph_neighbors_build": (_int, [_vp, _f, _int, _u64, _P(SphNeighborInfo)]),
    "sph_neighbors_query": (_int, [_vp, _vp, _sz, _f, _int, _u64, _P(SphNeighborInfo)]),
    "sph_neighbors_info": (_int, [_vp, _P(SphNeighborInfo)]),
    "sph_neighbors_device": (_int, [_vp, _P(_vp), _P(_vp)]),
    "sph_neighbors_export": (_int, [_vp, _vp, _vp, _u64]),
    "sph_neighbors_download": (_int, [_vp, _vp, _vp, _u64]),
    "sph_neighbors_host": (_int, [_vp, _sz, _pp, _vp, _sz, _f, _int, _vp, _vp, _u64, _P(SphNeighborInfo)]),
    # connected components
    "sph_components_build": (_int, [_vp, _f, _int, _P(SphComponentInfo)]),
    "sph_components_info": (_int, [_vp, _P(SphComponentInfo)]),
    "sph_components_device": (_int, [_vp, _P(_vp), _P(_vp), _P(_vp)]),
    "sph_components_download": (_int, [_vp, _vp, _vp, _vp, _u64]),
    "sph_components_host": (_int, [_vp, _sz, _pp, _f, _int, _vp, _vp, _vp, _u64, _P(SphComponentInfo)]),
    # k nearest neighbours
    "sph_knn_build": (_int, [_vp, _int, _f, _int, _P(SphKnnInfo)]),
    "sph_knn_query": (_int, [_vp, _vp, _sz, _int, _f, _int, _P(SphKnnInfo)]),
    "sph_knn_info": (_int, [_vp, _P(SphKnnInfo)]),
    "sph_knn_device": (_int, [_vp, _P(_vp), _P(_vp), _P(_vp)]),
    "sph_knn_download": (_int, [_vp, _vp, _vp, _vp]),
    "sph_knn_host": (_int, [_vp, _sz, _pp, _vp, _sz, _int, _f, _int, _vp, _vp, _vp, _P(SphKnnInfo)]),
    "sph_rays_cast": (_int, [_vp, _vp, _sz, _f, _int, _P(SphRaysInfo)]),
    "sph_rays_cast_device": (_int, [_vp, _vp, _sz, _f, _int, _P(SphRaysInfo)]),
    "sph_rays_info": (_int, [_vp, _P(SphRaysInfo)]),
    "sph_rays_device": (_int, [_vp, _P(_vp)]),
    "sph_rays_download": (_int, [_vp, _vp]),
    "sph_rays_host": (_int, [_vp, _sz, _pp, _vp, _sz, _f, _int, _vp, _P(SphRaysInfo)]),
    "sph_rays_walk_host": (_int, [_vp, _sz, _pp, _vp, _sz, _f, _int, _vp, _P(SphRaysInfo)]),
    "sph_rays_span": (_int, [_vp, _vp, _sz, _f, _int, _P(SphRaySpansInfo)]),
    "sph_rays_span_device": (_int, [_vp, _vp, _sz, _f, _int, _P(SphRaySpansInfo)]),
    "sph_rays_span_info": (_int, [_vp, _P(SphRaySpansInfo)]),
    "sph_rays_span_rows": (_int, [_vp, _P(_vp)]),
    "sph_rays_span_download": (_int, [_vp, _vp]),
    "sph_rays_span_host": (_int, [_vp, _sz, _pp, _vp, _sz, _f, _int, _vp, _P(SphRaySpansInfo)]),
    "sph_rays_span_walk_host": (_int, [_vp, _sz, _pp, _vp, _sz, _f, _int, _int, _vp, _P(SphRaySpansInfo)]),
    # free-surface particles
    "sph_shell_default": (None, [_P(SphShellConfig)]),
    "sph_shell_build": (_int, [_vp, _P(SphShellConfig), _P(SphShellInfo)]),
    "sph_shell_query": (_int, [_vp, _vp, _sz, _P(SphShellConfig), _P(SphShellInfo)]),
    "sph_shell_info": (_int, [_vp, _P(SphShellInfo)]),
    "sph_shell_device": (_int, [_vp, _P(_vp), _P(_vp)]),
    "sph_shell_download": (_int, [_vp, _vp, _vp]),
    "sph_shell_host": (_int, [_vp, _sz, _pp, _vp, _sz, _P(SphShellConfig), _vp, _vp, _vp, _P(SphShellInfo)]),
    # anisotropic kernels
    "sph_aniso_default": (None, [_P(SphAnisoConfig)]),
    "sph_aniso_build": (_int, [_vp, _P(SphAnisoConfig), _P(SphAnisoInfo)]),
    "sph_aniso_info": (_int, [_vp, _P(SphAnisoInfo)]),
    "sph_aniso_device": (_int, [_vp, _P(_vp)]),
    "sph_aniso_download": (_int, [_vp, _vp]),
    "sph_aniso_lattice": (_int, [_vp, _P(SphAnisoConfig), _pf, _pf, _pi, _vp, _P(SphAnisoInfo)]),
    "sph_aniso_surface": (_int, [_vp, _P(SphAnisoConfig), _pf, _pf, _pi, _f, _P(SphSurface), _P(SphAnisoInfo)]),
    "sph_aniso_host": (_int, [_vp, _sz, _pp, _P(SphAnisoConfig), _vp, _P(SphAnisoInfo)]),
    "sph_aniso_lattice_host": (_int, [_vp, _sz, _pp, _P(SphAnisoConfig), _pf, _pf, _pi, _vp, _P(SphAnisoInfo)]),
    # fused neighbourhood reductions of caller tensors
    "sph_aggregate_default": (None, [_P(SphAggregateConfig)]),
    "sph_aggregate_particles": (_int, [_vp, _P(SphAggregateConfig), _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_query": (_int, [_vp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_staged": (_int, [_vp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_host": (_int, [_vp, _sz, _pp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _vp]),
    "sph_aggregate_adjoint_particles": (_int, [_vp, _P(SphAggregateConfig), _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_adjoint_query": (_int, [_vp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_adjoint_staged": (_int, [_vp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_adjoint_host": (_int, [_vp, _sz, _pp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp]),
    "sph_aggregate_arg_particles": (_int, [_vp, _P(SphAggregateConfig), _vp, _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_arg_query": (_int, [_vp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_arg_host": (_int, [_vp, _sz, _pp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _vp, _vp]),
    "sph_aggregate_route_particles": (_int, [_vp, _P(SphAggregateConfig), _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_route_query": (_int, [_vp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_route_host": (_int, [_vp, _sz, _pp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _vp]),
    "sph_aggregate_basis_default": (None, [_P(SphBasisConfig)]),
    "sph_aggregate_basis_particles": (_int, [_vp, _P(SphBasisConfig), _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_basis_query": (_int, [_vp, _P(SphBasisConfig), _vp, _sz, _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_basis_staged": (_int, [_vp, _P(SphBasisConfig), _vp, _sz, _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_basis_host": (_int, [_vp, _sz, _pp, _P(SphBasisConfig), _vp, _sz, _vp, _vp, _vp]),
    "sph_aggregate_basis_adjoint_particles": (_int, [_vp, _P(SphBasisConfig), _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_basis_adjoint_query": (_int, [_vp, _P(SphBasisConfig), _vp, _sz, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_basis_adjoint_staged": (_int, [_vp, _P(SphBasisConfig), _vp, _sz, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_basis_adjoint_host": (_int, [_vp, _sz, _pp, _P(SphBasisConfig), _vp, _sz, _vp, _vp]),
    "sph_aggregate_posgrad_particles": (_int, [_vp, _P(SphAggregateConfig), _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_posgrad_query": (_int, [_vp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_posgrad_staged": (_int, [_vp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_posgrad_host": (_int, [_vp, _sz, _pp, _P(SphAggregateConfig), _vp, _sz, _vp, _vp, _vp, _vp]),
    "sph_aggregate_basis_posgrad_particles": (_int, [_vp, _P(SphBasisConfig), _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_basis_posgrad_query": (_int, [_vp, _P(SphBasisConfig), _vp, _sz, _vp, _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_basis_posgrad_staged": (_int, [_vp, _P(SphBasisConfig), _vp, _sz, _vp, _vp, _vp, _vp, _P(SphAggregateInfo)]),
    "sph_aggregate_basis_posgrad_host": (_int, [_vp, _sz, _pp, _P(SphBasisConfig), _vp, _sz, _vp, _vp, _vp, _vp]),
    # multi-GPU: z-slab decomposition
    "sph_create_slab": (_int, [_P(_vp), _vp, _vp, _sz, _pp, _int, _int, _int, _int, _sz, _vp]),
    "sph_slab_pack": (_int, [_vp, _vp, _vp, _u32, _u32, _P(_u32)]),
    "sph_slab_unpack": (_int, [_vp, _vp, _u32, _vp, _u32]),
    "sph_slab_download": (_int, [_vp, _vp, _sz, _P(_sz)]),
    # the same exchange without host round trips, and its RCCL transport
    "sph_slab_alloc_faces": (_int, [_vp, _u32]),
    "sph_slab_face_buffer": (_int, [_vp, _int, _P(_vp)]),
    "sph_slab_face_bytes": (_int, [_vp, _P(_u64)]),
    "sph_slab_pack_async": (_int, [_vp]),
    "sph_slab_unpack_async": (_int, [_vp, _vp, _vp, _u32]),
    "sph_slab_status": (_int, [_vp, _P(_u32)]),
    "sph_slab_clear_flags": (_int, [_vp, _u32]),
    "sph_slab_message_bytes": (_int, [_vp, _P(_u64)]),
    "sph_slab_message_records": (_int, [_u32, _u32, _u32]),
    "sph_comm_unique_id": (_int, [_vp]),
    "sph_comm_create": (_int, [_P(_vp), _vp, _int, _int]),
    "sph_comm_destroy": (_int, [_vp]),
    "sph_comm_selftest": (_int, [_vp, _u64]),
    "sph_comm_selftest_timed": (_int, [_vp, _u64, _pf]),
    "sph_slab_exchange": (_int, [_vp, _vp]),
    # agreement of the two ends of a link
    "sph_slab_set_verify": (_int, [_vp, _int]),
    "sph_slab_set_deadline": (_int, [_vp, _d]),
    "sph_slab_plan": (_int, [_vp, _P(SphSlabIntent), _pf]),
    "sph_slab_plans_agree": (_int, [_P(SphSlabIntent), _P(SphSlabIntent), _int, C.c_char_p, _sz]),
    "sph_sync_deadline": (_int, [_vp, _d]),
    "sph_slab_debug_tight_messages": (_int, [_vp, _int]),
    "sph_comm_selftest_faces": (_int, [_vp, _u32, _P(_u32), _pf]),
    # boundary-first substep
    "sph_slab_step_begin": (_int, [_vp, _f]),
    "sph_slab_step_finish": (_int, [_vp, _vp]),
    "sph_slab_step_finish_local": (_int, [_vp, _vp, _vp]),
    "sph_slab_step_times": (_int, [_vp, _pf]),
    # measurement
    "sph_kernel_times": (_int, [_vp, _P(_d), _P(C.c_int64), _int]),
    # checkpoints
    "sph_state_size": (_int, [_vp, _P(_sz)]),
    "sph_state_save": (_int, [_vp, _vp, _sz, _P(_sz)]),
    "sph_state_load": (_int, [_vp, _vp, _sz]),
    "sph_state_peek": (_int, [_vp, _sz, _P(SphStateInfo)]),
    "sph_state_digest": (_int, [_vp, _u32, _P(SphStateDigest)]),
    "sph_state_checksum_host": (_int, [_vp, _sz, _P(_u64)]),
}
ABI_SYMBOLS = tuple(_ABI)


# ---- the loader -----------------------------------------------------------------------------------------------------------
class SphError(RuntimeError):
    pass


_lib = None


def lib_path() -> str:
    return _build.LIB_PATH


def load_library(build_if_missing: bool = True) -> C.CDLL:
    """Load libsph_hip.so (building it in-tree first if asked and needed)."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_missing:
        _build.build()
    if not os.path.exists(_build.LIB_PATH):
        raise SphError(f"{_build.LIB_PATH} is missing: run __graft_entry__.build(); there is no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same soname as the
    # system one).  Whichever loads first wins, and torch cannot see the GPU behind the system
    # runtime, so let torch load first when it is installed (it is only plumbing here: halo
    # buffers, streams, torch.distributed).
    if os.environ.get("SPH_NO_TORCH_PRELOAD", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    # developer A/B of kernel variants: SPH_HIP_LIB names another build of the same sources
    L = C.CDLL(os.environ.get("SPH_HIP_LIB") or _build.LIB_PATH)
    for name, (restype, argtypes) in _ABI.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


# ---- free helpers: errors and marshalling ---------------------------------------------------------------------------------
def _check(rc: int):
    if rc != 0:
        msg = load_library().sph_last_error()
        raise SphError(f"sph C-ABI error {rc}: {msg.decode() if msg else '?'}")


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _ptr(arr):
    """The data pointer of a numpy array (the caller keeps the array alive across the call)."""
    return arr.ctypes.data_as(C.c_void_p)


def _ptr_or_none(arr):
    return _ptr(arr) if len(arr) else None


def _dims3(dims, who=None):
    """(nx, ny, nz) as int[3]; with `who`, every dimension >= 1 and at most 2^31 - 1 points, or SphError in who's name."""
    d = (C.c_int * 3)(*[int(x) for x in dims])
    if who and (min(d) < 1 or int(d[0]) * int(d[1]) * int(d[2]) > 2 ** 31 - 1):
        raise SphError(f"{who}: bad dims {tuple(d)}")
    return d


def _spacing3(spacing):
    """A scalar or (sx, sy, sz) as 3 float32."""
    return np.broadcast_to(np.asarray(spacing, np.float32), (3,)).copy()


def _points4(points, who, keep_w):
    """(m, 3) or (m, 4) points as a fresh (m, 4) float32 array; the fourth column is the caller's (keep_w) or 0."""
    pts = np.asarray(points, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] not in (3, 4):
        raise SphError(f"{who}: points must have shape (m, 3) or (m, 4), not {pts.shape}")
    p4 = np.zeros((len(pts), 4), np.float32)
    k = pts.shape[1] if keep_w else 3
    p4[:, :k] = pts[:, :k]
    return p4


def _neighbor_flags(self_, half, count_only) -> int:
    return (SPH_NEIGHBORS_SELF if self_ else 0) | (SPH_NEIGHBORS_HALF if half else 0) | (SPH_NEIGHBORS_COUNT_ONLY if count_only else 0)


def _knn_flags(self_, fluid_only) -> int:
    return (SPH_KNN_SELF if self_ else 0) | (SPH_KNN_FLUID_ONLY if fluid_only else 0)


def _rays_flags(fluid_only, any_hit) -> int:
    return (SPH_RAYS_FLUID_ONLY if fluid_only else 0) | (SPH_RAYS_ANY_HIT if any_hit else 0)


def _rays8(rays, who):
    """(m, 8) rays (ox, oy, oz, tmin, dx, dy, dz, tmax) as a contiguous float32 array."""
    r = np.ascontiguousarray(rays, dtype=np.float32)
    if r.ndim != 2 or r.shape[1] != 8:
        raise SphError(f"{who}: rays must have shape (m, 8), not {r.shape}")
    return r


def _split_hits(hits):
    """A RAY_HIT_DTYPE array as (t, ids, pos, normal)."""
    return hits["t"].copy(), hits["id"].copy(), hits["pos"].copy(), hits["normal"].copy()


def _is_cuda_f32(t) -> bool:
    """A contiguous float32 torch CUDA tensor?"""
    return t.is_cuda and t.dtype == __import__("torch").float32 and t.is_contiguous()


def _device_points4(points, who):
    """Query points as a (m, 4) float32 torch device tensor: such a tensor is used in place, anything else is uploaded (_points4)."""
    import torch
    if isinstance(points, torch.Tensor) and _is_cuda_f32(points) and points.dim() == 2 and points.shape[1] == 4:
        return points
    return torch.from_numpy(_points4(points, who, keep_w=False)).cuda()


def _device_values(values, who):
    """Per-particle values as an (n, C) float32 torch device tensor: a contiguous float32 device tensor of (n, C) is used in place,
    anything else ((n,) or (n, C)) is uploaded."""
    import torch
    if isinstance(values, torch.Tensor) and _is_cuda_f32(values) and values.dim() == 2:
        return values
    return torch.from_numpy(_scalar_values(values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else values)).cuda()


def _planes(grad, rows, moments, who):
    """What a SUM's output looks like, as float32 numpy of (rows, C) or with moments (rows, 4, C); (rows,) counts as (rows, 1)."""
    g = np.ascontiguousarray(grad, np.float32)
    if g.ndim == 1 and not moments:
        g = g.reshape(-1, 1)
    if g.ndim != (3 if moments else 2) or len(g) != rows or (moments and g.shape[1] != 4):
        raise SphError(f"{who}: grad of shape {g.shape} for {rows} rows{' of 4 planes' if moments else ''}")
    return g


def _device_planes(grad, rows, moments, who):
    """The same as a torch device tensor: a contiguous float32 device tensor of the right shape is used in place, anything else uploaded."""
    import torch
    if isinstance(grad, torch.Tensor) and _is_cuda_f32(grad) and grad.dim() == (3 if moments else 2):
        if int(grad.shape[0]) != rows or (moments and int(grad.shape[1]) != 4):
            raise SphError(f"{who}: grad of shape {tuple(grad.shape)} for {rows} rows{' of 4 planes' if moments else ''}")
        return grad
    return torch.from_numpy(_planes(grad.detach().cpu().numpy() if isinstance(grad, torch.Tensor) else grad, rows, moments, who)).cuda()


def _tensor_ptr(t):
    """The address of a torch tensor's data, None for an empty one."""
    return C.c_void_p(t.data_ptr()) if t.numel() else None


def _fetch(call, device, specs, null_empty=True):
    """The results of a query, one fresh array per spec (shape, numpy dtype, name of the torch dtype), filled by one call(*pointers):
    numpy zeros, or with `device` torch.empty on the device (a spec without a torch dtype stays a numpy array).  A spec of None is no
    array: None and a null pointer; an empty array goes as a null pointer too, unless null_empty is False."""
    out, ptrs = [], []
    for spec in specs:
        arr = ptr = None
        if spec is not None and device and spec[2]:
            import torch
            arr = torch.empty(spec[0], dtype=getattr(torch, spec[2]), device="cuda")
            ptr = C.c_void_p(arr.data_ptr()) if arr.numel() or not null_empty else None
        elif spec is not None:
            arr = np.zeros(spec[0], spec[1])
            ptr = _ptr(arr) if arr.size or not null_empty else None
        out.append(arr)
        ptrs.append(ptr)
    _check(call(*ptrs))
    return tuple(out)


def _assign(struct, name, value):
    """struct.name = value, element by element where the field is an array."""
    cur = getattr(struct, name)
    if hasattr(cur, "__len__"):
        for i, x in enumerate(value):
            cur[i] = x
    else:
        setattr(struct, name, value)


def _volume_lattice(values, spacing):
    """A (nz, ny, nx) array of signed distances and its spacing -> (contiguous fp32 array, dims (nx, ny, nz), spacing[3])."""
    v = np.ascontiguousarray(values, np.float32)
    if v.ndim != 3:
        raise SphError(f"a volume needs an array of shape (nz, ny, nx), not {v.shape}")
    return v, _dims3(v.shape[::-1]), _spacing3(spacing)


def _mesh_arrays(vertices, triangles):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    return v, t


def _histogram_specs(histograms):
    """[(field, bins, lo, hi) | SphHistogramSpec, ...] -> (ctypes array or None, count, total uint64 slots).  Checked by the library."""
    hs = list(histograms or ())
    if not hs:
        return None, 0, 0
    arr = (SphHistogramSpec * len(hs))()
    for i, h in enumerate(hs):
        arr[i] = h if isinstance(h, SphHistogramSpec) else SphHistogramSpec(int(h[0]), int(h[1]), float(h[2]), float(h[3]))
    return arr, len(hs), sum(int(a.bins) + 2 for a in arr)


# ---- free helpers: records and results ------------------------------------------------------------------------------------
def _scalar_coeffs(channels: int, diffusivity, decay):
    """2 K float32: D_0 .. D_{K-1}, lambda_0 .. lambda_{K-1} (a scalar is every channel's value)."""
    k = int(channels)
    return np.concatenate([np.broadcast_to(np.asarray(diffusivity, np.float32), (k,)), np.broadcast_to(np.asarray(decay, np.float32), (k,))]).astype(np.float32)


def _scalar_values(values, n=None):
    """(n, K) float32 from (n,) or (n, K) values."""
    v = np.ascontiguousarray(values, np.float32)
    if v.ndim == 1:
        v = v.reshape(-1, 1)
    if v.ndim != 2 or (n is not None and len(v) != n):
        raise SphError(f"scalar values must have shape (n,) or (n, K){'' if n is None else f' with n = {n}'}, not {v.shape}")
    return v


class ScalarMoments:
    """sph_scalars_moments of one channel plus what follows from it.  Attributes: count, sum, sum_squares, min, max (value, id)."""

    def __init__(self, m: SphScalarMoments):
        self.count, self.sum, self.sum_squares = int(m.count), float(m.sum), float(m.sumSquares)
        self.min, self.max = (np.float32(m.min.value), int(m.min.id)), (np.float32(m.max.value), int(m.max.id))

    @property
    def mean(self) -> float:
        return self.sum / self.count if self.count else 0.0

    @property
    def variance(self) -> float:
        """sum_squares / count - mean^2, not below 0."""
        return max(self.sum_squares / self.count - self.mean ** 2, 0.0) if self.count else 0.0

    def mixing_index(self, initial_variance: float) -> float:
        """1 - variance / initial_variance: 0 for the unmixed state the variance was taken from, 1 when uniform."""
        return mixing_index(self.variance, initial_variance)


def mixing_index(variance: float, initial_variance: float) -> float:
    if not initial_variance > 0.0:
        raise SphError(f"mixing_index: the initial variance must be > 0, not {initial_variance}")
    return 1.0 - float(variance) / float(initial_variance)


class Statistics:
    """Result of SPHFluidGPU.statistics(): `s` is the SphStatistics struct (its members are also attributes of this object),
    `histograms` a list of uint64 arrays of bins + 2 slots (below lo, the bins, at or above hi) in spec order.  The derived numbers
    are computed here, on the host, from the struct and the members at the time of the call."""

    def __init__(self, s: SphStatistics, histograms, params: SphParams):
        self.s = s
        self.histograms = histograms
        self.mass, self.h, self.dt, self.rho0 = float(params.param_mass), float(params.param_h), float(params.param_timeStep), float(params.param_restDensity)
        self.gravity = (float(params.param_gravityX), float(params.param_gravityY), float(params.param_gravityZ))

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "s"), name)

    def tobytes(self) -> bytes:
        return bytes(self.s) + b"".join(h.tobytes() for h in self.histograms)

    @property
    def ok(self) -> bool:
        """No non-finite and no escaped fluid record."""
        return self.s.numNonFinite == 0 and self.s.numEscaped == 0

    @property
    def kinetic_energy(self) -> float:
        return 0.5 * self.mass * self.s.sumSpeed2

    @property
    def potential_energy(self) -> float:
        return -self.mass * sum(g * p for g, p in zip(self.gravity, self.s.sumPos))

    @property
    def momentum(self):
        return tuple(self.mass * v for v in self.s.sumVel)

    @property
    def angular_momentum(self):
        """About param_boxCenter."""
        return tuple(self.mass * v for v in self.s.sumAngular)

    @property
    def center_of_mass(self):
        n = self.s.numCounted
        return tuple(p / n for p in self.s.sumPos) if n else (0.0, 0.0, 0.0)

    @property
    def bounding_box(self):
        return tuple(e.value for e in self.s.minPos), tuple(e.value for e in self.s.maxPos)

    @property
    def mean_density(self) -> float:
        n = self.s.numCounted
        return self.s.sumDensity / n if n else 0.0

    @property
    def std_density(self) -> float:
        n = self.s.numCounted
        if not n:
            return 0.0
        m = self.s.sumDensity / n
        return max(self.s.sumDensity2 / n - m * m, 0.0) ** 0.5

    @property
    def cfl(self) -> float:
        return self.s.maxSpeed * self.dt / self.h

    @property
    def volume(self) -> float:
        """SPH volume sum(mass / rho_j)."""
        return self.mass * self.s.sumInvDensity


def scalar_source(shape, center, size, channel: int = 0, mode: int = SPH_SOURCE_RATE, rate: float = 0.0, target: float = 0.0,
                  body: int = -1) -> SphScalarSource:
    """One source: shape SPH_SOURCE_SPHERE (size = radius) or SPH_SOURCE_BOX (size = 3 half extents); centre in
    the world frame (body -1) or in the local frame of obstacle `body`; SPH_SOURCE_RATE adds rate per second, SPH_SOURCE_RELAX
    relaxes towards target at rate per second."""
    s = SphScalarSource()
    load_library().sph_scalar_source_default(C.byref(s))
    sz = [float(size)] * 3 if np.ndim(size) == 0 else [float(x) for x in size]
    ce = [float(x) for x in center]
    if len(sz) != 3 or len(ce) != 3:
        raise SphError("scalar_source: center and size need 3 components (size may be one number)")
    s.shape, s.channel, s.mode, s.body = int(shape), int(channel), int(mode), int(body)
    for i in range(3):
        s.center[i], s.size[i] = ce[i], sz[i]
    s.rate, s.target = float(rate), float(target)
    return s


def source_array(sources) -> np.ndarray:
    """A list of SphScalarSource, or a structured array, as a contiguous SOURCE_DTYPE array (the layout of SphScalarSource)."""
    if isinstance(sources, np.ndarray):
        return np.ascontiguousarray(sources, SOURCE_DTYPE)
    sources = list(sources or ())
    if not sources:
        return np.zeros(0, SOURCE_DTYPE)
    return np.frombuffer(b"".join(bytes(o) for o in sources), SOURCE_DTYPE).copy()


def gate(shape, center, u, v, unbounded: bool = False) -> SphGate:
    """One flow gate: SPH_GATE_RECT or SPH_GATE_ELLIPSE with centre `center` and the orthogonal half-extent
    vectors u and v; forward is cross(u, v).  unbounded: the whole plane counts, not only the patch."""
    g = SphGate()
    ce, uu, vv = ([float(x) for x in a] for a in (center, u, v))
    if len(ce) != 3 or len(uu) != 3 or len(vv) != 3:
        raise SphError("gate: center, u and v need 3 components")
    g.shape, g.flags = int(shape), SPH_GATE_UNBOUNDED if unbounded else 0
    for i in range(3):
        g.center[i], g.u[i], g.v[i] = ce[i], uu[i], vv[i]
    return g


def gate_box(center, half) -> list:
    """Six rectangles with outward normals around the axis-aligned box centre +- half: a control volume.  Order -x, +x, -y, +y, -z, +z;
    forward - backward summed over the six is the net outflow."""
    c = [float(x) for x in center]
    h = [float(half)] * 3 if np.ndim(half) == 0 else [float(x) for x in half]
    out = []
    for a in range(3):
        b, d = (a + 1) % 3, (a + 2) % 3
        for sign in (-1.0, 1.0):
            ce, u, v = list(c), [0.0] * 3, [0.0] * 3
            ce[a] += sign * h[a]
            u[b], v[d] = h[b], sign * h[d]                            # cross(e_b, e_d) = e_a
            out.append(gate(SPH_GATE_RECT, ce, u, v))
    return out


def gate_array(gates) -> np.ndarray:
    """A list of SphGate, or a structured array, as a contiguous GATE_DTYPE array (the layout of SphGate)."""
    if isinstance(gates, np.ndarray):
        return np.ascontiguousarray(gates, GATE_DTYPE)
    gates = list(gates or ())
    if not gates:
        return np.zeros(0, GATE_DTYPE)
    return np.frombuffer(b"".join(bytes(o) for o in gates), GATE_DTYPE).copy()


def gate_discharge(rows, time: float, params: SphParams) -> np.ndarray:
    """Net volume per unit time through each gate: (forward - backward) * param_mass / param_restDensity / time, from the rows of
    gate_books() or of one history row."""
    rows = np.asarray(rows)
    net = rows["forward"].astype(np.float64) - rows["backward"].astype(np.float64)
    return net * float(params.param_mass) / float(params.param_restDensity) / float(time)


def _buoyancy(channels: int, beta, ref):
    """(beta, ref) as two float32 arrays of K values (a scalar is every channel's value), or (None, None) for beta None."""
    if beta is None:
        return None, None
    k = int(channels)
    return (np.broadcast_to(np.asarray(beta, np.float32), (k,)).copy(), np.broadcast_to(np.asarray(0.0 if ref is None else ref, np.float32), (k,)).copy())


def obstacle(shape, center, size, rotation=(1.0, 0.0, 0.0, 0.0), vel=(0.0, 0.0, 0.0), omega=(0.0, 0.0, 0.0),
             restitution: float = 0.15, friction: float = 0.02) -> SphObstacle:
    """One body: shape SPH_OBSTACLE_*; size a number or up to 3 numbers (sphere: radius | box: half extents |
    capsule: radius, half length of the core segment along local y; the rest 0); rotation a quaternion (w, x, y, z), local -> world."""
    sz = [float(size)] if np.ndim(size) == 0 else [float(x) for x in size]
    if len(sz) > 3:
        raise SphError(f"obstacle: size has {len(sz)} components")
    o = SphObstacle()
    o.shape = int(shape)
    for i, x in enumerate(sz + [0.0] * (3 - len(sz))):
        o.size[i] = x
    for field, val, n in (("center", center, 3), ("rotation", rotation, 4), ("vel", vel, 3), ("omega", omega, 3)):
        arr = getattr(o, field)
        vals = [float(x) for x in val]
        if len(vals) != n:
            raise SphError(f"obstacle: {field} needs {n} components, not {len(vals)}")
        for i, x in enumerate(vals):
            arr[i] = x
    o.restitution = float(restitution)
    o.friction = float(friction)
    return o


def obstacle_array(obstacles) -> np.ndarray:
    """A list of SphObstacle, or a structured array, as a contiguous OBSTACLE_DTYPE array (the layout of SphObstacle)."""
    if isinstance(obstacles, np.ndarray):
        return np.ascontiguousarray(obstacles, OBSTACLE_DTYPE)
    obstacles = list(obstacles)
    if not obstacles:
        return np.zeros(0, OBSTACLE_DTYPE)
    return np.frombuffer(b"".join(bytes(o) for o in obstacles), OBSTACLE_DTYPE).copy()


def dynamics(mass, inertia, com=(0.0, 0.0, 0.0), gravity_scale: float = 1.0, force=(0.0, 0.0, 0.0), torque=(0.0, 0.0, 0.0),
             linear_damping: float = 0.0, angular_damping: float = 0.0, confined: bool = True) -> SphObstacleDynamics:
    """One dynamics record.  inertia about the centre of mass in the body frame: 3 numbers (the diagonal),
    6 (xx, yy, zz, xy, xz, yz) or a symmetric 3 x 3 array."""
    I = np.asarray(inertia, np.float64)
    if I.shape == (3, 3):
        I = np.array([I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]])
    elif I.shape == (3,):
        I = np.concatenate([I, np.zeros(3)])
    if I.shape != (6,):
        raise SphError(f"dynamics: inertia of shape {np.shape(inertia)}")
    d = SphObstacleDynamics()
    d.mass = float(mass)
    d.inertia[:] = [float(x) for x in I]
    for field, val in (("com", com), ("force", force), ("torque", torque)):
        vals = [float(x) for x in val]
        if len(vals) != 3:
            raise SphError(f"dynamics: {field} needs 3 components, not {len(vals)}")
        getattr(d, field)[:] = vals
    d.gravityScale = float(gravity_scale)
    d.linearDamping = float(linear_damping)
    d.angularDamping = float(angular_damping)
    d.flags = SPH_DYNAMICS_CONFINED if confined else 0
    return d


def dynamics_sphere(density: float, size, **kw) -> SphObstacleDynamics:
    """A homogeneous sphere of radius size (or size[0]): m = 4/3 pi R^3 rho, I = 2/5 m R^2."""
    R = float(size if np.ndim(size) == 0 else size[0])
    m = density * 4.0 / 3.0 * math.pi * R ** 3
    return dynamics(m, [0.4 * m * R * R] * 3, **kw)


def dynamics_box(density: float, size, **kw) -> SphObstacleDynamics:
    """A homogeneous box of half extents size: m = 8 a b c rho, I_xx = m (b^2 + c^2) / 3 and so on."""
    a, b, c = (float(x) for x in size)
    m = density * 8.0 * a * b * c
    return dynamics(m, [m * (b * b + c * c) / 3.0, m * (a * a + c * c) / 3.0, m * (a * a + b * b) / 3.0], **kw)


def dynamics_capsule(density: float, size, **kw) -> SphObstacleDynamics:
    """A homogeneous capsule, size = (radius r, half length L of the core segment along local y): a cylinder of length 2 L and two
    half spheres, the half spheres' transverse moments by the parallel-axis rule from their own centroids (3 r / 8 beyond the ends)."""
    r, L = float(size[0]), float(size[1])
    mc = density * math.pi * r * r * 2.0 * L
    mh = density * 2.0 / 3.0 * math.pi * r ** 3                       # one half sphere
    iy = 0.5 * mc * r * r + 2.0 * (0.4 * mh * r * r)
    it = mc * (3.0 * r * r + 4.0 * L * L) / 12.0 + 2.0 * (mh * (0.4 - 9.0 / 64.0) * r * r + mh * (L + 0.375 * r) ** 2)
    return dynamics(mc + 2.0 * mh, [it, iy, it], **kw)


def dynamics_array(records) -> np.ndarray:
    """A list of SphObstacleDynamics (None: a kinematic body, mass 0) as a contiguous DYNAMICS_DTYPE array."""
    if isinstance(records, np.ndarray):
        return np.ascontiguousarray(records, DYNAMICS_DTYPE)
    records = list(records)
    if not records:
        return np.zeros(0, DYNAMICS_DTYPE)
    return np.frombuffer(b"".join(bytes(SphObstacleDynamics()) if r is None else bytes(r) for r in records), DYNAMICS_DTYPE).copy()


def mass_properties(moments, density: float):
    """(mass, centre of mass[3], inertia about it as (xx, yy, zz, xy, xz, yz)) from the ten moments of sph_volume_moments, by the
    parallel-axis rule in fp64."""
    m = np.asarray(moments, np.float64)
    if m.shape != (10,) or not m[0] > 0:
        raise SphError("mass_properties: ten moments with a positive volume are needed")
    vol = m[0]
    c = m[1:4] / vol
    sxx, syy, szz = m[4] - vol * c[0] * c[0], m[5] - vol * c[1] * c[1], m[6] - vol * c[2] * c[2]
    sxy, sxz, syz = m[7] - vol * c[0] * c[1], m[8] - vol * c[0] * c[2], m[9] - vol * c[1] * c[2]
    inertia = density * np.array([syy + szz, sxx + szz, sxx + syy, -sxy, -sxz, -syz])
    return float(density * vol), c, inertia


_PARAM_NAMES = {f[0] for f in SphParams._fields_}
_RIVER_NAMES = {f[0] for f in SphRiver._fields_}
_FOUNTAIN_NAMES = {f[0] for f in SphFountain._fields_}


class SPHFluidGPU:
    """Drop-in for the reference class of the same name (SPHFluid3D.h:26).

    SPHFluidGPU(numParticles)                    -> spawn as InitializeParticles does (seeded)
    SPHFluidGPU.from_particles(records, params)  -> caller-provided 80-byte records
    """

    def __init__(self, numParticles_: int = 50000, params: SphParams | None = None, seed: int = 1, stream: int | None = None,
                 _particles: np.ndarray | None = None):
        L = load_library()
        self._L = L
        self._p = params if params is not None else default_params()
        self._h = C.c_void_p()
        self._f = SphFountain()
        L.sph_fountain_default(C.byref(self._f))
        self._r = SphRiver()
        L.sph_river_default(C.byref(self._r))
        self.terrainHeights = np.zeros(0, np.float32)   # SPHFluid3D.h:175
        self._terrain_sent = None
        self.numParticles = int(numParticles_)
        self.seed = int(seed)
        if _particles is not None:
            arr = np.ascontiguousarray(_particles, dtype=PARTICLE_DTYPE)
            _check(L.sph_create_from_particles(C.byref(self._h), _ptr(arr), len(arr), C.byref(self._p), stream))
        else:
            _check(L.sph_create(C.byref(self._h), self.numParticles, C.byref(self._p), self.seed, stream))
        _check(L.sph_get_params(self._h, C.byref(self._p)))   # spawn overwrote param_mass (SPHFluid3D.cpp:92)

    @classmethod
    def from_particles(cls, particles: np.ndarray, params: SphParams, stream: int | None = None) -> "SPHFluidGPU":
        return cls(len(particles), params=params, stream=stream, _particles=particles)

    # -- public param_* members ----------------------------------------------------------
    def __getattr__(self, name):
        if name in _PARAM_NAMES or name in _FOUNTAIN_NAMES or name in _RIVER_NAMES:
            v = getattr(object.__getattribute__(self, "_p" if name in _PARAM_NAMES else ("_f" if name in _FOUNTAIN_NAMES else "_r")), name)
            return list(v) if hasattr(v, "__len__") else v
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in _PARAM_NAMES or name in _FOUNTAIN_NAMES or name in _RIVER_NAMES:
            st = self._p if name in _PARAM_NAMES else (self._f if name in _FOUNTAIN_NAMES else self._r)
            _assign(st, name, value)
        else:
            object.__setattr__(self, name, value)

    @property
    def params(self) -> SphParams:
        return self._p

    # -- reference methods ---------------------------------------------------------------
    def _push_params(self):
        _check(self._L.sph_set_params(self._h, C.byref(self._p)))

    def _push_members(self):
        _check(self._L.sph_set_params(self._h, C.byref(self._p)))  # members are re-read every dispatch (:458-506); spelled out: no extra frame in the timed loop
        _check(self._L.sph_set_fountain(self._h, C.byref(self._f)))  # fountain* members (:519-541)
        self._push_river()

    def _push_river(self):                                           # river members (:511-516); the heightfield only when it changed
        th = self.terrainHeights
        fresh = th is not self._terrain_sent and len(th) > 0
        ptr = None
        if fresh:
            th = np.ascontiguousarray(th, np.float32)
            if len(th) != self._r.terrainW * self._r.terrainH:
                raise SphError(f"terrainHeights has {len(th)} samples, terrainW x terrainH = {self._r.terrainW * self._r.terrainH}")
            ptr = _ptr(th)
        _check(self._L.sph_set_river(self._h, C.byref(self._r), ptr))
        if fresh:
            self._terrain_sent = self.terrainHeights

    def set_river(self, river: SphRiver, heights):                   # all river members + terrainHeights in one go
        C.memmove(C.byref(self._r), C.byref(river), C.sizeof(SphRiver))
        self.terrainHeights = np.ascontiguousarray(heights, np.float32).copy()
        self._push_river()

    def GenerateRiverTerrain(self, seed: int):                       # SPHFluid3D.cpp:772-878
        heights = np.zeros(self._r.terrainW * self._r.terrainH, np.float32)
        _check(self._L.sph_generate_river_terrain(C.byref(self._p), int(seed), C.byref(self._r), _ptr(heights)))
        self.terrainHeights = heights
        self._push_river()

    def DispatchCompute(self, overrideDt: float = -1.0):            # SPHFluid3D.cpp:431
        self._push_members()
        _check(self._L.sph_dispatch(self._h, overrideDt))
        _check(self._L.sph_get_fountain(self._h, C.byref(self._f)))  # fountainSeed++ (:541)

    SimulateSubstep = DispatchCompute   # BASELINE.json's name for the same entry point

    def DispatchN(self, n: int, overrideDt: float = -1.0):           # Scene0p.cpp:3720-3739 loop
        self._push_members()
        _check(self._L.sph_dispatch_n(self._h, overrideDt, int(n)))
        _check(self._L.sph_get_fountain(self._h, C.byref(self._f)))

    def ResetSimulation(self, seed: int | None = None):             # SPHFluid3D.cpp:713
        if seed is not None:
            self.seed = int(seed)
        self._push_params()
        self._push_river()                                           # riverMode && !terrainHeights.empty() picks the spawn branch (:104)
        _check(self._L.sph_reset(self._h, self.numParticles, self.seed))
        _check(self._L.sph_get_params(self._h, C.byref(self._p)))

    def ApplyWaveImpulse(self, amplitude, wavelength, phase, dir, yMin=-FLT_MAX, yMax=FLT_MAX):   # SPHFluid3D.cpp:604
        _check(self._L.sph_apply_wave_impulse(self._h, amplitude, wavelength, phase, _f3(dir), yMin, yMax))

    def ApplyVortexImpulse(self, tangentKick, inwardKick):          # SPHFluid3D.cpp:627
        self._push_params()   # reads param_boxCenter / EulerDeg / half
        _check(self._L.sph_apply_vortex_impulse(self._h, tangentKick, inwardKick))

    def ApplyAttractorImpulse(self, point, pullKick, radius):        # SPHFluid3D.cpp:650
        _check(self._L.sph_apply_attractor_impulse(self._h, _f3(point), pullKick, radius))

    def SetStencilTargets(self, points):                             # SPHFluid3D.cpp:684
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
        _check(self._L.sph_set_stencil_targets(self._h, _ptr(pts), len(pts)))
        self.stencilCount = len(pts)

    def ApplyStencilAttract(self, pullKick, dampKick):               # SPHFluid3D.cpp:695
        _check(self._L.sph_apply_stencil_attract(self._h, pullKick, dampKick))

    def ApplyCurlFlow(self, kick, scale, time):                      # SPHFluid3D.cpp:668
        _check(self._L.sph_apply_curl_flow(self._h, kick, scale, time))

    def EffectiveHalf(self):                                         # SPHFluid3D.h:127
        return effective_half(self._p)

    def ComputeGridExtents(self):                                    # SPHFluid3D.cpp:354
        return compute_grid_extents(self._p)

    def GetNumFluids(self) -> int:                                   # SPHFluid3D.cpp:601
        return int(self._L.sph_num_particles(self._h))

    # -- reference data members ----------------------------------------------------------
    @property
    def particles(self) -> np.ndarray:
        """Host copy of the INITIAL records (never refreshed, as in the reference)."""
        n = self.GetNumFluids()
        out = np.zeros(n, PARTICLE_DTYPE)
        _check(self._L.sph_initial_particles(self._h, _ptr(out), n))
        return out

    def _grid(self) -> SphGridInfo:
        g = SphGridInfo()
        _check(self._L.sph_grid_info(self._h, C.byref(g)))
        return g

    gridSizeX = property(lambda self: self._grid().dims[0])
    gridSizeY = property(lambda self: self._grid().dims[1])
    gridSizeZ = property(lambda self: self._grid().dims[2])
    numCells = property(lambda self: self._grid().numCells)
    gridMinV = property(lambda self: list(self._grid().gridMin))
    cellSize = property(lambda self: self._grid().cellSize)

    # -- engine extras -------------------------------------------------------------------
    def set_option(self, option: int, value: int):
        _check(self._L.sph_set_option(self._h, option, value))

    def get_option(self, option: int) -> int:
        v = C.c_int(0)
        _check(self._L.sph_get_option(self._h, option, C.byref(v)))
        return v.value

    def upload(self, particles: np.ndarray):
        arr = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
        _check(self._L.sph_upload_particles(self._h, _ptr(arr), len(arr)))

    def download(self) -> np.ndarray:
        n = self.GetNumFluids()
        out = np.zeros(n, PARTICLE_DTYPE)
        _check(self._L.sph_download_particles(self._h, _ptr(out), n))
        return out

    def device_particles(self) -> int:
        """Device address of the 80-byte AoS (the `ssbo` renderers bind, Scene0p.cpp:1625)."""
        p = C.c_void_p()
        _check(self._L.sph_device_particles(self._h, C.byref(p)))
        return int(p.value)

    def pack_render_buffer(self, dev_ptr: int, w_mode: int = 0):
        """(x, y, z, w) per particle in original order into a caller-owned device buffer (a mapped vertex
        buffer in a renderer; a torch tensor's data_ptr() in the tests)."""
        _check(self._L.sph_pack_render_buffer(self._h, C.c_void_p(dev_ptr), self.GetNumFluids(), int(w_mode)))

    def download_grid(self):
        g = compute_grid_extents(self._p)
        n = self.GetNumFluids()
        cnt = np.zeros(g.numCells, np.int32)
        pc = np.zeros(max(n, 1), np.int32)
        self._push_params()
        _check(self._L.sph_download_grid(self._h, _ptr(cnt), g.numCells, _ptr(pc), n))
        return cnt, pc[:n]

    def sync(self):
        _check(self._L.sph_sync(self._h))

    def debug_counters(self, reset: bool = False) -> dict:
        buf = (C.c_uint64 * len(STAMP_NAMES))()
        _check(self._L.sph_debug_counters(self._h, buf, len(STAMP_NAMES), 1 if reset else 0))
        return {k: int(buf[i]) for i, k in enumerate(STAMP_NAMES)}

    # -- field sampling (include/sph_abi.h "field sampling") ----------------------------------
    def sample(self, points) -> np.ndarray:
        """Fields of the current state at (m, 3) or (m, 4) probe points: a structured array of SAMPLE_DTYPE (density, fraction,
        pressure, count, vel).  Synchronises."""
        p4 = _points4(points, "sample", keep_w=False)
        out = np.zeros(len(p4), SAMPLE_DTYPE)
        self._push_params()
        _check(self._L.sph_sample_points(self._h, _ptr(p4), len(p4), _ptr(out)))
        return out

    def sample_device(self, dev_points: int, m: int, dev_out: int):
        """m probes of 4 floats at device address dev_points -> m 32-byte SphSample records at dev_out (a torch tensor's
        data_ptr(), say).  Asynchronous on the engine's stream."""
        self._push_params()
        _check(self._L.sph_sample_points_device(self._h, C.c_void_p(dev_points), int(m), C.c_void_p(dev_out)))

    def sample_lattice_device(self, origin, spacing, dims, dev_out: int, field: int = SPH_FIELD_DENSITY):
        """Lattice origin + i * spacing (dims = (nx, ny, nz), x fastest) into a caller's device buffer: one float per point, or one
        SphSample per point for SPH_FIELD_ALL.  Asynchronous on the engine's stream."""
        self._push_params()
        _check(self._L.sph_sample_lattice(self._h, _f3(origin), _f3(spacing), _dims3(dims), int(field), C.c_void_p(dev_out)))

    def sample_lattice(self, origin, spacing, dims, field: int = SPH_FIELD_DENSITY) -> np.ndarray:
        """Host copy of sample_lattice_device: shape (nz, ny, nx), float32 or SAMPLE_DTYPE (SPH_FIELD_ALL)."""
        import torch
        nx, ny, nz = (int(x) for x in dims)
        if min(nx, ny, nz) < 1:
            raise SphError(f"sample_lattice: dims must be >= 1, not {tuple(dims)}")
        words = 8 if field == SPH_FIELD_ALL else 1
        buf = torch.empty(nx * ny * nz * words, dtype=torch.float32, device="cuda")
        self.sample_lattice_device(origin, spacing, (nx, ny, nz), buf.data_ptr(), field)
        self.sync()
        host = buf.cpu().numpy()
        if field == SPH_FIELD_ALL:
            return host.view(SAMPLE_DTYPE).reshape(nz, ny, nx)
        return host.reshape(nz, ny, nx)

    def water_level(self, xz, y_lo: float, y_hi: float, dy: float, threshold: float = 0.5) -> np.ndarray:
        """Wave gauge: per (x, z) column, the first y from the top where `fraction` >= threshold, sampled at y_hi, y_hi - dy, ...
        down to y_lo and linearly interpolated against the sample above it; NaN where no sample reaches the threshold."""
        cols = np.asarray(xz, dtype=np.float32).reshape(-1, 2)
        ys = np.float32(y_hi) - np.arange(int(np.floor((y_hi - y_lo) / dy + 1e-6)) + 1, dtype=np.float32) * np.float32(dy)
        pts = np.zeros((len(cols), len(ys), 4), np.float32)
        pts[:, :, 0] = cols[:, None, 0]
        pts[:, :, 1] = ys[None, :]
        pts[:, :, 2] = cols[:, None, 1]
        frac = self.sample(pts.reshape(-1, 4))["fraction"].reshape(len(cols), len(ys))
        return gauge_levels(frac, ys, threshold)

    # -- spatial queries: what the five families below share ---------------------------------------
    def _radius(self, radius, default: float = 1.0):
        """A query's radius: the caller's, or for None `default` times param_h."""
        return default * self._p.param_h if radius is None else radius

    def _info(self, kind, getter):
        """A fresh info struct of `kind`, filled by the library's getter."""
        info = kind()
        _check(getter(self._h, C.byref(info)))
        return info

    # -- neighbour lists (include/sph_abi.h "fixed-radius neighbour lists") ------------------------
    def neighbors(self, radius=None, self_=False, half=False, count_only=False, max_pairs: int = 0, device: bool = False):
        """CSR neighbour lists of every particle within `radius` (None: param_h; at most three cells): (offsets int64[n + 1], indices
        int32[total]) in the engine's order, ascending (cell index, particle id) per row; rows are numbered by particle id.  self_ keeps
        the particle itself, half keeps only id_j > id_i, count_only returns indices None.  numpy arrays, or with device=True fresh
        torch device tensors.  A total above max_pairs (> 0) raises SphError; neighbor_lists() then still gives the offsets."""
        self._push_params()
        info = SphNeighborInfo()
        _check(self._L.sph_neighbors_build(self._h, float(self._radius(radius)), _neighbor_flags(self_, half, count_only), int(max_pairs), C.byref(info)))
        return self.neighbor_lists(device)

    def query_neighbors(self, points, radius, count_only=False, max_pairs: int = 0, device: bool = False):
        """The same for (m, 3) or (m, 4) query points: row i lists the particles within `radius` of points[i] (a torch device tensor of
        (m, 4) float32 is used in place).  A point with a non-finite coordinate has an empty row."""
        dev = _device_points4(points, "query_neighbors")
        self._push_params()
        info = SphNeighborInfo()
        _check(self._L.sph_neighbors_query(self._h, C.c_void_p(dev.data_ptr()), int(dev.shape[0]), float(radius), _neighbor_flags(False, False, count_only),
                                           int(max_pairs), C.byref(info)))
        return self.neighbor_lists(device)

    def neighbor_info(self) -> SphNeighborInfo:
        """What the engine's lists hold: rows, total, radius, stencil, flags, kind (0 none, 1 particles, 2 query), maxCount."""
        return self._info(SphNeighborInfo, self._L.sph_neighbors_info)

    def neighbor_lists(self, device: bool = False):
        """(offsets, indices) of the lists the engine holds; indices is None for count-only lists and after a max_pairs refusal."""
        info = self.neighbor_info()
        dp_off, dp_idx = C.c_void_p(), C.c_void_p()
        _check(self._L.sph_neighbors_device(self._h, C.byref(dp_off), C.byref(dp_idx)))
        rows, total = int(info.rows), int(info.total)
        indexed = not (info.flags & SPH_NEIGHBORS_COUNT_ONLY) and bool(dp_idx.value)      # (a refused build lends no indices)
        copy = self._L.sph_neighbors_export if device else self._L.sph_neighbors_download
        specs = ((rows + 1, np.int64, "int64"), (total, np.int32, "int32") if indexed else None)
        off, idx = _fetch(lambda p_off, p_idx: copy(self._h, p_off, p_idx, total), device, specs, null_empty=device)   # (the host copy is given an empty idx as it is)
        if device:
            self.sync()
        return off, idx

    def radius_graph(self, radius=None, half: bool = False):
        """The neighbour relation as a (2, E) int64 torch device tensor [receiver, sender] (E = total; half: every undirected edge once,
        receiver < sender), derived from the CSR lists on the device.  Edges stand in CSR order."""
        import torch
        off, idx = self.neighbors(radius, half=half, device=True)
        recv = torch.repeat_interleave(torch.arange(off.numel() - 1, device=off.device), off[1:] - off[:-1])
        return torch.stack((recv, idx.to(torch.int64)))

    # -- connected components (include/sph_abi.h "connected components") --------------------------
    def components(self, radius=None, fluid_only: bool = False, device: bool = False):
        """Connected bodies of the neighbour relation at `radius` (None: param_h; at most three cells): (labels int32[n], roots int32[n],
        table COMPONENT_DTYPE[C]).  roots[i] is the smallest particle id of i's body, bodies are numbered in ascending order of it and
        labels[i] is that number; fluid_only leaves out the records with isGhost != 0 (label and root -1).  numpy arrays; with device=True
        labels and roots are fresh torch int32 device tensors (the table stays a numpy array)."""
        self._push_params()
        info = SphComponentInfo()
        _check(self._L.sph_components_build(self._h, float(self._radius(radius)), SPH_COMPONENTS_FLUID_ONLY if fluid_only else 0, C.byref(info)))
        n, c = int(info.rows), int(info.numComponents)
        specs = ((n, np.int32, "int32"), (n, np.int32, "int32"), (c, COMPONENT_DTYPE, None))
        return _fetch(lambda p_labels, p_roots, p_table: self._L.sph_components_download(self._h, p_labels, p_roots, p_table, c), device, specs)

    def component_info(self) -> SphComponentInfo:
        """What the engine's components hold: rows, numComponents, numExcluded, largestCount, largestRoot, numSingletons, radius, stencil,
        flags, rounds.  SphError before any components() call."""
        return self._info(SphComponentInfo, self._L.sph_components_info)

    # -- k nearest neighbours (include/sph_abi.h "k nearest neighbours") ---------------------------
    def knn(self, k: int, radius=None, self_=False, fluid_only: bool = False, device: bool = False):
        """The k nearest particles of every particle within `radius` (None: param_h; at most three cells), nearest first, ties to the
        smaller id: (idx (n, k) int32 padded with -1, d2 (n, k) float32 padded with +inf, counts (n,) uint32); rows are numbered by
        particle id.  self_ makes the particle an ordinary candidate of its own row (distance 0), fluid_only leaves the records with
        isGhost != 0 out of every row and gives them empty rows.  numpy arrays, or with device=True fresh torch device tensors."""
        self._push_params()
        info = SphKnnInfo()
        _check(self._L.sph_knn_build(self._h, int(k), float(self._radius(radius)), _knn_flags(self_, fluid_only), C.byref(info)))
        return self.knn_rows(device)

    def query_knn(self, points, k: int, radius, fluid_only: bool = False, device: bool = False):
        """The same around (m, 3) or (m, 4) query points: row i holds the k nearest particles within `radius` of points[i] (a torch
        device tensor of (m, 4) float32 is used in place).  A point with a non-finite coordinate has an empty row."""
        dev = _device_points4(points, "query_knn")
        self._push_params()
        info = SphKnnInfo()
        m = int(dev.shape[0])
        _check(self._L.sph_knn_query(self._h, C.c_void_p(dev.data_ptr()) if m else None, m, int(k), float(radius), _knn_flags(False, fluid_only),
                                     C.byref(info)))
        return self.knn_rows(device)

    def knn_info(self) -> SphKnnInfo:
        """What the engine's rows hold: rows, total (sum of counts), rowsFull (rows with count == k), k, radius, stencil, flags, kind
        (1 particles, 2 query).  SphError before any knn() / query_knn() call."""
        return self._info(SphKnnInfo, self._L.sph_knn_info)

    def knn_rows(self, device: bool = False):
        """(idx, d2, counts) of the rows the engine holds."""
        info = self.knn_info()
        rows, k = int(info.rows), int(info.k)
        specs = (((rows, k), np.int32, "int32"), ((rows, k), np.float32, "float32"),
                 (rows, np.uint32, "int32"))                                             # (uint32 counts <= 64 in an int32 tensor: the same bits)
        return _fetch(lambda p_idx, p_d2, p_cnt: self._L.sph_knn_download(self._h, p_idx, p_d2, p_cnt), device, specs)

    def knn_graph(self, k: int, radius=None, self_=False):
        """The k-nearest-neighbour relation as a (2, E) int64 torch device tensor [receiver, sender], E = knn_info().total: the padded
        entries are removed; edges stand in row order, then rank order."""
        import torch
        idx, _, _ = self.knn(k, radius, self_=self_, device=True)
        recv = torch.arange(idx.shape[0], device=idx.device).unsqueeze(1).expand(-1, idx.shape[1])
        keep = idx >= 0
        return torch.stack((recv[keep], idx[keep].to(torch.int64)))

    # -- ray casts (include/sph_abi.h "ray casts") ------------------------------------------------
    def raycast(self, rays, radius=None, fluid_only: bool = False, any_hit: bool = False, device: bool = False):
        """The first particle every ray enters, each particle a solid sphere of `radius` (None: 0.25 * param_h; at most half a cell).
        rays: (m, 8) float32 rows (ox, oy, oz, tmin, dx, dy, dz, tmax), numpy or a torch device tensor (used in place); t is in units of
        the given direction.  Returns (t (m,), ids (m,) int32, pos (m, 3), normal (m, 3)); a miss is (+inf, -1, zeros).  fluid_only
        leaves out the records with isGhost != 0; any_hit only says whether anything is met (ids 0 / -1, t 0 / +inf).  numpy arrays, or
        with device=True fresh torch device tensors (views of one copy of the engine's hits, as knn's rows)."""
        import torch
        self._push_params()
        info = SphRaysInfo()
        r = self._radius(radius, 0.25)
        flags = _rays_flags(fluid_only, any_hit)
        if isinstance(rays, torch.Tensor):
            if not (_is_cuda_f32(rays) and rays.dim() == 2 and rays.shape[1] == 8):
                raise SphError(f"raycast: a torch tensor of rays must be a contiguous float32 device tensor of shape (m, 8), not {tuple(rays.shape)}")
            m = int(rays.shape[0])
            _check(self._L.sph_rays_cast_device(self._h, C.c_void_p(rays.data_ptr()) if m else None, m, float(r), flags, C.byref(info)))
        else:
            r8 = _rays8(rays, "raycast")
            _check(self._L.sph_rays_cast(self._h, _ptr(r8) if len(r8) else None, len(r8), float(r), flags, C.byref(info)))
        return self.ray_hits(device)

    def rays_info(self) -> SphRaysInfo:
        """What the engine's hits hold: rays, hits, voidRays, radius, flags.  SphError before any raycast() call."""
        return self._info(SphRaysInfo, self._L.sph_rays_info)

    def ray_hits(self, device: bool = False):
        """(t, ids, pos, normal) of the hits the engine holds."""
        m = int(self.rays_info().rays)
        spec = ((m, 8), None, "float32") if device else (m, RAY_HIT_DTYPE, None)        # (one device copy of the 32-byte hits, split into views)
        (z,) = _fetch(lambda p_hits: self._L.sph_rays_download(self._h, p_hits), device, (spec,))
        if device:
            import torch
            return z[:, 0], z[:, 1].view(torch.int32), z[:, 2:5], z[:, 5:8]
        return _split_hits(z)

    # -- ray spans (include/sph_abi.h "ray spans") ------------------------------------------------
    def ray_spans(self, rays, radius=None, fluid_only: bool = False, device: bool = False):
        """What every ray crosses in all, each particle a solid sphere of `radius` (None: 0.25 * param_h; at most half a cell): a
        RAY_SPAN_DTYPE array (tEnter, tExit, idEnter, idExit, count, flags, length), one row per ray; ray_thickness() turns length into
        world units.  rays as for raycast(): (m, 8) float32, numpy or a torch device tensor (used in place).  A sphere that contains the
        ray's start counts; nothing crossed is (+inf, -inf, -1, -1, 0); flags bit 0 marks a void ray.  With device=True a fresh (m, 8)
        int32 torch device tensor of the same 32-byte rows.  The held hits of raycast() are not touched."""
        import torch
        self._push_params()
        info = SphRaySpansInfo()
        r = self._radius(radius, 0.25)
        flags = _rays_flags(fluid_only, False)
        if isinstance(rays, torch.Tensor):
            if not (_is_cuda_f32(rays) and rays.dim() == 2 and rays.shape[1] == 8):
                raise SphError(f"ray_spans: a torch tensor of rays must be a contiguous float32 device tensor of shape (m, 8), not {tuple(rays.shape)}")
            m = int(rays.shape[0])
            _check(self._L.sph_rays_span_device(self._h, C.c_void_p(rays.data_ptr()) if m else None, m, float(r), flags, C.byref(info)))
        else:
            r8 = _rays8(rays, "ray_spans")
            _check(self._L.sph_rays_span(self._h, _ptr(r8) if len(r8) else None, len(r8), float(r), flags, C.byref(info)))
        return self.ray_span_rows(device)

    def ray_spans_info(self) -> SphRaySpansInfo:
        """What the engine's spans hold: rays, crossed, voidRays, total, maxCount, radius, flags.  SphError before any ray_spans() call."""
        return self._info(SphRaySpansInfo, self._L.sph_rays_span_info)

    def ray_span_rows(self, device: bool = False):
        """The spans the engine holds: a RAY_SPAN_DTYPE array, or with device=True an (m, 8) int32 torch device tensor of the same bytes."""
        m = int(self.ray_spans_info().rays)
        spec = ((m, 8), None, "int32") if device else (m, RAY_SPAN_DTYPE, None)
        (z,) = _fetch(lambda p_rows: self._L.sph_rays_span_download(self._h, p_rows), device, (spec,))
        return z

    # -- free-surface particles (include/sph_abi.h "free-surface particles") ----------------------
    def shell(self, radius=None, offset: float = 0.10, min_count: int = 0, fluid_only: bool = False, device: bool = False):
        """The free-surface shell of the particles from their positions alone: (rows, ids).  rows is a SHELL_DTYPE array numbered by
        particle id (normal, offsetRatio, crest, count, flags: SPH_SHELL_MEMBER, SPH_SHELL_ISOLATED), ids the int32 particle ids of the
        shell in ascending order.  A particle is in the shell when the weighted centroid of its neighbours within `radius` (None:
        param_h; at most three cells) lies further than offset * radius from it, when it has fewer than min_count neighbours, or none;
        normal points out of the fluid, crest measures how sharply convex the shell is there.  fluid_only leaves the records with
        isGhost != 0 out of every sum and gives them all-zero rows.  With device=True torch device tensors: ((n, 8) float32 rows --
        columns 0:3 normal, 3 offsetRatio, 4 crest, 5 / 6 count / flags as bits (view(torch.int32)) -- and ids (numShell,) int32)."""
        self._push_params()
        info = SphShellInfo()
        cfg = _shell_cfg(radius, offset, min_count, fluid_only)
        _check(self._L.sph_shell_build(self._h, C.byref(cfg), C.byref(info)))
        return self.shell_rows(device)

    def query_shell(self, points, radius, offset: float = 0.10, min_count: int = 0, fluid_only: bool = False, device: bool = False):
        """The same first pass around (m, 3) or (m, 4) query points (a torch device tensor of (m, 4) float32 is used in place): row i is
        the record of points[i] (no own slot is left out, crest is 0), ids lists the flagged points.  A smooth surface normal at a ray
        hit or a mesh vertex.  A point with a non-finite coordinate has an all-zero row."""
        dev = _device_points4(points, "query_shell")
        self._push_params()
        info = SphShellInfo()
        cfg = _shell_cfg(float(radius), offset, min_count, fluid_only)                   # (no default radius for a query: None is a TypeError)
        m = int(dev.shape[0])
        _check(self._L.sph_shell_query(self._h, C.c_void_p(dev.data_ptr()) if m else None, m, C.byref(cfg), C.byref(info)))
        return self.shell_rows(device)

    def shell_info(self) -> SphShellInfo:
        """What the engine's free-surface rows hold: rows, numShell, numIsolated, maxCount, radius, stencil, kind (1 particles, 2 query),
        flags.  SphError before any shell() / query_shell() call."""
        return self._info(SphShellInfo, self._L.sph_shell_info)

    def shell_rows(self, device: bool = False):
        """(rows, ids) of the free-surface rows the engine holds."""
        info = self.shell_info()
        rows, ns = int(info.rows), int(info.numShell)
        spec = ((rows, 8), None, "float32") if device else (rows, SHELL_DTYPE, None)    # (one device copy of the 32-byte rows)
        return _fetch(lambda p_rows, p_ids: self._L.sph_shell_download(self._h, p_rows, p_ids), device, (spec, (ns, np.int32, "int32")))

    # -- anisotropic kernels (include/sph_abi.h "anisotropic kernels") ------------------------------
    def anisotropy(self, radius=None, support=None, smoothing: float = 0.9, max_ratio: float = 4.0, max_stretch: float = 1.5, min_count: int = 25,
                   sparse_scale: float = 0.5, fluid_only: bool = False, device: bool = False):
        """Per particle the smoothed centre and the ellipsoid of the anisotropic kernel (Yu & Turk 2013): an
        ANISO_DTYPE array numbered by particle id (center, count, axis0 / axis1 / axis2: the semi-axis vectors in world units, longest
        first, flags: SPH_ANISO_VALID / _SPARSE / _CLAMPED, reach, amplitude).  radius (None: 2 param_h; at most three cells) bounds
        the neighbourhood whose weighted covariance shapes the ellipsoid, support (None: param_h) scales it, smoothing pulls the centre
        towards the neighbourhood's mean, max_ratio bounds longest / shortest axis, max_stretch the longest axis in units of support;
        a particle with fewer than min_count neighbours gets a sphere of sparse_scale * support.  fluid_only leaves the records with
        isGhost != 0 out of every sum and gives them all-zero rows.  With device=True an (n, 16) float32 torch device tensor (columns
        0:3 center, 4:7 axis0, 8:11 axis1, 11 reach, 12:15 axis2, 15 amplitude; 3 / 7 count / flags as bits)."""
        self._push_params()
        info = SphAnisoInfo()
        cfg = _aniso_cfg(radius, support, smoothing, max_ratio, max_stretch, min_count, sparse_scale, fluid_only)
        _check(self._L.sph_aniso_build(self._h, C.byref(cfg), C.byref(info)))
        return self.aniso_rows(device)

    def aniso_info(self) -> SphAnisoInfo:
        """What the engine's anisotropy rows hold: rows, numSparse, numClamped, maxCount, radius, support, stencil, maxReach,
        reachStencil, kind, flags.  SphError before any anisotropy() / aniso_lattice() / aniso_surface() call."""
        return self._info(SphAnisoInfo, self._L.sph_aniso_info)

    def aniso_rows(self, device: bool = False):
        """The anisotropy rows the engine holds."""
        rows = int(self.aniso_info().rows)
        spec = ((rows, 16), None, "float32") if device else (rows, ANISO_DTYPE, None)   # (one device copy of the 64-byte rows)
        return _fetch(lambda p_rows: self._L.sph_aniso_download(self._h, p_rows), device, (spec,))[0]

    def aniso_lattice(self, origin, spacing, dims, device: bool = False, **cfg):
        """The anisotropic fraction on the lattice origin + i * spacing (dims = (nx, ny, nz), x fastest), summed from the ellipsoids of
        a fresh anisotropy(**cfg) build: float32 of shape (nz, ny, nx), a numpy array or with device=True a torch device tensor.
        SphError where the largest reach exceeds three cells (aniso_info() then still describes the rows)."""
        import torch
        nx, ny, nz = (int(x) for x in dims)
        buf = torch.empty((max(nz, 0), max(ny, 0), max(nx, 0)), dtype=torch.float32, device="cuda")
        self._push_params()
        info = SphAnisoInfo()
        _check(self._L.sph_aniso_lattice(self._h, C.byref(_aniso_cfg(**cfg)), _f3(origin), _f3(_spacing3(spacing)), _dims3((nx, ny, nz)),
                                         C.c_void_p(buf.data_ptr()) if buf.numel() else None, C.byref(info)))
        self.sync()
        return buf if device else buf.cpu().numpy()

    def aniso_surface(self, origin=None, spacing=None, dims=None, iso: float = 0.5, **cfg):
        """Iso-surface {anisotropic fraction >= iso} as a closed triangle mesh, flatter on flat water and thinner on sheets than
        surface(): (vertices of SURFACE_VERTEX_DTYPE, triangles (T, 3) uint32).  Lattice members left None come from
        default_surface_lattice(); cfg: the arguments of anisotropy()."""
        do, ds, dd = self.default_surface_lattice() if origin is None or spacing is None or dims is None else (None, None, None)
        surf, info = SphSurface(), SphAnisoInfo()
        self._push_params()
        _check(self._L.sph_aniso_surface(self._h, C.byref(_aniso_cfg(**cfg)), _f3(do if origin is None else origin),
                                         _f3(_spacing3(ds if spacing is None else spacing)), _dims3(dd if dims is None else dims), float(iso),
                                         C.byref(surf), C.byref(info)))
        return self._download_surface(surf)

    # -- fused neighbourhood reductions (include/sph_abi.h "fused neighbourhood reductions") -----------
    def aggregate(self, values, radius=None, op="sum", weight="one", self_=False, fluid_only=False, delta=False, moments=False, counts=False,
                  device: bool = False):
        """Sum, mean, max or min of the caller's per-particle tensor over every particle's neighbours within `radius` (None: param_h;
        at most three cells), fused into the grid walk: no edge list, no gather, and the same bytes on every run (DESIGN.md section
        3u).  values: an (n, C) or (n,) numpy array, which is uploaded, or a contiguous float32 torch device tensor of (n, C), which
        is used in place; 1 <= C <= 128.  op "sum" | "mean" | "max" | "min"; weight "one" | "poly6" ((R^2 - r^2)^3, not with max /
        min); self_ keeps the particle itself (d = 0); fluid_only leaves the records with isGhost != 0 out and gives them empty rows;
        delta reduces values[j] - values[i]; moments (sum only) adds the three planes sum (w d_a) v, d = x_j - x_i.  Returns float32
        of shape (n, C), or (n, 4, C) with moments; with counts=True (out, counts uint32[n], the candidates reduced).  An empty row is
        0 for sum and mean, -inf for max, +inf for min.  numpy arrays, or with device=True fresh torch device tensors.
        Streams: the engine works on its own stream.  Torch's current stream is synchronised before the call, so that values written
        there are complete, and the engine's stream is synchronised (sync()) before the results are returned, also with device=True."""
        return self._aggregate(None, values, self._radius(radius), op, weight, self_, fluid_only, delta, moments, counts, device)

    def query_aggregate(self, points, values, radius, op="sum", weight="one", fluid_only=False, moments=False, counts=False, device: bool = False):
        """The same around (m, 3) or (m, 4) query points: row i reduces the particles within `radius` of points[i] (a torch device tensor
        of (m, 4) float32 is used in place).  A point with a non-finite coordinate has an empty row.  Streams as aggregate()."""
        return self._aggregate(_device_points4(points, "query_aggregate"), values, radius, op, weight, False, fluid_only, False, moments, counts, device)

    def _aggregate(self, dev_points, values, radius, op, weight, self_, fluid_only, delta, moments, counts, device):
        import torch
        vals = _device_values(values, "aggregate")
        n, c = int(vals.shape[0]), int(vals.shape[1])
        if n != self.GetNumFluids():
            raise SphError(f"aggregate: {n} rows of values for {self.GetNumFluids()} particles")
        cfg = _aggregate_cfg(radius, op, weight, c, self_, fluid_only, delta, moments)
        rows = n if dev_points is None else int(dev_points.shape[0])
        shape = (rows, 4, c) if moments else (rows, c)
        written = rows and n                                                          # (nothing is written otherwise: sph_abi.h)
        out = (torch.empty if written else torch.zeros)(shape, dtype=torch.float32, device="cuda")
        cnt = (torch.empty if written else torch.zeros)(rows, dtype=torch.int32, device="cuda") if counts else None
        torch.cuda.current_stream().synchronize()
        self._push_params()
        info = SphAggregateInfo()
        p_out, p_cnt = _tensor_ptr(out), None if cnt is None else _tensor_ptr(cnt)
        if dev_points is None:
            _check(self._L.sph_aggregate_particles(self._h, C.byref(cfg), _tensor_ptr(vals), p_out, p_cnt, C.byref(info)))
        else:
            _check(self._L.sph_aggregate_query(self._h, C.byref(cfg), _tensor_ptr(dev_points), rows, _tensor_ptr(vals), p_out, p_cnt, C.byref(info)))
        self.sync()
        if not device:
            out = out.cpu().numpy()
            cnt = None if cnt is None else cnt.cpu().numpy().view(np.uint32)
        return (out, cnt) if counts else out

    # -- the adjoint of the neighbourhood sums, extrema with winners, routing (include/sph_abi.h "the adjoint of the neighbourhood sums") --
    def aggregate_adjoint(self, grad, radius=None, weight="one", self_=False, fluid_only=False, delta=False, moments=False, device: bool = False):
        """The exact transpose of aggregate(op="sum") with the same arguments, applied to grad: (n, C), or (n, 4, C) with moments, what
        aggregate() would return (numpy, or a contiguous float32 torch device tensor, which is used in place).  Returns (n, C) float32:
        row k sums what the rows that accept particle k carry, in ascending sorted slot with the forward's own weights and offsets
        (DESIGN.md section 3v); without moments these are the bytes of aggregate(grad, ...).  Streams as aggregate()."""
        return self._adjoint(None, grad, self._radius(radius), "sum", weight, self_, fluid_only, delta, moments, None, device)

    def query_aggregate_adjoint(self, points, point_values, radius, weight="one", fluid_only=False, moments=False, device: bool = False):
        """The point -> particle transfer, the transpose of query_aggregate(op="sum"): point_values (m, C), or (m, 4, C) with moments, sit
        on the (m, 3) or (m, 4) query points, and row k of the (n, C) result sums what the points within `radius` of particle k carry,
        in ascending (clamped cell of the point, point index).  The points are binned into the engine's grid on the device, the particles
        gather: no float atomics, the same bytes on every run.  A point with a non-finite coordinate contributes nothing.  Streams as
        aggregate()."""
        return self._adjoint(_device_points4(points, "query_aggregate_adjoint"), point_values, radius, "sum", weight, False, fluid_only, False, moments, None, device)

    def aggregate_route(self, arg, grad, radius=None, op="max", self_=False, fluid_only=False, delta=False, device: bool = False):
        """The routing of a gradient through aggregate(op="max" | "min"): arg (n, C) int32 from aggregate_arg() with the same arguments,
        grad (n, C); row k of the (n, C) result sums grad[i][c] over the rows i with arg[i][c] == k, in the adjoint's row order."""
        return self._adjoint(None, grad, self._radius(radius), op, "one", self_, fluid_only, delta, False, arg, device)

    def query_aggregate_route(self, points, arg, grad, radius, op="max", fluid_only=False, device: bool = False):
        """The same through query_aggregate(op="max" | "min"): arg and grad are (m, C), one row per query point."""
        return self._adjoint(_device_points4(points, "query_aggregate_route"), grad, radius, op, "one", False, fluid_only, False, False, arg, device)

    def _adjoint(self, dev_points, grad, radius, op, weight, self_, fluid_only, delta, moments, arg, device):
        import torch
        n = self.GetNumFluids()
        rows = n if dev_points is None else int(dev_points.shape[0])
        g = _device_planes(grad, rows, moments, "aggregate_adjoint")
        c = int(g.shape[-1])
        cfg = _aggregate_cfg(radius, op, weight, c, self_, fluid_only, delta, moments)
        a = None
        if arg is not None:
            a = arg if isinstance(arg, torch.Tensor) and arg.is_cuda and arg.dtype == torch.int32 and arg.is_contiguous() else \
                torch.from_numpy(np.ascontiguousarray(arg.detach().cpu().numpy() if isinstance(arg, torch.Tensor) else arg, np.int32)).cuda()
            if tuple(a.shape) != (rows, c):
                raise SphError(f"aggregate_route: arg of shape {tuple(a.shape)} for grad of shape {(rows, c)}")
        out = torch.empty((n, c), dtype=torch.float32, device="cuda")
        torch.cuda.current_stream().synchronize()
        self._push_params()
        info = SphAggregateInfo()
        L, h, p = self._L, self._h, C.byref(cfg)
        if a is None and dev_points is None:
            _check(L.sph_aggregate_adjoint_particles(h, p, _tensor_ptr(g), _tensor_ptr(out), C.byref(info)))
        elif a is None:
            _check(L.sph_aggregate_adjoint_query(h, p, _tensor_ptr(dev_points), rows, _tensor_ptr(g), _tensor_ptr(out), C.byref(info)))
        elif dev_points is None:
            _check(L.sph_aggregate_route_particles(h, p, _tensor_ptr(a), _tensor_ptr(g), _tensor_ptr(out), C.byref(info)))
        else:
            _check(L.sph_aggregate_route_query(h, p, _tensor_ptr(dev_points), rows, _tensor_ptr(a), _tensor_ptr(g), _tensor_ptr(out), C.byref(info)))
        self.sync()
        return out if device else out.cpu().numpy()

    # -- position gradients of the neighbourhood sums (include/sph_abi.h "position gradients of the neighbourhood sums") --
    def positions(self, device: bool = False):
        """The current positions by particle id as (n, 3) float32: a numpy array, or with device=True a fresh torch device tensor (what
        aggregate_autograd(positions=...) hangs the position gradient on)."""
        if not device:
            return np.ascontiguousarray(self.download()["pos"][:, :3])
        import torch
        buf = torch.empty((self.GetNumFluids(), 4), dtype=torch.float32, device="cuda")
        torch.cuda.current_stream().synchronize()
        if buf.numel():
            self.pack_render_buffer(buf.data_ptr())
        self.sync()
        return buf[:, :3].contiguous()

    def aggregate_position_grad(self, values, grad, radius=None, weight="one", self_=False, fluid_only=False, delta=False, moments=False,
                                device: bool = False):
        """d/dx of L = sum(grad * aggregate(values, op="sum", ...)) with the same arguments: (n, 3) float32 by particle id.  values (n, C)
        as aggregate(); grad (n, C), or (n, 4, C) with moments, as aggregate_adjoint().  Row k sums, over k's neighbours in ascending
        sorted slot, the pair terms of both directions with the forward's own offsets and weights: no edge list,
        no float atomics, the same bytes on every run.  The cutoff is not differentiated; weight "one" without moments gives zeros.
        Streams as aggregate()."""
        return self._posgrad(None, values, grad, self._radius(radius), weight, self_, fluid_only, delta, moments, True, True, device)[1]

    def query_aggregate_position_grad(self, points, values, grad, radius, weight="one", fluid_only=False, moments=False, device: bool = False,
                                      want_points: bool = True, want_particles: bool = True):
        """The same for query_aggregate(points, values, op="sum", ...): (grad_points (m, 3), grad_particles (n, 3)); grad is (m, C) or
        (m, 4, C).  grad_points row i sums over the row's candidates in the forward's order, grad_particles row k over the points that
        accept particle k in ascending (clamped cell of the point, point index).  want_points / want_particles False: that walk is not
        launched and None stands in its place (not both)."""
        return self._posgrad(_device_points4(points, "query_aggregate_position_grad"), values, grad, radius, weight, False, fluid_only, False, moments,
                             want_points, want_particles, device)

    def _posgrad(self, dev_points, values, grad, radius, weight, self_, fluid_only, delta, moments, want_points, want_particles, device):
        import torch
        vals = _device_values(values, "aggregate_position_grad")
        n, c = int(vals.shape[0]), int(vals.shape[1])
        if n != self.GetNumFluids():
            raise SphError(f"aggregate_position_grad: {n} rows of values for {self.GetNumFluids()} particles")
        rows = n if dev_points is None else int(dev_points.shape[0])
        g = _device_planes(grad, rows, moments, "aggregate_position_grad")
        if int(g.shape[-1]) != c:
            raise SphError(f"aggregate_position_grad: grad of shape {tuple(g.shape)} for values of shape {(n, c)}")
        cfg = _aggregate_cfg(radius, "sum", weight, c, self_, fluid_only, delta, moments)
        out_pts = torch.empty((rows, 3), dtype=torch.float32, device="cuda") if dev_points is not None and want_points else None
        out_par = torch.empty((n, 3), dtype=torch.float32, device="cuda") if want_particles else None
        torch.cuda.current_stream().synchronize()
        self._push_params()
        info = SphAggregateInfo()
        L, h, p = self._L, self._h, C.byref(cfg)
        if dev_points is None:
            _check(L.sph_aggregate_posgrad_particles(h, p, _tensor_ptr(vals), _tensor_ptr(g), _tensor_ptr(out_par), C.byref(info)))
        else:
            # (an output of no rows still goes as a non-null pointer: null means "not wanted")
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if t.numel() else _NO_POINT.ctypes.data)
            _check(L.sph_aggregate_posgrad_query(h, p, _tensor_ptr(dev_points), rows, _tensor_ptr(vals), _tensor_ptr(g), ptr(out_pts), ptr(out_par), C.byref(info)))
        self.sync()
        if not device:
            out_pts, out_par = (None if t is None else t.cpu().numpy() for t in (out_pts, out_par))
        return out_pts, out_par

    def aggregate_autograd(self, values, radius=None, op="sum", weight="one", self_=False, fluid_only=False, delta=False, moments=False,
                           check_state: bool = True, positions=None):
        """aggregate() as a torch.autograd.Function: values is a float32 torch device tensor of (n, C) that may require grad, the result
        has the bytes of aggregate(..., device=True) and carries a graph whose backward is the engine's adjoint (sum: aggregate_adjoint;
        mean: the adjoint of grad / W; max / min: aggregate_route through the winners of aggregate_arg), so no edge list is built.
        Once differentiable: a backward of the backward raises.  positions: None (differentiable in values only), or the (n, 3)
        tensor of positions(device=True), which then takes part in the graph and receives dL/dx through aggregate_position_grad
        (zeros for max / min; the cutoff is not differentiated).  check_state: the forward stores
        state_digest(["particles"]) and the backward raises SphError if it has changed, because a dispatch in between would silently give
        the adjoint of another neighbour relation; each of the two reads checksums the particle section on the device and synchronises
        (about the cost of one download-free pass over the records); with positions the forward also verifies that the tensor holds
        the engine's positions byte for byte.  False skips all of it.  See autograd.py for the formulas."""
        from .autograd import EngineAggregateBackend, aggregate_autograd
        return aggregate_autograd(EngineAggregateBackend(self), None, values, self._radius(radius), op, weight, self_, fluid_only, delta, moments, check_state,
                                  positions=positions)

    def query_aggregate_autograd(self, points, values, radius, op="sum", weight="one", fluid_only=False, moments=False, check_state: bool = True,
                                 positions=None, points_grad: bool = False):
        """query_aggregate() as a torch.autograd.Function of values ((n, C) on the device); the result is (m, C) or (m, 4, C).  The backward
        is query_aggregate_adjoint / query_aggregate_route.  positions as aggregate_autograd(); points_grad=True: points must be a float32
        torch device tensor of (m, 3) or (m, 4) and receives the points' gradient of query_aggregate_position_grad (without it a points
        tensor that requires grad still gets None).  Everything else as aggregate_autograd()."""
        import torch
        from .autograd import EngineAggregateBackend, aggregate_autograd
        leaf = None
        if points_grad:
            if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32 or points.dim() != 2 or int(points.shape[1]) not in (3, 4):
                raise SphError("query_aggregate_autograd: points_grad takes the query points as a float32 torch device tensor of shape (m, 3) or (m, 4)")
            leaf = points
            flat = points.detach()
            points = flat.contiguous() if int(flat.shape[1]) == 4 else torch.cat([flat, torch.zeros_like(flat[:, :1])], dim=1).contiguous()
        return aggregate_autograd(EngineAggregateBackend(self), _device_points4(points, "query_aggregate_autograd"), values, radius, op, weight, False,
                                  fluid_only, False, moments, check_state, positions=positions, points_grad=points_grad, points_leaf=leaf)

    def aggregate_arg(self, values, radius=None, op="max", self_=False, fluid_only=False, delta=False, counts=False, device: bool = False):
        """aggregate(op="max" | "min") and who won: (out, arg) or with counts=True (out, counts, arg).  out and counts are the bytes of
        aggregate(); arg (n, C) int32 is the smallest particle id among the accepted candidates whose value is not NaN and equals the
        extremum as an ordered key (-0 below +0), -1 for an empty row or a row of NaNs.  Streams as aggregate()."""
        return self._aggregate_arg(None, values, self._radius(radius), op, self_, fluid_only, delta, counts, device)

    def query_aggregate_arg(self, points, values, radius, op="max", fluid_only=False, counts=False, device: bool = False):
        """The same around query points: arg is (m, C)."""
        return self._aggregate_arg(_device_points4(points, "query_aggregate_arg"), values, radius, op, False, fluid_only, False, counts, device)

    def _aggregate_arg(self, dev_points, values, radius, op, self_, fluid_only, delta, counts, device):
        import torch
        vals = _device_values(values, "aggregate_arg")
        n, c = int(vals.shape[0]), int(vals.shape[1])
        if n != self.GetNumFluids():
            raise SphError(f"aggregate_arg: {n} rows of values for {self.GetNumFluids()} particles")
        cfg = _aggregate_cfg(radius, op, "one", c, self_, fluid_only, delta, False)
        rows = n if dev_points is None else int(dev_points.shape[0])
        written = rows and n                                                          # (nothing is written otherwise: sph_abi.h)
        make = torch.empty if written else torch.zeros
        out = make((rows, c), dtype=torch.float32, device="cuda")
        arg = make((rows, c), dtype=torch.int32, device="cuda")
        cnt = make(rows, dtype=torch.int32, device="cuda") if counts else None
        if not written:
            arg.fill_(-1)
        torch.cuda.current_stream().synchronize()
        self._push_params()
        info = SphAggregateInfo()
        p_cnt = None if cnt is None else _tensor_ptr(cnt)
        if dev_points is None:
            _check(self._L.sph_aggregate_arg_particles(self._h, C.byref(cfg), _tensor_ptr(vals), _tensor_ptr(out), p_cnt, _tensor_ptr(arg), C.byref(info)))
        else:
            _check(self._L.sph_aggregate_arg_query(self._h, C.byref(cfg), _tensor_ptr(dev_points), rows, _tensor_ptr(vals), _tensor_ptr(out), p_cnt,
                                                   _tensor_ptr(arg), C.byref(info)))
        self.sync()
        if not device:
            out, arg = out.cpu().numpy(), arg.cpu().numpy()
            cnt = None if cnt is None else cnt.cpu().numpy().view(np.uint32)
        return (out, cnt, arg) if counts else (out, arg)

    # -- filter-grid basis sums and continuous convolutions (include/sph_abi.h "filter-grid basis sums") ----
    def aggregate_basis(self, x, radius=None, size=4, weight="poly6", self_=False, fluid_only=False, counts=False, device: bool = False):
        """The basis sums of a continuous convolution, A[i][b][c] = sum_j w(r_ij) phi_b(x_j - x_i) x[j][c] over every particle's neighbours
        within `radius` (None: param_h; at most three cells), fused into the grid walk: no edge list.  phi_b are
        the size^3 trilinear hat functions of a size x size x size filter grid over [-radius, radius]^3, b = (z * size + y) * size + x;
        size 2, 3 or 4.  x: (n, C) or (n,) numpy, or a contiguous float32 torch device tensor of (n, C), used in place; 1 <= C <= 128.
        weight "one" | "poly6"; self_ keeps the particle itself (d = 0: the centre of the grid); fluid_only as aggregate().  Returns
        float32 (n, size^3, C), with counts=True (out, counts uint32[n]); numpy, or with device=True fresh torch device tensors.  The
        same bytes on every run.  Streams as aggregate()."""
        return self._basis(None, x, self._radius(radius), size, weight, self_, fluid_only, counts, device)

    def query_aggregate_basis(self, points, x, radius, size=4, weight="poly6", fluid_only=False, counts=False, device: bool = False):
        """The same around (m, 3) or (m, 4) query points: (m, size^3, C).  A point with a non-finite coordinate has an empty row."""
        return self._basis(_device_points4(points, "query_aggregate_basis"), x, radius, size, weight, False, fluid_only, counts, device)

    def _basis(self, dev_points, x, radius, size, weight, self_, fluid_only, counts, device):
        import torch
        vals = _device_values(x, "aggregate_basis")
        n, c = int(vals.shape[0]), int(vals.shape[1])
        if n != self.GetNumFluids():
            raise SphError(f"aggregate_basis: {n} rows of values for {self.GetNumFluids()} particles")
        cfg = _basis_cfg(radius, size, weight, c, self_, fluid_only)
        rows = n if dev_points is None else int(dev_points.shape[0])
        written = rows and n                                                          # (nothing is written otherwise: sph_abi.h)
        out = (torch.empty if written else torch.zeros)((rows, _basis_planes(size), c), dtype=torch.float32, device="cuda")
        cnt = (torch.empty if written else torch.zeros)(rows, dtype=torch.int32, device="cuda") if counts else None
        torch.cuda.current_stream().synchronize()
        self._push_params()
        info = SphAggregateInfo()
        p_out, p_cnt = _tensor_ptr(out), None if cnt is None else _tensor_ptr(cnt)
        if dev_points is None:
            _check(self._L.sph_aggregate_basis_particles(self._h, C.byref(cfg), _tensor_ptr(vals), p_out, p_cnt, C.byref(info)))
        else:
            _check(self._L.sph_aggregate_basis_query(self._h, C.byref(cfg), _tensor_ptr(dev_points), rows, _tensor_ptr(vals), p_out, p_cnt, C.byref(info)))
        self.sync()
        if not device:
            out = out.cpu().numpy()
            cnt = None if cnt is None else cnt.cpu().numpy().view(np.uint32)
        return (out, cnt) if counts else out

    def aggregate_basis_adjoint(self, h, radius=None, size=4, weight="poly6", self_=False, fluid_only=False, device: bool = False):
        """The exact transpose of aggregate_basis() with the same arguments, applied to h of (n, size^3, C): (n, C) float32, row k sums
        coef_b * h[i][b][c] over the rows i that accept particle k, in ascending sorted slot, with the forward's own coefficients.  No
        float atomics, the same bytes on every run.  Streams as aggregate()."""
        return self._basis_adjoint(None, h, self._radius(radius), size, weight, self_, fluid_only, device)

    def query_aggregate_basis_adjoint(self, points, h, radius, size=4, weight="poly6", fluid_only=False, device: bool = False):
        """The transpose of query_aggregate_basis(): h (m, size^3, C) sits on the query points, the result is (n, C); the rows are
        taken in ascending (clamped cell of the point, point index), as query_aggregate_adjoint()."""
        return self._basis_adjoint(_device_points4(points, "query_aggregate_basis_adjoint"), h, radius, size, weight, False, fluid_only, device)

    def _basis_adjoint(self, dev_points, h, radius, size, weight, self_, fluid_only, device):
        import torch
        n = self.GetNumFluids()
        rows = n if dev_points is None else int(dev_points.shape[0])
        if isinstance(h, torch.Tensor) and _is_cuda_f32(h) and h.dim() == 3:
            ht = h
        else:
            ht = torch.from_numpy(_basis_planes_array(h.detach().cpu().numpy() if isinstance(h, torch.Tensor) else h, rows, size, "aggregate_basis_adjoint")).cuda()
        if tuple(ht.shape[:2]) != (rows, _basis_planes(size)):
            raise SphError(f"aggregate_basis_adjoint: h of shape {tuple(ht.shape)} for {rows} rows of {_basis_planes(size)} planes")
        c = int(ht.shape[2])
        cfg = _basis_cfg(radius, size, weight, c, self_, fluid_only)
        out = torch.empty((n, c), dtype=torch.float32, device="cuda")
        torch.cuda.current_stream().synchronize()
        self._push_params()
        info = SphAggregateInfo()
        if dev_points is None:
            _check(self._L.sph_aggregate_basis_adjoint_particles(self._h, C.byref(cfg), _tensor_ptr(ht), _tensor_ptr(out), C.byref(info)))
        else:
            _check(self._L.sph_aggregate_basis_adjoint_query(self._h, C.byref(cfg), _tensor_ptr(dev_points), rows, _tensor_ptr(ht), _tensor_ptr(out), C.byref(info)))
        self.sync()
        return out if device else out.cpu().numpy()

    def aggregate_basis_position_grad(self, x, grad, radius=None, size=4, weight="poly6", self_=False, fluid_only=False, device: bool = False):
        """d/dx of L = sum(grad * aggregate_basis(x, ...)) with the same arguments: (n, 3) float32 by particle id.  x (n, C) as
        aggregate_basis(); grad (n, size^3, C) as aggregate_basis_adjoint() takes its h; numpy, or contiguous float32 torch device tensors
        used in place and never written.  Row k sums, over k's neighbours in ascending sorted slot, the pair terms of both directions
        with the forward's own offsets, weights and cells: no edge list, no float atomics, the same bytes on every
        run.  The hats are differentiated piece by piece: neither their kinks nor the cutoff contribute; self_ changes no byte.
        Streams as aggregate()."""
        return self._basis_posgrad(None, x, grad, self._radius(radius), size, weight, self_, fluid_only, True, True, device)[1]

    def query_aggregate_basis_position_grad(self, points, x, grad, radius, size=4, weight="poly6", fluid_only=False, device: bool = False,
                                            want_points: bool = True, want_particles: bool = True):
        """The same for query_aggregate_basis(points, x, ...): (grad_points (m, 3), grad_particles (n, 3)); grad is (m, size^3, C).
        grad_points row i sums over the row's candidates in the forward's order, grad_particles row k over the points that accept
        particle k in ascending (clamped cell of the point, point index).  want_points / want_particles False: that walk is not launched
        and None stands in its place (not both)."""
        return self._basis_posgrad(_device_points4(points, "query_aggregate_basis_position_grad"), x, grad, radius, size, weight, False, fluid_only,
                                   want_points, want_particles, device)

    def _basis_posgrad(self, dev_points, x, grad, radius, size, weight, self_, fluid_only, want_points, want_particles, device):
        import torch
        vals = _device_values(x, "aggregate_basis_position_grad")
        n, c = int(vals.shape[0]), int(vals.shape[1])
        if n != self.GetNumFluids():
            raise SphError(f"aggregate_basis_position_grad: {n} rows of values for {self.GetNumFluids()} particles")
        rows = n if dev_points is None else int(dev_points.shape[0])
        if isinstance(grad, torch.Tensor) and _is_cuda_f32(grad) and grad.dim() == 3:
            g = grad
        else:
            g = torch.from_numpy(_basis_planes_array(grad.detach().cpu().numpy() if isinstance(grad, torch.Tensor) else grad, rows, size,
                                                     "aggregate_basis_position_grad")).cuda()
        if tuple(g.shape) != (rows, _basis_planes(size), c):
            raise SphError(f"aggregate_basis_position_grad: grad of shape {tuple(g.shape)} for {rows} rows of {_basis_planes(size)} planes and {c} channels")
        cfg = _basis_cfg(radius, size, weight, c, self_, fluid_only)
        out_pts = torch.empty((rows, 3), dtype=torch.float32, device="cuda") if dev_points is not None and want_points else None
        out_par = torch.empty((n, 3), dtype=torch.float32, device="cuda") if want_particles else None
        torch.cuda.current_stream().synchronize()
        self._push_params()
        info = SphAggregateInfo()
        L, h, p = self._L, self._h, C.byref(cfg)
        if dev_points is None:
            _check(L.sph_aggregate_basis_posgrad_particles(h, p, _tensor_ptr(vals), _tensor_ptr(g), _tensor_ptr(out_par), C.byref(info)))
        else:
            # (an output of no rows still goes as a non-null pointer: null means "not wanted")
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr() if t.numel() else _NO_POINT.ctypes.data)
            _check(L.sph_aggregate_basis_posgrad_query(h, p, _tensor_ptr(dev_points), rows, _tensor_ptr(vals), _tensor_ptr(g), ptr(out_pts), ptr(out_par),
                                                       C.byref(info)))
        self.sync()
        if not device:
            out_pts, out_par = (None if t is None else t.cpu().numpy() for t in (out_pts, out_par))
        return out_pts, out_par

    def continuous_conv(self, x, filters, radius=None, weight="poly6", self_=True, fluid_only=False, normalize=False, check_state: bool = True,
                        max_basis_bytes: int = 2 ** 31, positions=None):
        """A continuous convolution (Ummenhofer et al. 2020) of the particles' features over the engine's own neighbourhoods, as a
        torch.autograd.Function: out[i] = sum_j w(r_ij) x[j] @ F(x_j - x_i), F the trilinear interpolation of filters (K, K, K, Cin, Cout)
        (axes z, y, x; K 2, 3 or 4) laid over [-radius, radius]^3.  x: a float32 torch device tensor of (n, Cin); the result is
        (n, Cout).  Once differentiable in x and filters, and with positions= (the (n, 3) tensor of positions(device=True), as
        aggregate_autograd()) in the positions too, through aggregate_basis_position_grad; without the keyword the
        Function, the engine calls and the bytes are those of a call that does not know it.  The basis sums are
        aggregate_basis()'s, in blocks of input channels so that one basis tensor stays under max_basis_bytes (channels are
        independent: the blocking changes no basis byte), and recomputed in the backward rather than saved; their bytes are fixed.  The
        product with the filters is torch's matmul, for which no byte claim is made.  normalize divides by the sum of the weights
        (0 where it is 0).  check_state as aggregate_autograd().  See autograd.py for the formulas."""
        from .autograd import EngineAggregateBackend, continuous_conv
        return continuous_conv(EngineAggregateBackend(self), None, x, filters, self._radius(radius), weight, self_, fluid_only, normalize, check_state,
                               max_basis_bytes, positions=positions)

    def query_continuous_conv(self, points, x, filters, radius, weight="poly6", fluid_only=False, normalize=False, check_state: bool = True,
                              max_basis_bytes: int = 2 ** 31, positions=None, points_grad: bool = False):
        """continuous_conv() around (m, 3) or (m, 4) query points: the result is (m, Cout).  points_grad=True: points must be a float32
        torch device tensor of (m, 3) or (m, 4) and receives the points' gradient (a fourth column gets zeros)."""
        import torch
        from .autograd import EngineAggregateBackend, continuous_conv
        leaf = None
        if points_grad:
            if not isinstance(points, torch.Tensor) or not points.is_cuda or points.dtype != torch.float32 or points.dim() != 2 or int(points.shape[1]) not in (3, 4):
                raise SphError("query_continuous_conv: points_grad takes the query points as a float32 torch device tensor of shape (m, 3) or (m, 4)")
            leaf = points
            flat = points.detach()
            points = flat.contiguous() if int(flat.shape[1]) == 4 else torch.cat([flat, torch.zeros_like(flat[:, :1])], dim=1).contiguous()
        return continuous_conv(EngineAggregateBackend(self), _device_points4(points, "query_continuous_conv"), x, filters, radius, weight, False, fluid_only,
                               normalize, check_state, max_basis_bytes, positions=positions, points_grad=points_grad, points_leaf=leaf)

    # -- iso-surface meshes (include/sph_abi.h "iso-surface") ------------------------------------
    def default_surface_lattice(self):
        """(origin, spacing, dims) of surface()'s default lattice: spacing h/2 over the ComputeGridExtents box widened by 2h on every side."""
        g = self.ComputeGridExtents()
        h = np.float32(self._p.param_h)
        s = np.float32(h / np.float32(2))
        lo = np.array(g.gridMin, np.float32) - np.float32(2) * h
        ext = np.float32(g.cellSize) * np.array(g.dims, np.float32) + np.float32(4) * h
        dims = tuple(int(np.ceil(ext[a] / s)) + 1 for a in range(3))
        return tuple(float(x) for x in lo), (float(s),) * 3, dims

    def _download_surface(self, surf: SphSurface):
        v = np.zeros(surf.numVertices, SURFACE_VERTEX_DTYPE)
        t = np.zeros((surf.numTriangles, 3), np.uint32)
        _check(self._L.sph_surface_download(self._h, _ptr(v), len(v), _ptr(t), len(t)))
        return v, t

    def extract_surface(self, origin, spacing, dims, iso: float = 0.5, field: int = SPH_FIELD_FRACTION) -> SphSurface:
        """sph_extract_surface: counts and borrowed device arrays (valid until the next extract call, ResetSimulation or close)."""
        surf = SphSurface()
        self._push_params()
        _check(self._L.sph_extract_surface(self._h, _f3(origin), _f3(spacing), _dims3(dims), int(field), float(iso), C.byref(surf)))
        return surf

    def surface(self, origin=None, spacing=None, dims=None, iso: float = 0.5, field: int = SPH_FIELD_FRACTION):
        """Iso-surface {field >= iso} of the current state as a closed triangle mesh: (vertices of
        SURFACE_VERTEX_DTYPE, triangles (T, 3) uint32).  Lattice members left None come from default_surface_lattice()."""
        do, ds, dd = self.default_surface_lattice() if origin is None or spacing is None or dims is None else (None, None, None)
        surf = self.extract_surface(do if origin is None else origin, ds if spacing is None else spacing, dd if dims is None else dims, iso, field)
        return self._download_surface(surf)

    def extract_surface_volume(self, dev_values: int, origin, spacing, dims, iso: float = 0.5) -> SphSurface:
        """sph_extract_surface_volume on a device address: counts and borrowed device arrays."""
        surf = SphSurface()
        _check(self._L.sph_extract_surface_volume(self._h, C.c_void_p(dev_values), _f3(origin), _f3(spacing), _dims3(dims), float(iso), C.byref(surf)))
        return surf

    def surface_from_volume(self, values, origin, spacing, dims=None, iso: float = 0.5):
        """Iso-surface {values >= iso} of a caller's lattice of floats (x fastest): a torch CUDA float32 tensor of shape (nz, ny, nx)
        (dims may then be omitted) or a device address with dims = (nx, ny, nz).  Returns (vertices, triangles) like surface()."""
        if hasattr(values, "data_ptr"):
            if not _is_cuda_f32(values):
                raise SphError("surface_from_volume: values must be a contiguous float32 CUDA tensor")
            if dims is None:
                if values.dim() != 3:
                    raise SphError(f"surface_from_volume: a tensor of shape {tuple(values.shape)} needs dims")
                dims = (values.shape[2], values.shape[1], values.shape[0])
            if int(np.prod([int(x) for x in dims])) != values.numel():
                raise SphError(f"surface_from_volume: dims {tuple(dims)} do not match {values.numel()} values")
            ptr = values.data_ptr()
        else:
            if dims is None:
                raise SphError("surface_from_volume: a device address needs dims")
            ptr = int(values)
        surf = self.extract_surface_volume(ptr, origin, spacing, dims, iso)
        return self._download_surface(surf)

    # -- state statistics (include/sph_abi.h "statistics") ----------------------------------------
    def statistics(self, histograms=None) -> Statistics:
        """Counts, extrema, fp64 sums, cell occupancy and up to 4 histograms ((field, bins, lo, hi) with field one of SPH_STAT_*) of the
        current state, reduced on the GPU.  Synchronises."""
        specs, n, words = _histogram_specs(histograms)
        out = SphStatistics()
        hist = np.zeros(words, np.uint64)
        self._push_params()
        _check(self._L.sph_statistics(self._h, C.byref(out), specs, n, _ptr(hist) if n else None))
        hs, at = [], 0
        for i in range(n):
            hs.append(hist[at:at + specs[i].bins + 2].copy())
            at += specs[i].bins + 2
        return Statistics(out, hs, self._p)

    def statistics_device(self, dev_out: int, histograms=None, dev_hist: int = 0):
        """The same into device memory: an 832-byte SphStatistics at dev_out and sum(bins + 2) uint64 at dev_hist (torch tensors'
        data_ptr(), say).  Asynchronous on the engine's stream."""
        specs, n, _ = _histogram_specs(histograms)
        self._push_params()
        _check(self._L.sph_statistics_device(self._h, C.c_void_p(dev_out), specs, n, C.c_void_p(dev_hist) if dev_hist else None))

    # -- passive tracers (include/sph_abi.h "passive tracers") -----------------------------------
    def set_tracers(self, points, integrator: int = SPH_TRACER_MIDPOINT, history: int = 0, stride: int = 1):
        """(m, 3) or (m, 4) points (x, y, z[, initial age]) replace the engine's tracer set: every substep from now on advects them
        with the fluid's Shepard velocity and keeps the `history` newest snapshots, one every `stride`
        substeps, on the device.  Synchronises."""
        p4 = _points4(points, "set_tracers", keep_w=True)
        _check(self._L.sph_tracers_set(self._h, _ptr(p4), len(p4), int(integrator), int(history), int(stride)))

    def set_tracers_device(self, dev_points: int, m: int, integrator: int = SPH_TRACER_MIDPOINT, history: int = 0, stride: int = 1):
        """The same from m points of 4 floats at device address dev_points.  Asynchronous on the engine's stream."""
        _check(self._L.sph_tracers_set_device(self._h, C.c_void_p(dev_points), int(m), int(integrator), int(history), int(stride)))

    def clear_tracers(self):
        _check(self._L.sph_tracers_set(self._h, None, 0, SPH_TRACER_EULER, 0, 1))

    def num_tracers(self) -> int:
        return int(self._L.sph_tracers_count(self._h))

    def tracer_info(self):
        """(substeps that advected the current set, stored snapshots, number of the oldest stored snapshot)."""
        c, n, q = C.c_uint64(), C.c_uint32(), C.c_uint64()
        _check(self._L.sph_tracers_info(self._h, C.byref(c), C.byref(n), C.byref(q)))
        return int(c.value), int(n.value), int(q.value)

    def tracers(self) -> np.ndarray:
        """The tracers in the caller's order: a structured array of TRACER_DTYPE (pos, age, vel, fraction).  Synchronises."""
        out = np.zeros(self.num_tracers(), TRACER_DTYPE)
        _check(self._L.sph_tracers_download(self._h, _ptr(out), len(out)))
        return out

    def tracers_device(self) -> int:
        """Borrowed device address of the 32-byte records in the caller's order (0 without tracers); valid until the next
        dispatch, set, reset or close.  No synchronisation."""
        p = C.c_void_p()
        _check(self._L.sph_tracers_device(self._h, C.byref(p)))
        return int(p.value or 0)

    # -- spray, foam and bubbles (include/sph_abi.h "spray, foam and bubbles") --------------------
    def set_diffuse(self, config=None, **overrides):
        """Switch secondary particles on: config is a SphDiffuseConfig (diffuse_config()) or None for the
        defaults, overrides name its fields.  The capacity of the pool in place keeps the pool and replaces the coefficients."""
        cfg = diffuse_config(**overrides) if config is None else _copy_config(config, overrides)
        _check(self._L.sph_diffuse_set(self._h, C.byref(cfg)))

    def clear_diffuse(self):
        _check(self._L.sph_diffuse_set(self._h, None))

    def diffuse_config(self) -> "SphDiffuseConfig":
        """The config in force (capacity 0 without a pool)."""
        cfg = SphDiffuseConfig()
        _check(self._L.sph_diffuse_get(self._h, C.byref(cfg)))
        return cfg

    def diffuse_info(self) -> dict:
        """Counter, alive count and running totals of the pool as a dict of ints (aliveByKind: a list).  Synchronises."""
        info = SphDiffuseInfo()
        _check(self._L.sph_diffuse_info(self._h, C.byref(info)))
        return _info_dict(info)

    def diffuse(self) -> np.ndarray:
        """The living records in pool order: a structured array of DIFFUSE_DTYPE.  Synchronises."""
        out = np.zeros(max(int(self.diffuse_config().capacity), 1), DIFFUSE_DTYPE)
        n = C.c_size_t()
        _check(self._L.sph_diffuse_download(self._h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def diffuse_device(self):
        """(records, aliveCountWord): borrowed device addresses of the 48-byte records and of the alive count (0, 0 without a pool)."""
        r, a = C.c_void_p(), C.c_void_p()
        _check(self._L.sph_diffuse_device(self._h, C.byref(r), C.byref(a)))
        return int(r.value or 0), int(a.value or 0)

    def seed_diffuse(self, records):
        """Caller-made DIFFUSE_DTYPE records behind the living ones, taken as they are.  Synchronises."""
        rec = np.ascontiguousarray(records, DIFFUSE_DTYPE)
        _check(self._L.sph_diffuse_seed(self._h, _ptr_or_none(rec), len(rec)))

    def set_diffuse_crest(self, config=None, **overrides):
        """Switch the pool's crest births on: config is a SphDiffuseCrest (diffuse_crest_config()) or None for
        the defaults, overrides name its fields.  rate 0 switches the term off.  Needs a pool (set_diffuse)."""
        cfg = diffuse_crest_config(**overrides) if config is None else _copy_config(config, overrides)
        self._push_params()                                                             # (the radius is checked against their grid)
        _check(self._L.sph_diffuse_set_crest(self._h, C.byref(cfg)))

    def clear_diffuse_crest(self):
        _check(self._L.sph_diffuse_set_crest(self._h, None))

    def diffuse_crest(self) -> "SphDiffuseCrest":
        """The crest config in force (all zero while the term is off)."""
        cfg = SphDiffuseCrest()
        _check(self._L.sph_diffuse_get_crest(self._h, C.byref(cfg)))
        return cfg

    def diffuse_crest_info(self) -> dict:
        """The books of the crest term: acting substeps, crest children, the shell size of the last acting substep, whether the term
        is on, the radius and stencil in force.  Synchronises."""
        info = SphDiffuseCrestInfo()
        _check(self._L.sph_diffuse_crest_info(self._h, C.byref(info)))
        return _crest_info_dict(info)

    def tracer_history(self):
        """(first, array (count, M, 4)): the stored snapshots (x, y, z, age), oldest first, and the number of the first one.  Synchronises."""
        _, n, _ = self.tracer_info()
        out = np.zeros((max(n, 1), self.num_tracers(), 4), np.float32)
        cnt, first = C.c_uint32(), C.c_uint64()
        _check(self._L.sph_tracers_history(self._h, _ptr(out), out.shape[0], C.byref(cnt), C.byref(first)))
        return int(first.value), out[:cnt.value]

    # -- diffusing scalar fields (include/sph_abi.h "diffusing scalar fields") --
    def set_scalars(self, values=None, diffusivity=0.0, decay=0.0, channels: int | None = None):
        """(n,) or (n, K) values replace the engine's scalar channels; values=None seeds channel 0 from padB of the records (the
        reference's dye) and the others with 0 (`channels`, default 1).  diffusivity / decay: one number or K of them.  Synchronises."""
        if values is None:
            k = 1 if channels is None else int(channels)
            co = _scalar_coeffs(max(k, 1), diffusivity, decay)
            _check(self._L.sph_scalars_set(self._h, None, self.GetNumFluids(), k, co.ctypes.data_as(_pf)))   # (the engine's count: a reset may spawn fewer than numParticles)
            return
        v = _scalar_values(values)
        co = _scalar_coeffs(max(v.shape[1], 1), diffusivity, decay)
        _check(self._L.sph_scalars_set(self._h, _ptr(v), len(v), v.shape[1], co.ctypes.data_as(_pf)))

    def set_scalars_device(self, dev_values: int, n: int, channels: int, diffusivity=0.0, decay=0.0):
        """The same from a device address of n * channels floats, asynchronous on the engine's stream."""
        co = _scalar_coeffs(max(int(channels), 1), diffusivity, decay)
        _check(self._L.sph_scalars_set_device(self._h, C.c_void_p(dev_values), int(n), int(channels), co.ctypes.data_as(_pf)))

    def set_scalar_coefficients(self, diffusivity=0.0, decay=0.0):
        """New D_k and lambda_k for the current channels, stream-ordered (replayed graphs see them)."""
        co = _scalar_coeffs(max(self.num_scalar_channels(), 1), diffusivity, decay)
        _check(self._L.sph_scalars_set_coefficients(self._h, co.ctypes.data_as(_pf)))

    def clear_scalars(self):
        _check(self._L.sph_scalars_set(self._h, None, 0, 0, None))

    def num_scalar_channels(self) -> int:
        return int(self._L.sph_scalars_channels(self._h))

    def scalars(self) -> np.ndarray:
        """The values in the caller's order, shape (n, K) float32.  Synchronises."""
        k = self.num_scalar_channels()
        out = np.zeros((self.GetNumFluids() if k else 0, k), np.float32)
        _check(self._L.sph_scalars_download(self._h, _ptr(out), out.size))
        return out

    def scalars_device(self) -> int:
        """Borrowed device address of the n * K floats (0 without scalars); valid until the next dispatch, set, reset or close."""
        p = C.c_void_p()
        _check(self._L.sph_scalars_device(self._h, C.byref(p)))
        return p.value or 0

    def paint_scalar(self, center, radius: float, value: float, channel: int = 0, mode: int = SPH_SCALAR_SET):
        """channel = value (SPH_SCALAR_SET) or += value (SPH_SCALAR_ADD) for every non-ghost particle strictly inside the sphere."""
        _check(self._L.sph_scalars_paint(self._h, _f3(center), float(radius), int(channel), float(value), int(mode)))

    def scalar_info(self):
        """(substeps stepped since set_scalars, diffusion number of the last one).  Synchronises."""
        c, s = C.c_uint64(), C.c_float()
        _check(self._L.sph_scalars_info(self._h, C.byref(c), C.byref(s)))
        return int(c.value), np.float32(s.value)

    def scalar_moments(self):
        """One ScalarMoments per channel (count, fp64 sums in the statistics' fixed order, extrema with ids).  Synchronises."""
        out = (SphScalarMoments * SPH_MAX_SCALAR_CHANNELS)()
        self._push_params()
        _check(self._L.sph_scalars_moments(self._h, C.byref(out)))
        return [ScalarMoments(out[k]) for k in range(self.num_scalar_channels())]

    def sample_scalar(self, points, channel: int = 0) -> np.ndarray:
        """Shepard value of a channel at (m, 3) or (m, 4) probe points: (m,) float32.  Synchronises."""
        p4 = _points4(points, "sample_scalar", keep_w=False)
        out = np.zeros(len(p4), np.float32)
        self._push_params()
        _check(self._L.sph_scalars_sample_points(self._h, _ptr(p4), len(p4), int(channel), _ptr(out)))
        return out

    def sample_scalar_device(self, dev_points: int, m: int, dev_out: int, channel: int = 0):
        self._push_params()
        _check(self._L.sph_scalars_sample_points_device(self._h, C.c_void_p(dev_points), int(m), int(channel), C.c_void_p(dev_out)))

    def scalar_lattice_device(self, origin, spacing, dims, dev_out: int, channel: int = 0):
        """Shepard value of a channel on the lattice origin + i * spacing (x fastest) into a device buffer of one float per point; it
        feeds extract_surface_volume / surface_from_volume unchanged.  Asynchronous on the engine's stream."""
        self._push_params()
        _check(self._L.sph_scalars_sample_lattice(self._h, _f3(origin), _f3(_spacing3(spacing)), _dims3(dims, "scalar_lattice"), int(channel),
                                                  C.c_void_p(dev_out)))

    def scalar_lattice(self, origin, spacing, dims, channel: int = 0, device: bool = False):
        """scalar_lattice_device into a fresh torch CUDA tensor of shape (nz, ny, nx); device=False returns its host copy (numpy)."""
        import torch
        nx, ny, nz = (int(x) for x in dims)
        _dims3(dims, "scalar_lattice")
        buf = torch.empty((nz, ny, nx), dtype=torch.float32, device="cuda")
        self.scalar_lattice_device(origin, spacing, (nx, ny, nz), buf.data_ptr(), channel)
        self.sync()
        return buf if device else buf.cpu().numpy()

    # -- active scalars: buoyancy and continuous sources (include/sph_abi.h "active scalars") --
    def set_scalar_buoyancy(self, beta=None, ref=0.0):
        """beta_k and ref_k per channel (a scalar is every channel's value); beta=None switches the kick off.  Every substep from now
        on adds -(dt sum_k beta_k (c_k - ref_k)) g to the velocity of every fluid particle.  No synchronisation."""
        b, r = _buoyancy(max(self.num_scalar_channels(), 1), beta, ref)
        _check(self._L.sph_scalars_set_buoyancy(self._h, None if b is None else b.ctypes.data_as(_pf), None if r is None else r.ctypes.data_as(_pf)))

    def scalar_buoyancy(self):
        """(beta, ref): two float32 arrays of K values as set (zeros while off)."""
        k = self.num_scalar_channels()
        b, r = np.zeros(max(k, 1), np.float32), np.zeros(max(k, 1), np.float32)
        _check(self._L.sph_scalars_get_buoyancy(self._h, b.ctypes.data_as(_pf), r.ctypes.data_as(_pf)))
        return b[:k], r[:k]

    def set_scalar_sources(self, sources=()):
        """Replace the source table (a list of scalar_source() results or a SOURCE_DTYPE array; empty clears it).  No synchronisation."""
        arr = source_array(sources)
        _check(self._L.sph_scalars_set_sources(self._h, _ptr_or_none(arr), len(arr)))

    def scalar_sources(self) -> np.ndarray:
        """The sources as set, a SOURCE_DTYPE array."""
        out = np.zeros(SPH_MAX_SCALAR_SOURCES, SOURCE_DTYPE)
        k = C.c_int()
        _check(self._L.sph_scalars_get_sources(self._h, _ptr(out), len(out), C.byref(k)))
        return out[:k.value].copy()

    def scalar_injected(self, reset: bool = False):
        """(sums, hits, time, substeps): per source the fp64 sum of c' - c and the (particle, substep) hits since the last zeroing, the
        simulated time and the substeps over which they were summed; reset zeroes them after the read.  Synchronises."""
        sums, hits = np.zeros(SPH_MAX_SCALAR_SOURCES, np.float64), np.zeros(SPH_MAX_SCALAR_SOURCES, np.uint64)
        t, n = C.c_double(), C.c_uint64()
        _check(self._L.sph_scalars_injected(self._h, _ptr(sums), _ptr(hits), SPH_MAX_SCALAR_SOURCES, C.byref(t), C.byref(n), 1 if reset else 0))
        k = len(self.scalar_sources())
        return sums[:k].copy(), hits[:k].copy(), float(t.value), int(n.value)

    # -- flow gates (include/sph_abi.h "flow gates") ----------------------
    def set_gates(self, gates, history: int = 0, stride: int = 1):
        """Replace the gate table (a list of gate() results or a GATE_DTYPE array; empty clears it).  Every substep from now on books
        what crosses each gate; with history > 0 the cumulative books go into a ring row on the device every `stride` substeps.
        Another count, history or stride zeroes books and ring.  No synchronisation."""
        arr = gate_array(gates)
        _check(self._L.sph_gates_set(self._h, _ptr_or_none(arr), len(arr), int(history), int(stride)))

    def clear_gates(self):
        _check(self._L.sph_gates_set(self._h, None, 0, 0, 1))

    def _gates_info(self):
        k, h, s = C.c_int(), C.c_uint32(), C.c_uint32()
        _check(self._L.sph_gates_get(self._h, None, 0, C.byref(k), C.byref(h), C.byref(s)))
        return k.value, h.value, s.value

    def gates(self) -> np.ndarray:
        """The gates as set, a GATE_DTYPE array."""
        out = np.zeros(SPH_MAX_GATES, GATE_DTYPE)
        k = C.c_int()
        _check(self._L.sph_gates_get(self._h, _ptr(out), len(out), C.byref(k), None, None))
        return out[:k.value].copy()

    def gate_books(self, reset: bool = False):
        """(rows, time, substeps): per gate the books (GATE_BOOKS_DTYPE: forward, backward, vel, scalar) since the last zeroing, the
        simulated time and the substeps over which they were summed; reset zeroes them after the read.  Synchronises."""
        rows = np.zeros(SPH_MAX_GATES, GATE_BOOKS_DTYPE)
        t, n = C.c_double(), C.c_uint64()
        _check(self._L.sph_gates_books(self._h, _ptr(rows), C.byref(t), C.byref(n), 1 if reset else 0))
        return rows[:self._gates_info()[0]].copy(), float(t.value), int(n.value)

    def gate_history(self):
        """(first, rows (count, gates) GATE_BOOKS_DTYPE, times (count,)): the stored ring rows, oldest first, and the index of the first
        one (row i was taken after (first + i + 1) * stride substeps).  Synchronises."""
        k, h, _ = self._gates_info()
        rows, times = np.zeros((max(h, 1), max(k, 1)), GATE_BOOKS_DTYPE), np.zeros(max(h, 1), np.float64)
        first, cnt = C.c_uint64(), C.c_uint32()
        _check(self._L.sph_gates_history(self._h, C.byref(first), C.byref(cnt), _ptr(rows.reshape(-1)), _ptr(times)))
        return int(first.value), rows.reshape(-1)[:cnt.value * k].reshape(cnt.value, k).copy(), times[:cnt.value].copy()

    # -- field monitors (include/sph_abi.h "field monitors") ----------------
    def set_monitor(self, points=None, *, lattice=None, slot: int = 0, every: int = 1, wet_fraction: float = 0.5, history: int = 0,
                    stride: int = 1, ring_points=None):
        """Set monitor `slot` to explicit points ((m, 3) or (m, 4), numpy or a (m, 4) float32 torch device tensor) or to
        lattice=(origin, spacing, dims) with dims = (nx, ny, nz).  From now on every `every`-th substep adds, inside the substep, the
        sample() of each point to the point's running sums; with history > 0 every `stride`-th of them also stores the raw samples of
        the first ring_points points (None: min(M, 64)) in a ring on the device.  A set call restarts the slot."""
        if (points is None) == (lattice is None):
            raise SphError("set_monitor: give either points or lattice=(origin, spacing, dims)")
        cfg = monitor_config(every=int(every), wetFraction=float(wet_fraction), history=int(history), stride=int(stride),
                             ringPoints=0 if ring_points is None else int(ring_points))
        self._push_params()
        if lattice is not None:
            origin, spacing, dims = lattice
            _check(self._L.sph_monitor_set_lattice(self._h, int(slot), _f3(origin), _f3(_spacing3(spacing)), _dims3(dims), C.byref(cfg)))
            return
        if type(points).__module__.startswith("torch"):
            dev = _device_points4(points, "set_monitor")
            _check(self._L.sph_monitor_set_device(self._h, int(slot), C.c_void_p(dev.data_ptr()), len(dev), C.byref(cfg)))
            return
        p4 = _points4(points, "set_monitor", keep_w=False)
        _check(self._L.sph_monitor_set(self._h, int(slot), _ptr_or_none(p4), len(p4), C.byref(cfg)))

    def monitor_info(self, slot: int = 0) -> dict:
        """What the slot holds as a dict: kind (SPH_MONITOR_NONE for an empty slot), dims, points, the config as set (every,
        wetFraction, history, stride, ringPoints), substeps, acting, time, ringRows, firstRow, origin, spacing.  Synchronises."""
        info = SphMonitorInfo()
        _check(self._L.sph_monitor_info(self._h, int(slot), C.byref(info)))
        out = {name: int(getattr(info, name)) for name in ("kind", "points", "substeps", "acting", "firstRow", "ringRows")}
        out.update({name: int(getattr(info.config, name)) for name in ("every", "history", "stride", "ringPoints")})
        out.update(wetFraction=float(info.config.wetFraction), time=float(info.time), dims=tuple(int(x) for x in info.dims),
                   origin=tuple(float(x) for x in info.origin), spacing=tuple(float(x) for x in info.spacing))
        return out

    def monitor_rows(self, slot: int = 0, device: bool = False):
        """The rows of the slot in the caller's order: a MONITOR_ROW_DTYPE array, of shape (nz, ny, nx) for a lattice; with
        device=True the borrowed device address of the 128-byte rows (no synchronisation, no copy)."""
        if device:
            p = C.c_void_p()
            _check(self._L.sph_monitor_device(self._h, int(slot), C.byref(p)))
            return int(p.value or 0)
        info = self.monitor_info(slot)
        out = np.zeros(info["points"], MONITOR_ROW_DTYPE)
        _check(self._L.sph_monitor_download(self._h, int(slot), _ptr_or_none(out), len(out)))
        return out.reshape(info["dims"][::-1]) if info["kind"] == SPH_MONITOR_LATTICE else out

    def monitor_history(self, slot: int = 0):
        """(first, samples (rows, ringPoints) SAMPLE_DTYPE, times (rows,)): the ring rows held, oldest first, the fp64 time of the state
        each was sampled on, and the index of the first one (ring row r was written by acting substep r * stride).  Synchronises."""
        info = self.monitor_info(slot)
        cap, rp = max(info["history"], 1), info["ringPoints"]
        samples, times = np.zeros((cap, max(rp, 1)), SAMPLE_DTYPE), np.zeros(cap, np.float64)
        first, cnt = C.c_uint64(), C.c_uint32()
        _check(self._L.sph_monitor_history(self._h, int(slot), C.byref(first), C.byref(cnt), _ptr(samples.reshape(-1)), _ptr(times), cap))
        return int(first.value), samples.reshape(-1)[:cnt.value * rp].reshape(cnt.value, rp).copy(), times[:cnt.value].copy()

    def monitor_field(self, field: int, slot: int = 0, device: bool = False):
        """A derived field (SPH_MONITOR_*) of the slot: M float32, of shape (nz, ny, nx) for a lattice (surface_from_volume takes it as
        it is); a numpy array, or with device=True a torch device tensor (asynchronous on the engine's stream)."""
        import torch
        info = self.monitor_info(slot)
        shape = info["dims"][::-1] if info["kind"] == SPH_MONITOR_LATTICE else (info["points"],)
        buf = torch.empty(shape, dtype=torch.float32, device="cuda")
        _check(self._L.sph_monitor_field(self._h, int(slot), int(field), C.c_void_p(buf.data_ptr())))
        if device:
            return buf
        self.sync()
        return buf.cpu().numpy()

    def reset_monitor(self, slot: int = 0):
        """Zero rows, counters and ring of the slot on the stream and keep its buffers: averaging begins anew (after a spin-up, say)."""
        _check(self._L.sph_monitor_reset(self._h, int(slot)))

    def clear_monitor(self, slot=None):
        """Drop the monitor of one slot, or (None) of every slot."""
        _check(self._L.sph_monitor_clear(self._h, -1 if slot is None else int(slot)))

    # -- kinematic solid obstacles (include/sph_abi.h "obstacles") -------------------------------
    def set_obstacles(self, obstacles):
        """Replace the set of bodies (a list of obstacle() results or an OBSTACLE_DTYPE array; empty clears it).  Every substep from
        now on keeps the fluid out of them, advances their poses and sums the fluid's impulses.  No synchronisation."""
        arr = obstacle_array(obstacles)
        _check(self._L.sph_obstacles_set(self._h, _ptr_or_none(arr), len(arr)))

    def clear_obstacles(self):
        _check(self._L.sph_obstacles_set(self._h, None, 0))

    def set_obstacle_motion(self, index: int, vel, omega):
        """New linear / angular velocity of body `index`; the pose stays the one the device holds.  No synchronisation."""
        _check(self._L.sph_obstacles_set_motion(self._h, int(index), _f3(vel), _f3(omega)))

    def obstacles(self) -> np.ndarray:
        """The bodies with their current (advanced) poses, an OBSTACLE_DTYPE array.  Synchronises."""
        out = np.zeros(SPH_MAX_OBSTACLES, OBSTACLE_DTYPE)
        k = C.c_int()
        _check(self._L.sph_obstacles_get(self._h, _ptr(out), len(out), C.byref(k)))
        return out[:k.value].copy()

    def obstacle_impulses(self, reset: bool = False):
        """(J, time, substeps): J (K, 6) float64 = (Jx, Jy, Jz, Lx, Ly, Lz) the fluid gave each body since the last zeroing, the
        simulated time and the substeps over which they were summed; reset zeroes them after the read.  Synchronises."""
        out = np.zeros((SPH_MAX_OBSTACLES, 6), np.float64)
        t, n = C.c_double(), C.c_uint64()
        _check(self._L.sph_obstacles_impulses(self._h, _ptr(out), SPH_MAX_OBSTACLES, C.byref(t), C.byref(n), 1 if reset else 0))
        return out[:len(self.obstacles())].copy(), float(t.value), int(n.value)

    # -- triangle-mesh obstacles through signed distance lattices (include/sph_abi.h "signed distance lattices") --------
    def create_volume(self, values, spacing) -> int:
        """A volume from signed distances (negative inside) of shape (nz, ny, nx): a numpy array or a contiguous float32 torch CUDA tensor.
        spacing is a scalar or (sx, sy, sz).  Returns the volume's id."""
        vid = C.c_int(-1)
        if hasattr(values, "data_ptr"):
            if not _is_cuda_f32(values) or values.dim() != 3:
                raise SphError("create_volume: values must be a contiguous float32 CUDA tensor of shape (nz, ny, nx)")
            _check(self._L.sph_volume_create(self._h, C.c_void_p(values.data_ptr()), _dims3(values.shape[::-1]), _f3(_spacing3(spacing)), 1, C.byref(vid)))
        else:
            v, dims, sp = _volume_lattice(values, spacing)
            _check(self._L.sph_volume_create(self._h, _ptr(v), dims, _f3(sp), 0, C.byref(vid)))
        return int(vid.value)

    def destroy_volume(self, volume_id: int):
        _check(self._L.sph_volume_destroy(self._h, int(volume_id)))

    def volume_info(self, volume_id: int):
        """(dims (nx, ny, nz), spacing[3], half[3]) of a volume; half is the box size that covers the lattice exactly."""
        d, sp, hf = (C.c_int * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
        _check(self._L.sph_volume_info(self._h, int(volume_id), d, sp, hf))
        return tuple(d), np.array(sp, np.float32), np.array(hf, np.float32)

    def bind_obstacle_volume(self, index: int, volume_id: int):
        """Body `index` (a box) takes its shape from the volume (volume_id < 0 unbinds).  set_obstacles clears every binding."""
        _check(self._L.sph_obstacles_bind_volume(self._h, int(index), int(volume_id)))

    def obstacle_volume(self, index: int) -> int:
        vid = C.c_int(-1)
        _check(self._L.sph_obstacles_volume(self._h, int(index), C.byref(vid)))
        return int(vid.value)

    def mesh_distance(self, vertices, triangles, origin, spacing, dims):
        """Signed distance (negative inside) from the lattice points origin + i * spacing, dims = (nx, ny, nz), to a closed triangle mesh
        (counter-clockwise seen from outside): a float32 torch CUDA tensor of shape (nz, ny, nx).  Asynchronous on the engine's stream."""
        import torch
        v, t = _mesh_arrays(vertices, triangles)
        d = _dims3(dims, "mesh_distance")
        sp = _spacing3(spacing)
        out = torch.empty((int(d[2]), int(d[1]), int(d[0])), dtype=torch.float32, device="cuda")
        _check(self._L.sph_mesh_distance(self._h, _ptr(v), len(v), _ptr(t), len(t), _f3(origin), _f3(sp), d, C.c_void_p(out.data_ptr())))
        self.sync()                                                      # (the tensor is handed to the caller's own stream)
        return out

    def volume_from_mesh(self, vertices, triangles, spacing: float, margin: float = 2.0):
        """A volume around a mesh: a lattice of the given spacing about the mesh's bounding box widened by `margin` spacings on every side.
        Returns (id, center, half): obstacle(SPH_OBSTACLE_BOX, center, half) + bind_obstacle_volume(index, id) is the whole recipe."""
        v, t = _mesh_arrays(vertices, triangles)
        if not len(v):
            raise SphError("volume_from_mesh: no vertices")
        h = np.float32(spacing)
        lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
        dims = [max(2, int(math.ceil((hi[a] - lo[a]) / float(h) + 2.0 * margin)) + 1) for a in range(3)]
        center = (0.5 * (lo + hi)).astype(np.float32)
        vid = C.c_int(-1)
        _check(self._L.sph_volume_from_mesh(self._h, _ptr(v), len(v), _ptr(t), len(t), _f3(center), _f3((h, h, h)), _dims3(dims), C.byref(vid)))
        return int(vid.value), center, self.volume_info(vid.value)[2]

    # -- dynamic rigid bodies (include/sph_abi.h "dynamic rigid bodies") -------------------------------
    def set_obstacle_dynamics(self, index: int, record=None):
        """Body `index` moves under the fluid's impulses, gravity and the container from the next substep on (a dynamics() record; None:
        kinematic again).  Stream-ordered; a replayed graph sees it.  set_obstacles clears every record."""
        _check(self._L.sph_obstacles_set_dynamics(self._h, int(index), C.byref(record) if record is not None else None))

    def obstacle_dynamics(self, index: int):
        """The record of body `index` as set, or None for a kinematic body."""
        out, on = SphObstacleDynamics(), C.c_int()
        _check(self._L.sph_obstacles_get_dynamics(self._h, int(index), C.byref(out), C.byref(on)))
        return out if on.value else None

    def volume_moments(self, volume_id: int) -> np.ndarray:
        """The ten moments of the solid a volume describes (sph_volume_moments): cell volume times the weighted sums of
        1, x, y, z, xx, yy, zz, xy, xz, yz.  Synchronises."""
        out = np.zeros(10, np.float64)
        _check(self._L.sph_volume_moments(self._h, int(volume_id), _ptr(out)))
        return out

    def volume_mass_properties(self, volume_id: int, density: float):
        """(mass, centre of mass in the body frame, inertia about it as xx, yy, zz, xy, xz, yz) of a homogeneous body shaped by the volume."""
        return mass_properties(self.volume_moments(volume_id), density)

    # -- measurement (include/sph_abi.h "measurement") and the end of the engine's life ---------------------------
    def kernel_times(self, reset: bool = False):
        ms = (C.c_double * len(KERNEL_CLASSES))()
        cnt = (C.c_int64 * len(KERNEL_CLASSES))()
        _check(self._L.sph_kernel_times(self._h, ms, cnt, 1 if reset else 0))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(KERNEL_CLASSES)}

    # -- checkpoints (include/sph_abi.h "checkpoints") ---------------------------------------
    def save_state(self, path=None) -> np.ndarray:
        """The engine's state as a blob (a uint8 array), written to `path` too if one is given.  Synchronises; the members are pushed
        first, as before a dispatch, so the blob carries the values the next substep would have read."""
        self._push_members()
        need = C.c_size_t(0)
        _check(self._L.sph_state_size(self._h, C.byref(need)))
        blob = np.zeros(need.value, np.uint8)
        _check(self._L.sph_state_save(self._h, _ptr(blob), blob.size, C.byref(need)))
        if path is not None:
            blob.tofile(path)
        return blob

    def load_state(self, blob_or_path):
        """Make this engine what the saved one was (whatever it held before), and refresh every host-side mirror of the class: the
        param_*, fountain* and river members with the heightfield, numParticles, stencilCount.  SphError on a bad blob: the engine is
        then unchanged."""
        blob = _state_blob(blob_or_path)
        info = SphStateInfo()
        _check(self._L.sph_state_peek(_ptr(blob), blob.size, C.byref(info)))         # (where the heightfield lies, from the library: no offsets by hand)
        _check(self._L.sph_state_load(self._h, _ptr(blob), blob.size))
        _check(self._L.sph_get_params(self._h, C.byref(self._p)))
        _check(self._L.sph_get_fountain(self._h, C.byref(self._f)))
        _check(self._L.sph_get_river(self._h, C.byref(self._r)))
        at = int(info.terrainOffset)
        self.terrainHeights = blob[at:at + 4 * int(info.terrainCount)].view(np.float32).copy()
        self._terrain_sent = self.terrainHeights                     # (the library holds exactly these)
        self.stencilCount = int(info.stencilCount)
        self.numParticles = self.GetNumFluids()

    @classmethod
    def from_state(cls, blob_or_path, stream: int | None = None) -> "SPHFluidGPU":
        """A new engine that continues the saved run: created from the blob's particle count and params, then loaded."""
        blob = _state_blob(blob_or_path)
        info = state_info(blob)
        f = cls(1, params=info["params"], stream=stream, _particles=np.zeros(1, PARTICLE_DTYPE))     # (the load re-sizes it)
        f.load_state(blob)
        return f

    def state_digest(self, sections=None) -> dict:
        """name -> (lo, hi) of the sections the engine holds (sections: names, or None for all): their checksums computed on the device,
        by definition what a blob saved now stores for them.  Synchronises."""
        self._push_members()
        mask = 0
        for name in (sections or ()):
            mask |= 1 << STATE_SECTIONS.index(name)
        d = SphStateDigest()
        _check(self._L.sph_state_digest(self._h, mask, C.byref(d)))
        return {name: (int(d.sum[i][0]), int(d.sum[i][1])) for i, name in enumerate(STATE_SECTIONS) if d.sections & (1 << i)}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.sph_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- host-only functions (no device is needed), in the order of include/sph_abi.h ------------------------------------------
def default_params(**overrides) -> SphParams:
    p = SphParams()
    _check(load_library().sph_params_default(C.byref(p)))
    for k, v in overrides.items():
        _assign(p, k, v)
    return p


def compute_grid_extents(p: SphParams) -> SphGridInfo:
    g = SphGridInfo()
    _check(load_library().sph_compute_grid_extents(C.byref(p), C.byref(g)))
    return g


def rotation_mat3(euler_deg) -> np.ndarray:
    out = (C.c_float * 9)()
    _check(load_library().sph_rotation_mat3(_f3(euler_deg), out))
    return np.array(out, np.float32)


def effective_half(p: SphParams) -> np.ndarray:
    out = (C.c_float * 3)()
    _check(load_library().sph_effective_half(C.byref(p), out))
    return np.array(out, np.float32)


def spawn_particles(p: SphParams, n_requested: int, seed: int):
    buf = np.zeros(max(n_requested, 1), PARTICLE_DTYPE)
    n = C.c_size_t()
    mass = C.c_float()
    _check(load_library().sph_spawn_particles(C.byref(p), n_requested, seed, _ptr(buf), C.byref(n), C.byref(mass)))
    return buf[: n.value].copy(), float(mass.value)


def default_river(**kw) -> SphRiver:
    r = SphRiver()
    load_library().sph_river_default(C.byref(r))
    for k, v in kw.items():
        _assign(r, k, v)
    return r


def generate_river_terrain(p: SphParams, seed: int, river: SphRiver | None = None):
    """GenerateRiverTerrain (SPHFluid3D.cpp:772-878) as a pure host function: fills `river`, returns (river, heights);
    writes param_gravityY / Z of `p` like the reference."""
    r = river if river is not None else default_river()
    heights = np.zeros(r.terrainW * r.terrainH, np.float32)
    _check(load_library().sph_generate_river_terrain(C.byref(p), int(seed), C.byref(r), _ptr(heights)))
    return r, heights


def spawn_river_particles(p: SphParams, river: SphRiver, heights: np.ndarray, n_requested: int, seed: int):
    """The river branch of InitializeParticles (SPHFluid3D.cpp:104-160)."""
    h = np.ascontiguousarray(heights, np.float32)
    buf = np.zeros(max(n_requested, 1), PARTICLE_DTYPE)
    n = C.c_size_t()
    mass = C.c_float()
    _check(load_library().sph_spawn_river_particles(C.byref(p), C.byref(river), _ptr(h), n_requested, seed, _ptr(buf), C.byref(n), C.byref(mass)))
    return buf[: n.value].copy(), float(mass.value)


def gauge_levels(frac: np.ndarray, ys: np.ndarray, threshold: float = 0.5) -> np.ndarray:
    """The rule of SPHFluidGPU.water_level on fraction columns frac[c, k] sampled at heights ys[k] (descending): the first sample
    from the top with fraction >= threshold, interpolated linearly against the sample above it (that sample itself when it is the
    topmost one); NaN where no sample reaches the threshold."""
    frac = np.asarray(frac, np.float64)
    ys = np.asarray(ys, np.float64)
    out = np.full(frac.shape[0], np.nan)
    for c in range(frac.shape[0]):
        hit = np.nonzero(frac[c] >= threshold)[0]
        if len(hit) == 0:
            continue
        k = int(hit[0])
        if k == 0:
            out[c] = ys[0]
            continue
        f0, f1 = frac[c, k - 1], frac[c, k]            # above (below threshold), at / over the threshold
        out[c] = ys[k] + (ys[k - 1] - ys[k]) * (f1 - threshold) / (f1 - f0)
    return out


def write_ply(path, vertices: np.ndarray, triangles: np.ndarray) -> None:
    """Binary little-endian PLY of a surface: x, y, z, nx, ny, nz per vertex (SURFACE_VERTEX_DTYPE), 3 uint32 indices per face."""
    v = np.ascontiguousarray(vertices, dtype=SURFACE_VERTEX_DTYPE)
    t = np.ascontiguousarray(triangles, dtype="<u4").reshape(-1, 3)
    faces = np.empty(len(t), dtype=np.dtype([("n", "u1"), ("idx", "<u4", (3,))], align=False))
    faces["n"] = 3
    faces["idx"] = t
    head = ("ply\nformat binary_little_endian 1.0\ncomment iso-surface (DESIGN.md section 3b)\n"
            f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\n"
            f"element face {len(t)}\nproperty list uchar uint vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(faces.tobytes())


def write_pathlines_ply(path, history: np.ndarray) -> None:
    """Binary little-endian PLY of pathlines: history is (count, M, 4) as SPHFluidGPU.tracer_history returns it; one vertex
    (x, y, z, age) per snapshot and tracer, one edge between consecutive snapshots of the same tracer."""
    h = np.ascontiguousarray(history, dtype="<f4")
    if h.ndim != 3 or h.shape[2] != 4:
        raise SphError(f"write_pathlines_ply: history must have shape (count, M, 4), not {h.shape}")
    count, m = h.shape[0], h.shape[1]
    a = (np.arange(max(count - 1, 0), dtype=np.int64)[:, None] * m + np.arange(m, dtype=np.int64)[None, :]).reshape(-1)
    edges = np.empty((len(a), 2), "<i4")
    edges[:, 0] = a
    edges[:, 1] = a + m
    head = ("ply\nformat binary_little_endian 1.0\ncomment tracer pathlines (DESIGN.md section 3d)\n"
            f"element vertex {count * m}\nproperty float x\nproperty float y\nproperty float z\nproperty float age\n"
            f"element edge {len(edges)}\nproperty int vertex1\nproperty int vertex2\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(h.tobytes())
        fh.write(edges.tobytes())


def write_points_ply(path, records: np.ndarray) -> None:
    """Binary little-endian PLY of diffuse particles: one vertex (x, y, z, kind) per DIFFUSE_DTYPE record."""
    r = np.ascontiguousarray(records, DIFFUSE_DTYPE)
    v = np.empty(len(r), np.dtype([("pos", "<f4", (3,)), ("kind", "u1")], align=False))
    v["pos"] = r["pos"]
    v["kind"] = r["kind"]
    head = ("ply\nformat binary_little_endian 1.0\ncomment spray 0, foam 1, bubbles 2 (DESIGN.md section 3j)\n"
            f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\nproperty uchar kind\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(v.tobytes())


def _copy_config(config, overrides):
    kind = type(config)
    cfg = kind.from_buffer_copy(config)
    for name, value in overrides.items():
        if name not in dict(kind._fields_) or name == "pad":
            raise SphError(f"{kind.__name__} has no field {name}")
        setattr(cfg, name, value)
    return cfg


def diffuse_config(**overrides) -> SphDiffuseConfig:
    """sph_diffuse_default with the named fields replaced.  No device is needed."""
    cfg = SphDiffuseConfig()
    load_library().sph_diffuse_default(C.byref(cfg))
    return _copy_config(cfg, overrides)


def _info_dict(info) -> dict:
    out = {name: int(getattr(info, name)) for name, _ in SphDiffuseInfo._fields_ if name not in ("aliveByKind", "pad")}
    out["aliveByKind"] = [int(x) for x in info.aliveByKind]
    return out


def diffuse_crest_config(**overrides) -> SphDiffuseCrest:
    """sph_diffuse_crest_default with the named fields replaced.  No device is needed."""
    cfg = SphDiffuseCrest()
    load_library().sph_diffuse_crest_default(C.byref(cfg))
    return _copy_config(cfg, overrides)


_CREST_BOOKS = ("acting", "crestSpawned", "shellSize")


def _crest_info_dict(info) -> dict:
    out = {name: int(getattr(info, name)) for name in _CREST_BOOKS + ("on", "stencil")}
    out["radius"] = float(info.radius)
    return out


def diffuse_step_host(config, params, pool, samples, particles, substep: int, dt: float = -1.0, totals=None, crest=None, shell_rows=None):
    """sph_diffuse_step_host: (pool one substep later, totals dict).  pool: DIFFUSE_DTYPE records, samples: the SAMPLE_DTYPE records at
    their positions, particles: the state the substep starts from, substep: the counter before the step, totals: the dict a previous
    call returned (or None for zeros).  crest: a SphDiffuseCrest -- then sph_diffuse_step_host_crest with shell_rows, the SHELL_DTYPE
    rows by id of `particles` (shell_host with the crest config's radius, offset, minCount and flags); the totals dict then carries the
    crest books (acting, crestSpawned, shellSize) too.  No device is needed."""
    src = np.ascontiguousarray(pool, DIFFUSE_DTYPE)
    smp = np.ascontiguousarray(samples, SAMPLE_DTYPE)
    if len(smp) != len(src):
        raise SphError(f"{len(smp)} samples for {len(src)} diffuse records")
    rec = np.ascontiguousarray(particles, PARTICLE_DTYPE)
    out = np.zeros(max(min(int(config.capacity), len(src) + 8 * len(rec)), 1), DIFFUSE_DTYPE)
    info, books = SphDiffuseInfo(), SphDiffuseCrestInfo()
    for name, value in (totals or {}).items():
        if name == "aliveByKind":
            info.aliveByKind[:] = list(value)
        elif name in _CREST_BOOKS:
            setattr(books, name, value)
        else:
            setattr(info, name, value)
    n = C.c_size_t()
    if crest is None:
        _check(load_library().sph_diffuse_step_host(C.byref(config), C.byref(params), float(dt), int(substep), _ptr_or_none(src), len(src),
                                                    _ptr_or_none(smp), _ptr_or_none(rec), len(rec), _ptr(out), C.byref(n), C.byref(info)))
        return out[:n.value].copy(), dict(_info_dict(info), **{k: v for k, v in (totals or {}).items() if k in _CREST_BOOKS})
    rows = None if shell_rows is None else np.ascontiguousarray(shell_rows, SHELL_DTYPE)
    if rows is not None and len(rows) != len(rec):
        raise SphError(f"{len(rows)} shell rows for {len(rec)} particles")
    _check(load_library().sph_diffuse_step_host_crest(C.byref(config), C.byref(crest), C.byref(params), float(dt), int(substep), _ptr_or_none(src),
                                                      len(src), _ptr_or_none(smp), _ptr_or_none(rec), len(rec),
                                                      None if rows is None else _ptr_or_none(rows), _ptr(out), C.byref(n), C.byref(info),
                                                      C.byref(books)))
    return out[:n.value].copy(), dict(_info_dict(info), **{k: int(getattr(books, k)) for k in _CREST_BOOKS})


_NO_POINT = np.zeros((1, 4), np.float32)                                            # somewhere for the pointer of an empty query to point


def _host_args(records, params, query, if_empty=None):
    """What the host twins of the queries begin with: (number of result rows, (records, n, params, query, m)).  query: the (m, 4)
    points or (m, 8) rays, or None for one row per record (a null pointer, m = 0); the pointer of an empty query is that of `if_empty`
    (None: null).  The pointers keep their arrays alive."""
    rec = np.ascontiguousarray(records, PARTICLE_DTYPE)
    if query is None:
        return len(rec), (_ptr_or_none(rec), len(rec), C.byref(params), None, 0)
    at = query if len(query) else if_empty
    return len(query), (_ptr_or_none(rec), len(rec), C.byref(params), None if at is None else _ptr(at), len(query))


def neighbors_host(records, params, radius, points=None, self_=False, half=False, count_only=False):
    """sph_neighbors_host: (offsets, indices) of SPHFluidGPU.neighbors (points None) or query_neighbors on host records, computed on the
    CPU by the same accept function over a counting sort of its own.  No device is needed."""
    L = load_library()
    p4 = None if points is None else _points4(points, "neighbors_host", keep_w=False)
    rows, head = _host_args(records, params, p4, if_empty=p4)                           # (null means "no query points": an empty array stays one)
    flags = _neighbor_flags(self_, half, count_only)
    off = np.zeros(rows + 1, np.int64)
    info = SphNeighborInfo()

    def call(fl, idx, cap):
        return L.sph_neighbors_host(*head, float(radius), fl, _ptr(off), _ptr(idx) if idx is not None else None, cap, C.byref(info))
    _check(call(flags | SPH_NEIGHBORS_COUNT_ONLY, None, 0))
    if count_only:
        return off, None
    idx = np.zeros(int(info.total), np.int32)
    _check(call(flags, idx, len(idx)))
    return off, idx


def components_host(records, params, radius, fluid_only: bool = False):
    """sph_components_host: (labels, roots, table, info) of SPHFluidGPU.components on host records, computed on the CPU by a sequential
    union-find with the same accept function.  No device is needed."""
    rec = np.ascontiguousarray(records, PARTICLE_DTYPE)
    n = len(rec)
    labels, roots, table = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, COMPONENT_DTYPE)
    info = SphComponentInfo()
    _check(load_library().sph_components_host(_ptr_or_none(rec), n, C.byref(params), float(radius), SPH_COMPONENTS_FLUID_ONLY if fluid_only else 0,
                                              _ptr_or_none(labels), _ptr_or_none(roots), _ptr_or_none(table), n, C.byref(info)))
    return labels, roots, table[:int(info.numComponents)].copy(), info


def knn_host(records, params, k, radius, points=None, self_=False, fluid_only=False):
    """sph_knn_host: (idx, d2, counts, info) of SPHFluidGPU.knn (points None) or query_knn on host records, computed on the CPU: the
    counting sort of neighbors_host, the same r2, per row the accepted keys sorted and cut at k.  No device is needed."""
    p4 = None if points is None else _points4(points, "knn_host", keep_w=False)
    rows, head = _host_args(records, params, p4, if_empty=_NO_POINT)                    # (non-null: query rows, also for m = 0)
    kk = int(k)
    width = kk if 1 <= kk <= SPH_KNN_MAX_K else 1                                    # (a refused k writes nothing)
    idx, d2, cnt = np.zeros((rows, width), np.int32), np.zeros((rows, width), np.float32), np.zeros(rows, np.uint32)
    info = SphKnnInfo()
    _check(load_library().sph_knn_host(*head, kk, float(radius), _knn_flags(self_, fluid_only), _ptr_or_none(idx), _ptr_or_none(d2), _ptr_or_none(cnt),
                                       C.byref(info)))
    return idx, d2, cnt, info


def shell_config(**overrides) -> SphShellConfig:
    """sph_shell_default with the named fields replaced.  No device is needed."""
    cfg = SphShellConfig()
    load_library().sph_shell_default(C.byref(cfg))
    return _copy_config(cfg, overrides)


def _shell_cfg(radius, offset, min_count, fluid_only) -> SphShellConfig:
    """The config of shell(), query_shell() and shell_host(); radius None goes as 0: the library's default, param_h."""
    return shell_config(radius=0.0 if radius is None else radius, offset=offset, minCount=min_count, flags=SPH_SHELL_FLUID_ONLY if fluid_only else 0)


def shell_host(records, params, radius=None, offset=0.10, min_count=0, fluid_only=False, points=None, sums=False):
    """sph_shell_host: (rows, ids, info) of SPHFluidGPU.shell (points None) or query_shell on host records, computed on the CPU by the
    device's own per-candidate, finish and crest functions over the counting sort of neighbors_host, in the same order: the same bytes.
    sums=True adds the (rows, 4) float32 sums of pass 1 (Sx, Sy, Sz, W) the rows were finished from.  No device is needed."""
    p4 = None if points is None else _points4(points, "shell_host", keep_w=False)
    rows, head = _host_args(records, params, p4, if_empty=_NO_POINT)                    # (non-null: query rows, also for m = 0)
    out, ids, acc = np.zeros(rows, SHELL_DTYPE), np.zeros(rows, np.int32), np.zeros((rows, 4), np.float32)
    info = SphShellInfo()
    cfg = _shell_cfg(radius, offset, min_count, fluid_only)
    _check(load_library().sph_shell_host(*head, C.byref(cfg), _ptr_or_none(out), _ptr_or_none(ids), _ptr_or_none(acc) if sums else None, C.byref(info)))
    res = (out, ids[:int(info.numShell)].copy(), info)
    return res + (acc,) if sums else res


def aniso_config(**overrides) -> SphAnisoConfig:
    """sph_aniso_default with the named fields replaced.  No device is needed."""
    cfg = SphAnisoConfig()
    load_library().sph_aniso_default(C.byref(cfg))
    return _copy_config(cfg, overrides)


def _aniso_cfg(radius=None, support=None, smoothing=0.9, max_ratio=4.0, max_stretch=1.5, min_count=25, sparse_scale=0.5, fluid_only=False) -> SphAnisoConfig:
    """The config of anisotropy(), aniso_lattice(), aniso_surface() and the two twins; radius / support None go as 0: the library's
    defaults, 2 param_h and param_h."""
    return aniso_config(radius=0.0 if radius is None else radius, support=0.0 if support is None else support, smoothing=smoothing, maxRatio=max_ratio,
                        maxStretch=max_stretch, sparseScale=sparse_scale, minCount=min_count, flags=SPH_ANISO_FLUID_ONLY if fluid_only else 0)


def aniso_host(records, params, **cfg):
    """sph_aniso_host: (rows, info) of SPHFluidGPU.anisotropy(**cfg) on host records, computed on the CPU by the device's own sum and
    finish functions over the counting sort of neighbors_host, in the same order: the same bytes.  No device is needed."""
    rec = np.ascontiguousarray(records, PARTICLE_DTYPE)
    out = np.zeros(len(rec), ANISO_DTYPE)
    info = SphAnisoInfo()
    _check(load_library().sph_aniso_host(_ptr_or_none(rec), len(rec), C.byref(params), C.byref(_aniso_cfg(**cfg)), _ptr_or_none(out), C.byref(info)))
    return out, info


def aggregate_config(**overrides) -> SphAggregateConfig:
    """sph_aggregate_default with the named fields replaced.  No device is needed."""
    cfg = SphAggregateConfig()
    load_library().sph_aggregate_default(C.byref(cfg))
    return _copy_config(cfg, overrides)


def _aggregate_cfg(radius, op, weight, channels, self_=False, fluid_only=False, delta=False, moments=False) -> SphAggregateConfig:
    """The config of aggregate(), query_aggregate() and aggregate_host(); op and weight by name or by number."""
    flags = (SPH_AGGREGATE_SELF if self_ else 0) | (SPH_AGGREGATE_FLUID_ONLY if fluid_only else 0) | (SPH_AGGREGATE_DELTA if delta else 0) | \
        (SPH_AGGREGATE_MOMENTS if moments else 0)
    try:
        op, weight = AGGREGATE_OPS.get(op, op), AGGREGATE_WEIGHTS.get(weight, weight)
        return aggregate_config(radius=float(radius), op=int(op), weight=int(weight), flags=flags, channels=int(channels))
    except (TypeError, ValueError):
        raise SphError(f"aggregate: op {op!r} (one of {sorted(AGGREGATE_OPS)}), weight {weight!r} (one of {sorted(AGGREGATE_WEIGHTS)})") from None


def aggregate_host(records, params, values, radius, points=None, op="sum", weight="one", self_=False, fluid_only=False, delta=False, moments=False,
                   counts=False):
    """sph_aggregate_host: the result of SPHFluidGPU.aggregate (points None) or query_aggregate on host records and (n, C) host values,
    computed on the CPU by the same per-candidate functions over the counting sort of neighbors_host: the same bytes.  No device is
    needed."""
    p4 = None if points is None else _points4(points, "aggregate_host", keep_w=False)
    rows, head = _host_args(records, params, p4, if_empty=_NO_POINT)                    # (non-null: query rows, also for m = 0)
    vals = _scalar_values(values, head[1])
    c = int(vals.shape[1])
    cfg = _aggregate_cfg(radius, op, weight, c, self_, fluid_only, delta, moments)
    out = np.zeros((rows, 4, c) if moments else (rows, c), np.float32)
    cnt = np.zeros(rows, np.uint32)
    _check(load_library().sph_aggregate_host(head[0], head[1], head[2], C.byref(cfg), head[3], head[4], _ptr_or_none(vals), _ptr_or_none(out),
                                             _ptr_or_none(cnt) if counts else None))
    return (out, cnt) if counts else out


def aggregate_adjoint_host(records, params, grad, radius, points=None, weight="one", self_=False, fluid_only=False, delta=False, moments=False):
    """sph_aggregate_adjoint_host: the (n, C) result of SPHFluidGPU.aggregate_adjoint (points None) or query_aggregate_adjoint on host
    records and host grad, computed on the CPU by the same per-term functions in the same order: the same bytes.  No device is needed."""
    p4 = None if points is None else _points4(points, "aggregate_adjoint_host", keep_w=False)
    rows, head = _host_args(records, params, p4, if_empty=_NO_POINT)
    g = _planes(grad, rows, moments, "aggregate_adjoint_host")
    c = int(g.shape[-1])
    cfg = _aggregate_cfg(radius, "sum", weight, c, self_, fluid_only, delta, moments)
    out = np.zeros((head[1], c), np.float32)
    _check(load_library().sph_aggregate_adjoint_host(head[0], head[1], head[2], C.byref(cfg), head[3], head[4], _ptr_or_none(g), _ptr_or_none(out)))
    return out


def aggregate_position_grad_host(records, params, values, grad, radius, points=None, weight="one", self_=False, fluid_only=False, delta=False,
                                 moments=False):
    """sph_aggregate_posgrad_host: the (n, 3) result of SPHFluidGPU.aggregate_position_grad (points None), or the pair (grad_points (m, 3),
    grad_particles (n, 3)) of query_aggregate_position_grad, on host records, values and grad, computed on the CPU by the same per-term
    functions in the same order: the same bytes.  No device is needed."""
    p4 = None if points is None else _points4(points, "aggregate_position_grad_host", keep_w=False)
    rows, head = _host_args(records, params, p4, if_empty=_NO_POINT)
    vals = _scalar_values(values, head[1])
    c = int(vals.shape[1])
    g = _planes(grad, rows, moments, "aggregate_position_grad_host")
    if int(g.shape[-1]) != c:
        raise SphError(f"aggregate_position_grad_host: grad of shape {g.shape} for values of shape {vals.shape}")
    cfg = _aggregate_cfg(radius, "sum", weight, c, self_, fluid_only, delta, moments)
    out_pts, out_par = np.zeros((rows if p4 is not None else 0, 3), np.float32), np.zeros((head[1], 3), np.float32)
    _check(load_library().sph_aggregate_posgrad_host(head[0], head[1], head[2], C.byref(cfg), head[3], head[4], _ptr_or_none(vals), _ptr_or_none(g),
                                                     None if p4 is None else _ptr(out_pts if len(out_pts) else _NO_POINT), _ptr(out_par if len(out_par) else _NO_POINT)))
    return out_par if p4 is None else (out_pts, out_par)


def aggregate_arg_host(records, params, values, radius, points=None, op="max", self_=False, fluid_only=False, delta=False, counts=False):
    """sph_aggregate_arg_host: (out, arg), or with counts=True (out, counts, arg), of SPHFluidGPU.aggregate_arg (points None) or
    query_aggregate_arg on host records: the same bytes.  No device is needed."""
    p4 = None if points is None else _points4(points, "aggregate_arg_host", keep_w=False)
    rows, head = _host_args(records, params, p4, if_empty=_NO_POINT)
    vals = _scalar_values(values, head[1])
    c = int(vals.shape[1])
    cfg = _aggregate_cfg(radius, op, "one", c, self_, fluid_only, delta, False)
    out = np.zeros((rows, c), np.float32)
    arg = np.full((rows, c), -1, np.int32)
    cnt = np.zeros(rows, np.uint32)
    _check(load_library().sph_aggregate_arg_host(head[0], head[1], head[2], C.byref(cfg), head[3], head[4], _ptr_or_none(vals), _ptr_or_none(out),
                                                 _ptr_or_none(cnt) if counts else None, _ptr_or_none(arg)))
    return (out, cnt, arg) if counts else (out, arg)


def aggregate_route_host(records, params, arg, grad, radius, points=None, op="max", self_=False, fluid_only=False, delta=False):
    """sph_aggregate_route_host: the (n, C) result of SPHFluidGPU.aggregate_route (points None) or query_aggregate_route on host records:
    the same bytes.  No device is needed."""
    p4 = None if points is None else _points4(points, "aggregate_route_host", keep_w=False)
    rows, head = _host_args(records, params, p4, if_empty=_NO_POINT)
    g = _planes(grad, rows, False, "aggregate_route_host")
    c = int(g.shape[1])
    a = np.ascontiguousarray(arg, np.int32)
    if a.shape != (rows, c):
        raise SphError(f"aggregate_route_host: arg of shape {a.shape} for grad of shape {(rows, c)}")
    cfg = _aggregate_cfg(radius, op, "one", c, self_, fluid_only, delta, False)
    out = np.zeros((head[1], c), np.float32)
    _check(load_library().sph_aggregate_route_host(head[0], head[1], head[2], C.byref(cfg), head[3], head[4], _ptr_or_none(a), _ptr_or_none(g), _ptr_or_none(out)))
    return out


def basis_config(**overrides) -> SphBasisConfig:
    """sph_aggregate_basis_default with the named fields replaced.  No device is needed."""
    cfg = SphBasisConfig()
    load_library().sph_aggregate_basis_default(C.byref(cfg))
    return _copy_config(cfg, overrides)


def _basis_planes(size) -> int:
    """B = K^3 of a filter grid of size K; the library refuses a K outside 2 .. 4, so anything else counts as no plane."""
    try:
        k = int(size)
    except (TypeError, ValueError):
        raise SphError(f"aggregate_basis: size {size!r} (2, 3 or 4)") from None
    return k ** 3 if 2 <= k <= 4 else 0


def _basis_cfg(radius, size, weight, channels, self_=False, fluid_only=False) -> SphBasisConfig:
    """The config of aggregate_basis(), its adjoint and the host twins; weight by name or by number."""
    flags = (SPH_AGGREGATE_SELF if self_ else 0) | (SPH_AGGREGATE_FLUID_ONLY if fluid_only else 0)
    try:
        return basis_config(radius=float(radius), weight=int(AGGREGATE_WEIGHTS.get(weight, weight)), flags=flags, channels=int(channels), size=int(size))
    except (TypeError, ValueError):
        raise SphError(f"aggregate_basis: weight {weight!r} (one of {sorted(AGGREGATE_WEIGHTS)}), size {size!r} (2, 3 or 4)") from None


def _basis_planes_array(h, rows, size, who):
    """h as float32 numpy of (rows, K^3, C)."""
    a = np.ascontiguousarray(h, np.float32)
    if a.ndim != 3 or a.shape[0] != rows or a.shape[1] != _basis_planes(size):
        raise SphError(f"{who}: h of shape {a.shape} for {rows} rows of {_basis_planes(size)} planes")
    return a


def aggregate_basis_host(records, params, x, radius, points=None, size=4, weight="poly6", self_=False, fluid_only=False, counts=False):
    """sph_aggregate_basis_host: the (rows, size^3, C) result of SPHFluidGPU.aggregate_basis (points None) or query_aggregate_basis on
    host records and (n, C) host values, computed on the CPU by the same per-candidate functions in the same order: the same bytes.  No
    device is needed."""
    p4 = None if points is None else _points4(points, "aggregate_basis_host", keep_w=False)
    rows, head = _host_args(records, params, p4, if_empty=_NO_POINT)                    # (non-null: query rows, also for m = 0)
    vals = _scalar_values(x, head[1])
    c = int(vals.shape[1])
    cfg = _basis_cfg(radius, size, weight, c, self_, fluid_only)
    out = np.zeros((rows, _basis_planes(size), c), np.float32)
    cnt = np.zeros(rows, np.uint32)
    _check(load_library().sph_aggregate_basis_host(head[0], head[1], head[2], C.byref(cfg), head[3], head[4], _ptr_or_none(vals), _ptr_or_none(out),
                                                   _ptr_or_none(cnt) if counts else None))
    return (out, cnt) if counts else out


def aggregate_basis_adjoint_host(records, params, h, radius, points=None, size=4, weight="poly6", self_=False, fluid_only=False):
    """sph_aggregate_basis_adjoint_host: the (n, C) result of SPHFluidGPU.aggregate_basis_adjoint (points None) or
    query_aggregate_basis_adjoint on host records and host h of (rows, size^3, C): the same bytes.  No device is needed."""
    p4 = None if points is None else _points4(points, "aggregate_basis_adjoint_host", keep_w=False)
    rows, head = _host_args(records, params, p4, if_empty=_NO_POINT)
    a = _basis_planes_array(h, rows, size, "aggregate_basis_adjoint_host")
    c = int(a.shape[2])
    cfg = _basis_cfg(radius, size, weight, c, self_, fluid_only)
    out = np.zeros((head[1], c), np.float32)
    _check(load_library().sph_aggregate_basis_adjoint_host(head[0], head[1], head[2], C.byref(cfg), head[3], head[4], _ptr_or_none(a), _ptr_or_none(out)))
    return out


def aggregate_basis_position_grad_host(records, params, x, grad, radius, points=None, size=4, weight="poly6", self_=False, fluid_only=False,
                                       want_points=True, want_particles=True):
    """sph_aggregate_basis_posgrad_host: the (n, 3) result of SPHFluidGPU.aggregate_basis_position_grad (points None), or the pair
    (grad_points (m, 3), grad_particles (n, 3)) of query_aggregate_basis_position_grad (None for an output that is not wanted), on host
    records, x and grad, computed on the CPU by the same per-term functions in the same order: the same bytes.  No device is needed."""
    p4 = None if points is None else _points4(points, "aggregate_basis_position_grad_host", keep_w=False)
    rows, head = _host_args(records, params, p4, if_empty=_NO_POINT)
    vals = _scalar_values(x, head[1])
    c = int(vals.shape[1])
    g = _basis_planes_array(grad, rows, size, "aggregate_basis_position_grad_host")
    if int(g.shape[2]) != c:
        raise SphError(f"aggregate_basis_position_grad_host: grad of shape {g.shape} for values of shape {vals.shape}")
    cfg = _basis_cfg(radius, size, weight, c, self_, fluid_only)
    out_pts = np.zeros((rows, 3), np.float32) if p4 is not None and want_points else None
    out_par = np.zeros((head[1], 3), np.float32) if p4 is None or want_particles else None
    ptr = lambda a: None if a is None else _ptr(a if len(a) else _NO_POINT)
    _check(load_library().sph_aggregate_basis_posgrad_host(head[0], head[1], head[2], C.byref(cfg), head[3], head[4], _ptr_or_none(vals), _ptr_or_none(g),
                                                           ptr(out_pts), ptr(out_par)))
    return out_par if p4 is None else (out_pts, out_par)


def aniso_lattice_host(records, params, origin, spacing, dims, **cfg):
    """sph_aniso_lattice_host: (values of shape (nz, ny, nx), info) of SPHFluidGPU.aniso_lattice on host records, computed on the CPU
    in the same order: the same bytes.  No device is needed."""
    rec = np.ascontiguousarray(records, PARTICLE_DTYPE)
    nx, ny, nz = (int(x) for x in dims)
    out = np.zeros((max(nz, 0), max(ny, 0), max(nx, 0)), np.float32)
    info = SphAnisoInfo()
    _check(load_library().sph_aniso_lattice_host(_ptr_or_none(rec), len(rec), C.byref(params), C.byref(_aniso_cfg(**cfg)), _f3(origin),
                                                 _f3(_spacing3(spacing)), _dims3((nx, ny, nz)), _ptr(out) if out.size else None, C.byref(info)))
    return out, info


def rays_host(records, params, rays, radius, fluid_only=False, any_hit=False, with_info=False, walk=False):
    """sph_rays_host: (t, ids, pos, normal) of SPHFluidGPU.raycast on host records, computed on the CPU by brute force over all
    participating records with the same hit arithmetic: the definition of a cast.  with_info adds the SphRaysInfo.  walk=True runs
    sph_rays_walk_host in its place: the device's grid walk, on the host.  No device is needed."""
    rows, head = _host_args(records, params, _rays8(rays, "rays_host"))
    hits = np.zeros(rows, RAY_HIT_DTYPE)
    info = SphRaysInfo()
    L = load_library()
    _check((L.sph_rays_walk_host if walk else L.sph_rays_host)(*head, float(radius), _rays_flags(fluid_only, any_hit), _ptr_or_none(hits), C.byref(info)))
    out = _split_hits(hits)
    return out + (info,) if with_info else out


def _spans_host(who, fn, records, params, rays, radius, fluid_only, with_info, *variant):
    rows, head = _host_args(records, params, _rays8(rays, who))
    out = np.zeros(rows, RAY_SPAN_DTYPE)
    info = SphRaySpansInfo()
    _check(fn(*head, float(radius), _rays_flags(fluid_only, False), *variant, _ptr_or_none(out), C.byref(info)))
    return (out, info) if with_info else out


def ray_spans_host(records, params, rays, radius, fluid_only=False, with_info=False):
    """sph_rays_span_host: the RAY_SPAN_DTYPE rows of SPHFluidGPU.ray_spans on host records, computed on the CPU by brute force over all
    participating records: the definition of a span.  with_info adds the SphRaySpansInfo.  No device is needed."""
    return _spans_host("ray_spans_host", load_library().sph_rays_span_host, records, params, rays, radius, fluid_only, with_info)


def ray_spans_walk_host(records, params, rays, radius, fluid_only=False, with_info=False, variant=0):
    """sph_rays_span_walk_host: the same rows by the device's span walk over a grid built on the host; variant 0 = the layer walk,
    1 = the block walk (SPH_OPT_RAY_SPANS_VARIANT).  No device is needed."""
    return _spans_host("ray_spans_walk_host", load_library().sph_rays_span_walk_host, records, params, rays, radius, fluid_only, with_info, int(variant))


def ray_thickness(rows, radius) -> np.ndarray:
    """The summed chord length of RAY_SPAN_DTYPE rows in world units, float64: length * 2 r * 2^-24.  Overlapping spheres add."""
    return np.asarray(rows)["length"].astype(np.float64) * (2.0 * float(radius) * 2.0 ** -24)


def camera_rays(eye, target, up, fov_y, width, height, tmin=0.0, tmax=np.inf) -> np.ndarray:
    """(width * height, 8) rays of a pinhole camera at `eye` looking at `target`: row y * width + x goes through the centre of pixel
    (x, y), y downwards, of an image plane at distance 1 with a vertical field of view of fov_y radians.  Directions are not normalised
    (the one through the image centre has length 1).  Only an array of rays: no image is written anywhere."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    th = np.tan(0.5 * float(fov_y))
    px = ((np.arange(width) + 0.5) / width * 2.0 - 1.0) * th * (width / height)
    py = (1.0 - (np.arange(height) + 0.5) / height * 2.0) * th
    d = f[None, None, :] + px[None, :, None] * s[None, None, :] + py[:, None, None] * u[None, None, :]
    r = np.zeros((height * width, 8), np.float32)
    r[:, 0:3] = eye
    r[:, 3] = tmin
    r[:, 4:7] = d.reshape(-1, 3)
    r[:, 7] = tmax
    return r


def parallel_rays(origin, u, v, direction, nu, nv, tmin=0.0, tmax=np.inf) -> np.ndarray:
    """(nu * nv, 8) parallel rays: row j * nu + i starts at origin + (i + 0.5) / nu * u + (j + 0.5) / nv * v, the centres of an nu x nv
    sheet spanned by the vectors u and v, and every ray has the given direction (not normalised)."""
    origin, u, v, direction = (np.asarray(x, np.float64) for x in (origin, u, v, direction))
    a = (np.arange(nu) + 0.5) / nu
    b = (np.arange(nv) + 0.5) / nv
    o = origin[None, None, :] + a[None, :, None] * u[None, None, :] + b[:, None, None] * v[None, None, :]
    r = np.zeros((nu * nv, 8), np.float32)
    r[:, 0:3] = o.reshape(-1, 3)
    r[:, 3] = tmin
    r[:, 4:7] = direction
    r[:, 7] = tmax
    return r


def component_centers(table, grid) -> np.ndarray:
    """(C, 3) float64 centres of the bodies of a component table: gridMin + cellSize * sumQ / (65536 * count), `grid` the SphGridInfo of
    the state (compute_grid_extents).  A body flagged SPH_COMPONENT_NONFINITE has no centre (NaN)."""
    t = np.asarray(table)
    gmin = np.array(list(grid.gridMin), np.float64)
    cnt = t["count"].astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        ctr = gmin + float(grid.cellSize) * t["sumQ"].astype(np.float64) / (65536.0 * cnt)
    ctr[(t["flags"] & SPH_COMPONENT_NONFINITE) != 0] = np.nan
    return ctr


def obstacles_apply_host(obstacles, particle_mass: float, particles: np.ndarray):
    """sph_obstacles_apply_host on a copy of the records: (records, impulses (K, 6)).  No device is needed."""
    arr = obstacle_array(obstacles)
    rec = np.ascontiguousarray(particles, PARTICLE_DTYPE).copy()
    imp = np.zeros((max(len(arr), 1), 6), np.float64)
    L = load_library()
    _check(L.sph_obstacles_apply_host(_ptr_or_none(arr), len(arr), float(particle_mass), _ptr(rec), len(rec), _ptr(imp)))
    return rec, imp[:len(arr)]


def obstacles_advance_host(obstacles, dt: float) -> np.ndarray:
    """sph_obstacles_advance_host on a copy: the bodies one substep of dt later.  No device is needed."""
    arr = obstacle_array(obstacles).copy()
    _check(load_library().sph_obstacles_advance_host(_ptr_or_none(arr), len(arr), float(dt)))
    return arr


def volume_sample_host(values, spacing, local):
    """sph_volume_sample_host at one local point of a (nz, ny, nx) lattice: (phi, gradient[3], inside).  No device is needed."""
    v, dims, sp = _volume_lattice(values, spacing)
    phi, inside, g = C.c_float(), C.c_int(), (C.c_float * 3)()
    _check(load_library().sph_volume_sample_host(_ptr(v), dims, _f3(sp), _f3(local), C.byref(phi), g, C.byref(inside)))
    return np.float32(phi.value), np.array(g, np.float32), bool(inside.value)


def obstacles_apply_host_volumes(obstacles, volumes, bindings, particle_mass: float, particles: np.ndarray):
    """sph_obstacles_apply_host_volumes on a copy of the records: (records, impulses (K, 6)).  volumes is a list of (values (nz, ny, nx),
    spacing), bindings one volume index (or -1) per body.  No device is needed."""
    arr = obstacle_array(obstacles)
    rec = np.ascontiguousarray(particles, PARTICLE_DTYPE).copy()
    imp = np.zeros((max(len(arr), 1), 6), np.float64)
    keep, vols = [], (SphVolumeHost * max(len(volumes), 1))()
    for i, (values, spacing) in enumerate(volumes):
        v, dims, sp = _volume_lattice(values, spacing)
        keep.append(v)
        vols[i].values = v.ctypes.data
        vols[i].dims[:] = list(dims)
        vols[i].spacing[:] = [float(x) for x in sp]
    bind = np.ascontiguousarray(bindings, np.int32)
    if len(bind) != len(arr):
        raise SphError(f"{len(bind)} bindings for {len(arr)} obstacles")
    _check(load_library().sph_obstacles_apply_host_volumes(_ptr_or_none(arr), len(arr), C.byref(vols), len(volumes),
                                                           _ptr_or_none(bind), float(particle_mass), _ptr(rec), len(rec), _ptr(imp)))
    return rec, imp[:len(arr)]


def mesh_distance_host(vertices, triangles, origin, spacing, dims) -> np.ndarray:
    """sph_mesh_distance_host: the signed distances as a float32 array of shape (nz, ny, nx).  No device is needed (plain loops: small cases)."""
    v, t = _mesh_arrays(vertices, triangles)
    d = _dims3(dims, "mesh_distance_host")
    sp = _spacing3(spacing)
    out = np.empty((int(d[2]), int(d[1]), int(d[0])), np.float32)
    _check(load_library().sph_mesh_distance_host(_ptr(v), len(v), _ptr(t), len(t), _f3(origin), _f3(sp), d, _ptr(out)))
    return out


def obstacles_step_host(obstacles, records, impulses, params, dt: float) -> np.ndarray:
    """sph_obstacles_step_host on a copy: the bodies after the body step of one substep.  records: one
    dynamics() record or None per body; impulses: the substep's (K, 6) sums or None.  No device is needed."""
    arr = obstacle_array(obstacles).copy()
    dyn = dynamics_array(records)
    if len(dyn) != len(arr):
        raise SphError(f"{len(dyn)} dynamics records for {len(arr)} obstacles")
    imp = None if impulses is None else np.ascontiguousarray(impulses, np.float64).reshape(len(arr), 6)
    _check(load_library().sph_obstacles_step_host(_ptr_or_none(arr), _ptr_or_none(dyn), len(arr), None if imp is None else _ptr_or_none(imp),
                                                  C.byref(params), float(dt)))
    return arr


def scalars_step_host(particles: np.ndarray, params: SphParams, values, diffusivity=0.0, decay=0.0, dt: float = -1.0):
    """sph_scalars_step_host on a copy of the values: ((n, K) values one substep later, the diffusion number).  No device is needed."""
    rec = np.ascontiguousarray(particles, PARTICLE_DTYPE)
    v = _scalar_values(values, len(rec)).copy()
    co = _scalar_coeffs(max(v.shape[1], 1), diffusivity, decay)
    s = C.c_float()
    _check(load_library().sph_scalars_step_host(_ptr(rec), len(rec), C.byref(params), float(dt), _ptr(v), v.shape[1], co.ctypes.data_as(_pf), C.byref(s)))
    return v, np.float32(s.value)


def volume_moments_host(values, spacing) -> np.ndarray:
    """sph_volume_moments_host of a (nz, ny, nx) lattice: the ten moments.  No device is needed."""
    v, dims, sp = _volume_lattice(values, spacing)
    out = np.zeros(10, np.float64)
    _check(load_library().sph_volume_moments_host(_ptr(v), dims, _f3(sp), _ptr(out)))
    return out


def scalars_couple_host(particles: np.ndarray, params: SphParams, values, beta=None, ref=0.0, sources=(), obstacles=(), dt: float = -1.0):
    """sph_scalars_couple_host on copies: (records, (n, K) values, sums, hits) after the coupling step of one substep (DESIGN.md
    section 3i).  obstacles: the poses body-bound sources ride on (what SPHFluidGPU.obstacles() returns).  No device is needed."""
    rec = np.ascontiguousarray(particles, PARTICLE_DTYPE).copy()
    v = _scalar_values(values, len(rec)).copy()
    b, r = _buoyancy(max(v.shape[1], 1), beta, ref)
    src, obs = source_array(sources), obstacle_array(obstacles)
    sums, hits = np.zeros(max(len(src), 1), np.float64), np.zeros(max(len(src), 1), np.uint64)
    _check(load_library().sph_scalars_couple_host(_ptr(rec), len(rec), C.byref(params), float(dt), _ptr(v), v.shape[1],
                                                  None if b is None else b.ctypes.data_as(_pf), None if r is None else r.ctypes.data_as(_pf),
                                                  _ptr_or_none(src), len(src), _ptr_or_none(obs), len(obs), _ptr(sums), _ptr(hits)))
    return rec, v, sums[:len(src)], hits[:len(src)]


def gates_step_host(entry: np.ndarray, exit_records: np.ndarray, gates, values=None, books=None) -> np.ndarray:
    """sph_gates_step_host: the books (GATE_BOOKS_DTYPE, one row per gate) after one substep whose entry and exit records are given
    (record i of both is the same particle), added in index order to a copy of `books` (None: zeros).  values: (n,) or (n, K) scalar
    values after the substep, or None.  No device is needed."""
    a, b = np.ascontiguousarray(entry, PARTICLE_DTYPE), np.ascontiguousarray(exit_records, PARTICLE_DTYPE)
    if len(a) != len(b):
        raise SphError("gates_step_host: entry and exit records differ in length")
    arr = gate_array(gates)
    v = None if values is None else _scalar_values(values, len(b))
    k = 0 if v is None else v.shape[1]
    out = np.zeros(max(len(arr), 1), GATE_BOOKS_DTYPE) if books is None else np.ascontiguousarray(books, GATE_BOOKS_DTYPE).copy()
    if len(out) < len(arr):
        raise SphError("gates_step_host: fewer book rows than gates")
    _check(load_library().sph_gates_step_host(_ptr(a), _ptr(b), len(b), _ptr_or_none(arr), len(arr), None if not k else _ptr(v), k, _ptr(out)))
    return out[:len(arr)] if books is None else out


def monitor_config(**overrides) -> SphMonitorConfig:
    """sph_monitor_config_default with the named fields replaced.  No device is needed."""
    cfg = SphMonitorConfig()
    load_library().sph_monitor_config_default(C.byref(cfg))
    return _copy_config(cfg, overrides)


def monitor_accumulate_host(rows, samples, wet_fraction: float = 0.5) -> np.ndarray:
    """sph_monitor_accumulate_host: the rows (MONITOR_ROW_DTYPE, any shape) after one acting substep whose samples (SAMPLE_DTYPE, the
    same number) are given, added to a copy of `rows` (None: zeros).  No device is needed."""
    smp = np.ascontiguousarray(samples, SAMPLE_DTYPE)
    out = np.zeros(smp.shape, MONITOR_ROW_DTYPE) if rows is None else np.ascontiguousarray(rows, MONITOR_ROW_DTYPE).copy()
    if out.size != smp.size:
        raise SphError("monitor_accumulate_host: rows and samples differ in length")
    _check(load_library().sph_monitor_accumulate_host(_ptr(out.reshape(-1)), _ptr(smp.reshape(-1)), smp.size, float(wet_fraction)))
    return out


def monitor_field_host(rows, field: int) -> np.ndarray:
    """sph_monitor_field_host: the derived field (SPH_MONITOR_*) of MONITOR_ROW_DTYPE rows, float32 of the rows' shape."""
    r = np.ascontiguousarray(rows, MONITOR_ROW_DTYPE)
    out = np.zeros(r.shape, np.float32)
    _check(load_library().sph_monitor_field_host(_ptr(r.reshape(-1)), r.size, int(field), _ptr(out.reshape(-1))))
    return out


def monitor_schedule_host(every: int, stride: int, history: int, substeps: int):
    """sph_monitor_schedule_host: (acts, rows) of the first `substeps` substeps after a set: acts[s] is 1 where substep s acts, rows[s]
    the ring row it writes or 0xFFFFFFFF."""
    acts, rows = np.zeros(substeps, np.uint32), np.zeros(substeps, np.uint32)
    _check(load_library().sph_monitor_schedule_host(int(every), int(stride), int(history), int(substeps), _ptr(acts), _ptr(rows)))
    return acts, rows


# ---- checkpoints: the host-only calls and the pure-Python twin of the parser ---------------------------------------------
def _state_blob(blob_or_path) -> np.ndarray:
    """A blob as a contiguous uint8 array: an array or bytes as they are, anything else is a path to read."""
    if isinstance(blob_or_path, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(blob_or_path), np.uint8)
    if isinstance(blob_or_path, np.ndarray):
        return np.ascontiguousarray(blob_or_path).view(np.uint8).reshape(-1)
    return np.fromfile(blob_or_path, np.uint8)


def _state_dict(formatVersion, abiVersion, checksumKind, n, totalBytes, params, sections) -> dict:
    return dict(formatVersion=int(formatVersion), abiVersion=int(abiVersion), checksumKind=int(checksumKind), n=int(n), totalBytes=int(totalBytes),
                params=params, sections=sections)


def state_info(blob) -> dict:
    """sph_state_peek: the blob validated whole (SphError names what is wrong) and its header and section table: formatVersion,
    abiVersion, checksumKind, n, totalBytes, params, and sections: name -> dict(version, offset, bytes, sum=(lo, hi))."""
    blob = _state_blob(blob)
    info = SphStateInfo()
    _check(load_library().sph_state_peek(_ptr(blob), blob.size, C.byref(info)))
    secs = {name: dict(version=int(info.version[i]), offset=int(info.offset[i]), bytes=int(info.bytes[i]), sum=(int(info.sum[i][0]), int(info.sum[i][1])))
            for i, name in enumerate(STATE_SECTIONS) if info.sections & (1 << i)}
    params = SphParams()
    C.memmove(C.byref(params), C.byref(info.params), C.sizeof(SphParams))
    return _state_dict(info.formatVersion, info.abiVersion, info.checksumKind, info.n, info.totalBytes, params, secs)


def state_checksum_host(buf):
    """sph_state_checksum_host: (lo, hi) of a buffer of a multiple of 8 bytes (an array of any dtype, or bytes)."""
    arr = _state_blob(buf)
    out = (C.c_uint64 * 2)()
    _check(load_library().sph_state_checksum_host(_ptr(arr) if arr.size else None, arr.size, out))
    return int(out[0]), int(out[1])


def state_sections(blob) -> dict:
    """The header and section table of a blob read in Python from the documented format (include/sph_abi.h): what state_info returns,
    without the library and WITHOUT its validation (no checksum is verified, no size is checked beyond what the reading needs)."""
    blob = _state_blob(blob)
    if blob.size < STATE_HEADER_DTYPE.itemsize:
        raise SphError(f"state_sections: {blob.size} bytes are less than a header")
    h = blob[:STATE_HEADER_DTYPE.itemsize].view(STATE_HEADER_DTYPE)[0]
    if int(h["magic"]) != SPH_STATE_MAGIC:
        raise SphError("state_sections: wrong magic")
    end = STATE_HEADER_DTYPE.itemsize + STATE_ENTRY_DTYPE.itemsize * int(h["sectionCount"])
    if blob.size < end:
        raise SphError("state_sections: the section table is truncated")
    secs = {}
    for s in blob[STATE_HEADER_DTYPE.itemsize:end].view(STATE_ENTRY_DTYPE):
        tag = int(s["tag"])
        name = STATE_SECTIONS[tag.bit_length() - 1] if tag and tag & (tag - 1) == 0 and tag.bit_length() <= len(STATE_SECTIONS) else f"tag{tag}"
        secs[name] = dict(version=int(s["version"]), offset=int(s["offset"]), bytes=int(s["bytes"]), sum=(int(s["sum"][0]), int(s["sum"][1])))
    params = SphParams.from_buffer_copy(h["params"].tobytes())
    return _state_dict(h["format"], h["abi"], h["checksumKind"], h["n"], h["totalBytes"], params, secs)


def monitor_means(rows) -> dict:
    """A numpy convenience over MONITOR_ROW_DTYPE rows, not byte-checked (plain float64 numpy, nan where the dividing count is 0):
    wet_share, fraction, density (over all samples), pressure, vel (..., 3) (over wet samples) and reynolds (..., 3, 3), the
    covariance <u_a u_b> - <u_a><u_b> of the wet samples."""
    r = np.asarray(rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        n, w = r["samples"].astype(np.float64), r["wet"].astype(np.float64)
        n, w = np.where(n > 0, n, np.nan), np.where(w > 0, w, np.nan)
        vel = r["sumVel"] / w[..., None]
        second = np.zeros(r.shape + (3, 3))
        for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            second[..., a, b] = second[..., b, a] = r["sumVelVel"][..., k] / w
        return dict(wet_share=r["wet"] / n, fraction=r["sumFraction"] / n, density=r["sumDensity"] / n, pressure=r["sumPressure"] / w, vel=vel,
                    reynolds=second - vel[..., :, None] * vel[..., None, :])
