"""MI355X-native SPH substep engine behind the reference's SPHFluidGPU surface.

Only the hot path SURVEY.md section 8 names lives here: csrc/ (HIP kernels + C-ABI,
include/sph_abi.h), engine.py (host mirror of the reference class), synthetic.py (bench
inputs), halo.py (z-slab decomposition).  Import with
importlib.import_module("componentframeworks-smoothed-particle-hydrodynamics_amd").
"""
from .engine import (  # noqa: F401
    ABI_SYMBOLS, KERNEL_CLASSES, PARTICLE_DTYPE, SPH_OPT_AOS_MODE, SPH_OPT_DEBUG, SPH_OPT_GRAPH, SPH_OPT_GRAPH_LAUNCHES, SPH_OPT_GRID_BUILD,
    SPH_ERR_TIMEOUT, SPH_OPT_NEIGHBOR_KERNEL, SPH_OPT_TIMING, SPHFluidGPU, SphError, SphFountain, SphGridInfo, SphParams, SphRiver, SphSlabIntent,
    SPH_SLAB_FLAG_SEND_OVERFLOW, SPH_SLAB_FLAG_SLOT_OVERFLOW, SPH_SLAB_FLAG_BAD_HEADER, SPH_SLAB_FLAG_TRUNCATED, SPH_SLAB_FLAG_LAYER_JUMP, SPH_SLAB_FLAG_SIZE_MISMATCH,
    compute_grid_extents, default_params, default_river, effective_half, generate_river_terrain, load_library, rotation_mat3, spawn_particles,
    spawn_river_particles, SAMPLE_DTYPE, SPH_FIELD_ALL, SPH_FIELD_DENSITY, SPH_FIELD_FRACTION, SPH_FIELD_PRESSURE, SPH_FIELD_SPEED, SphSample,
    gauge_levels, SURFACE_VERTEX_DTYPE, SphSurface, write_ply,
    SPH_STAT_DENSITY, SPH_STAT_PRESSURE, SPH_STAT_SPEED, SPH_STAT_POS_X, SPH_STAT_POS_Y, SPH_STAT_POS_Z, SPH_STAT_FOAM, SPH_STAT_MAX_SPECS,
    SPH_STAT_MAX_BINS, SphHistogramSpec, SphStatExtremum, SphStatistics, Statistics,
    SPH_TRACER_EULER, SPH_TRACER_MIDPOINT, SphTracer, TRACER_DTYPE, write_pathlines_ply,
    SPH_MAX_OBSTACLES, SPH_OBSTACLE_SPHERE, SPH_OBSTACLE_BOX, SPH_OBSTACLE_CAPSULE, SphObstacle, OBSTACLE_DTYPE, obstacle, obstacle_array,
    obstacles_apply_host, obstacles_advance_host,
    SPH_MAX_VOLUMES, SPH_OPT_MESH_SPLIT, SphVolumeHost, volume_sample_host, obstacles_apply_host_volumes, mesh_distance_host,
    SPH_DYNAMICS_CONFINED, SphObstacleDynamics, DYNAMICS_DTYPE, dynamics, dynamics_sphere, dynamics_box, dynamics_capsule, dynamics_array,
    mass_properties, obstacles_step_host, volume_moments_host,
    SPH_MAX_SCALAR_CHANNELS, SPH_OPT_SCALAR_SWEEP, SPH_SCALAR_ADD, SPH_SCALAR_SET, ScalarMoments, SphScalarMoments, mixing_index, scalars_step_host,
    SPH_MAX_SCALAR_SOURCES, SPH_SOURCE_SPHERE, SPH_SOURCE_BOX, SPH_SOURCE_RATE, SPH_SOURCE_RELAX, SphScalarSource, SOURCE_DTYPE, scalar_source,
    source_array, scalars_couple_host,
    SPH_MAX_GATES, SPH_MAX_GATE_HISTORY, SPH_GATE_RECT, SPH_GATE_ELLIPSE, SPH_GATE_UNBOUNDED, SphGate, SphGateBooks, GATE_DTYPE, GATE_BOOKS_DTYPE,
    gate, gate_box, gate_array, gate_discharge, gates_step_host,
    SPH_MAX_MONITORS, SPH_MAX_MONITOR_POINTS, SPH_MAX_MONITOR_HISTORY, SPH_MONITOR_NONE, SPH_MONITOR_POINTS, SPH_MONITOR_LATTICE, SPH_MONITOR_FIELDS,
    SPH_MONITOR_WET_SHARE, SPH_MONITOR_MEAN_FRACTION, SPH_MONITOR_VAR_FRACTION, SPH_MONITOR_MEAN_DENSITY, SPH_MONITOR_MEAN_PRESSURE,
    SPH_MONITOR_VAR_PRESSURE, SPH_MONITOR_MEAN_VEL_X, SPH_MONITOR_MEAN_VEL_Y, SPH_MONITOR_MEAN_VEL_Z, SPH_MONITOR_TKE,
    SphMonitorConfig, SphMonitorRow, SphMonitorInfo, MONITOR_ROW_DTYPE, monitor_config, monitor_accumulate_host, monitor_field_host,
    monitor_schedule_host, monitor_means,
    SPH_OPT_DIFFUSE_TIMED, SPH_DIFFUSE_SPRAY, SPH_DIFFUSE_FOAM, SPH_DIFFUSE_BUBBLE, SphDiffuse, SphDiffuseConfig, SphDiffuseInfo, DIFFUSE_DTYPE, diffuse_config,
    diffuse_step_host, write_points_ply, SphDiffuseCrest, SphDiffuseCrestInfo, diffuse_crest_config,
    SPH_OPT_NEIGHBORS_FILL, SPH_NEIGHBORS_SELF, SPH_NEIGHBORS_HALF, SPH_NEIGHBORS_COUNT_ONLY, SphNeighborInfo, neighbors_host,
    SPH_OPT_COMPONENTS_VARIANT, SPH_COMPONENTS_FLUID_ONLY, SPH_COMPONENT_NONFINITE, SphComponent, SphComponentInfo, COMPONENT_DTYPE, components_host,
    component_centers,
    SPH_OPT_KNN_VARIANT, SPH_KNN_SELF, SPH_KNN_FLUID_ONLY, SPH_KNN_MAX_K, SphKnnInfo, knn_host,
    SPH_OPT_RAYS_VARIANT, SPH_RAYS_FLUID_ONLY, SPH_RAYS_ANY_HIT, SphRayHit, SphRaysInfo, RAY_HIT_DTYPE, rays_host, camera_rays, parallel_rays,
    SPH_OPT_RAY_SPANS_VARIANT, SphRaySpan, SphRaySpansInfo, RAY_SPAN_DTYPE, ray_spans_host, ray_spans_walk_host, ray_thickness,
    SPH_OPT_SHELL_TIMED, SPH_SHELL_FLUID_ONLY, SPH_SHELL_MEMBER, SPH_SHELL_ISOLATED, SphShell, SphShellConfig, SphShellInfo, SHELL_DTYPE, shell_host,
    shell_config,
    SPH_ANISO_FLUID_ONLY, SPH_ANISO_VALID, SPH_ANISO_SPARSE, SPH_ANISO_CLAMPED, SphAniso, SphAnisoConfig, SphAnisoInfo, ANISO_DTYPE, aniso_config,
    aniso_host, aniso_lattice_host,
    SPH_OPT_AGGREGATE_VARIANT, SPH_AGGREGATE_SUM, SPH_AGGREGATE_MEAN, SPH_AGGREGATE_MAX, SPH_AGGREGATE_MIN, SPH_AGGREGATE_WEIGHT_ONE,
    SPH_AGGREGATE_WEIGHT_POLY6, SPH_AGGREGATE_SELF, SPH_AGGREGATE_FLUID_ONLY, SPH_AGGREGATE_DELTA, SPH_AGGREGATE_MOMENTS,
    SPH_AGGREGATE_MAX_CHANNELS, SphAggregateConfig, SphAggregateInfo, aggregate_config, aggregate_host,
    aggregate_adjoint_host, aggregate_arg_host, aggregate_route_host, aggregate_position_grad_host,
    SPH_BASIS_GRID, SphBasisConfig, basis_config, aggregate_basis_host, aggregate_basis_adjoint_host, aggregate_basis_position_grad_host,
    SPH_STATE_FORMAT, SPH_STATE_CHECKSUM_MIX64, SPH_STATE_MAGIC, STATE_SECTIONS, SphStateInfo, SphStateDigest, SphStateHeader, SphStateEntry, SphStateCore,
    STATE_HEADER_DTYPE, STATE_ENTRY_DTYPE, state_info, state_checksum_host, state_sections,
)
from .autograd import EngineAggregateBackend, HostAggregateBackend, aggregate_autograd, continuous_conv  # noqa: F401
from . import build, synthetic  # noqa: F401
