"""Checkpoints on the GPU: the device digest against its host twin, saves that leave no trace, and runs that are
saved, loaded into another engine and continued, against the uninterrupted run -- bit for bit, for the records and every output of the
features a blob carries (tracers, the diffuse pool with crest births, scalars with buoyancy and sources, obstacles with a dynamic and a
volume-bound body, gates, monitors, fountain and river mode).

The numbers make the phases matter: saved after A = 5 substeps, continued for B = 7; tracer stride 3, monitor every 4, gate stride 2, crest every 4, and
rings (3, 4 and 2 rows) that wrap within A + B."""
import numpy as np
import pytest

from conftest import small_scene
import state_ref as S
import support as T
from state_scenes import FEATURES, gates_on, outputs, same_outputs, tracers_on

pytestmark = pytest.mark.gpu
A, B = 5, 7


@pytest.fixture(scope="module")
def scene(pkg):
    return small_scene(pkg, n=4096, grid=16, seed=3)


@pytest.fixture(scope="module")
def other(pkg):
    """The engine a blob is loaded into starts from another n and other members."""
    rec, sp = small_scene(pkg, n=1000, grid=12, seed=9)
    sp.param_viscosity = 2.0
    return rec, sp


def run_a(f, steps):
    """`steps` substeps as single dispatches and one sph_dispatch_n."""
    f.DispatchCompute()
    if steps > 3:
        f.DispatchN(steps - 3)
        steps = 3
    for _ in range(steps - 1):
        f.DispatchCompute()


def continued(pkg, scene, other, names, mode, before=None):
    """Run A (set up, A substeps, save, B substeps) against run B (another engine with junk of the same features, load, B substeps under
    another pass variant and record mode; mode "graph": the B substeps as one dispatch and three sph_dispatch_n(2), the last a replay)."""
    rec, sp = scene
    fa = T.engine(pkg, rec, sp, kern=3, aos=1)
    if before:
        before(fa)
    for name in names:
        FEATURES[name][0](pkg, fa, rec)
    run_a(fa, A)
    blob = fa.save_state()
    at_save = fa.state_digest()
    peek = pkg.state_info(blob)
    assert {k: v["sum"] for k, v in peek["sections"].items()} == at_save and set(at_save) == {"core", "particles", *names}
    run_a(fa, B)
    want, want_digest = outputs(fa, names), fa.state_digest()
    fa.close()

    fb = T.engine(pkg, *other, kern=2, aos=0, graph=1 if mode == "graph" else 0)
    for name in names:
        FEATURES[name][0](pkg, fb, other[0], junk=True)
    fb.DispatchN(2)
    fb.load_state(blob)
    assert fb.state_digest() == at_save and fb.GetNumFluids() == len(rec)
    assert bytes(fb.params) == bytes(peek["params"]) and fb.numParticles == len(rec)
    T.same_bits(fb.particles, np.frombuffer(blob[peek["sections"]["particles"]["offset"]:][:80 * len(rec)].tobytes(), pkg.PARTICLE_DTYPE), "initial particles")
    if mode == "graph":
        fb.DispatchCompute()
        for _ in range(3):
            fb.DispatchN(2)
        assert fb.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) >= 2
    else:
        run_a(fb, B)
    same_outputs(outputs(fb, names), want, f"{names} {mode}")
    assert fb.state_digest() == want_digest
    fb.close()


# ---- the baseline: the core continues from the records alone ---------------------------------------------------------------
def test_core_continues_from_records_alone(pkg, scene):
    """Nothing of this feature: download, create_from_particles, continue (what the particles section relies on)."""
    rec, sp = scene
    fa = T.engine(pkg, rec, sp)
    run_a(fa, A)
    mid = fa.download()
    run_a(fa, B)
    fb = T.engine(pkg, mid, sp, kern=2, aos=0)
    run_a(fb, B)
    T.same_bits(fb.download(), fa.download(), "continued from records")
    fa.close(); fb.close()


# ---- the digest and its twin --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd_records(pkg):
    rec, sp = small_scene(pkg, n=4097, grid=18, seed=3)
    rec = rec.copy()
    bits = rec["padB"].view(np.uint32)
    bits[0::7] = 0x7FC12345                                            # NaN payloads
    bits[1::7] = 0x00000001                                            # a denormal
    rec["vel"].view(np.uint32)[2::5, 1] = 0x80000000                    # -0.0
    rec["acc"].view(np.uint32)[::3, 3] = 0xFFC00001
    rec["pad0"][::2] = -7
    return rec, sp


@pytest.mark.parametrize("aos", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_particle_digest_equals_host_checksum(pkg, odd_records, n, aos):
    rec, sp = odd_records
    f = T.engine(pkg, rec[:n], sp, aos=aos)
    assert f.state_digest(["particles"]) == {"particles": pkg.state_checksum_host(rec[:n])} and pkg.state_checksum_host(rec[:n]) == S.checksum(rec[:n].tobytes())
    f.DispatchCompute()
    assert f.state_digest()["particles"] == pkg.state_checksum_host(f.download())
    f.DispatchN(2)
    assert f.state_digest()["particles"] == S.checksum(f.download().tobytes())
    f.close()


def test_every_section_digest_equals_the_blob(pkg, scene):
    rec, sp = scene
    f = T.engine(pkg, rec, sp)
    f.SetStencilTargets(np.ones((3, 4), np.float32))
    for name in FEATURES:
        FEATURES[name][0](pkg, f, rec)
    for _ in range(2):
        run_a(f, A)
        blob = f.save_state()
        info, twin = pkg.state_info(blob), pkg.state_sections(blob)
        assert f.state_digest() == {k: v["sum"] for k, v in info["sections"].items()} and set(info["sections"]) == {"core", "particles", *FEATURES}
        assert info["sections"] == twin["sections"] and info["n"] == twin["n"] == len(rec)
        for name, s in info["sections"].items():                      # the stored sums are the restatement's over the payload
            assert S.checksum(blob[s["offset"]:s["offset"] + s["bytes"]]) == s["sum"], name
    # the set-ups of state_scenes are not idle: every feature has done something a continuation can get wrong
    info, crest = f.diffuse_info(), f.diffuse_crest_info()
    print(info, crest, f.scalar_injected(), f.obstacle_impulses()[0])
    assert info["alive"] > 0 and info["spawned"] > 0 and info["diedLife"] + info["diedAge"] > 0 and crest["acting"] == 3 and crest["crestSpawned"] > 0
    assert f.scalar_injected()[1].min() > 0 and np.abs(f.obstacle_impulses()[0]).max(axis=1).min() > 0.0
    assert f.gate_books()[0]["forward"].sum() + f.gate_books()[0]["backward"].sum() > 0 and f.monitor_rows(0)["wet"].sum() > 0
    f.close()


# ---- a save is invisible ------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
def test_a_save_is_invisible(pkg, scene, graph):
    rec, sp = scene
    names = list(FEATURES)

    def run(save):
        f = T.engine(pkg, rec, sp, graph=graph)
        for name in names:
            FEATURES[name][0](pkg, f, rec)
        for _ in range(4 if graph else 3):
            if graph:
                f.DispatchN(2)                                          # (seen, seen with the state in place, captured and launched, replayed)
            else:
                f.DispatchCompute()
            if save:
                f.save_state()
                f.state_digest()
        if graph:
            assert f.get_option(pkg.SPH_OPT_GRAPH_LAUNCHES) >= 2
        out = outputs(f, names)
        f.close()
        return out
    same_outputs(run(True), run(False), f"saves, graph {graph}")


# ---- continuation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("names", [(), ("tracers",), ("diffuse",), ("scalars",), ("obstacles",), ("gates",), ("monitors",), tuple(FEATURES)], ids=lambda n: "+".join(n) or "core")
def test_saved_loaded_and_continued(pkg, scene, other, names, mode):
    continued(pkg, scene, other, names, mode)


def test_fountain_mode_continues(pkg, scene, other):
    """The seed advances with every dispatch: it is part of the core section."""
    def fountain(f):
        f.fountainMode = 1
        f.fountainOffset = (0.0, -1.0, 0.0)
        f.fountainRadius = 0.6
    continued(pkg, scene, other, ("tracers",), "eager", before=fountain)


def test_river_mode_continues(pkg, scene, other):
    def river(f):
        f.terrainW, f.terrainH = 24, 17
        f.GenerateRiverTerrain(4)
        f.riverMode = 1
    continued(pkg, scene, other, ("gates",), "eager", before=river)


# ---- refusals leave no trace ------------------------------------------------------------------------------------
def test_damaged_blobs_leave_the_engine_unchanged(pkg, scene):
    rec, sp = scene
    f = T.engine(pkg, rec, sp)
    for name in FEATURES:
        FEATURES[name][0](pkg, f, rec)
    run_a(f, A)
    before, out_before = f.state_digest(), outputs(f, list(FEATURES))
    good, damaged = S.damaged_blobs(pkg, rec[:500], sp)
    for name, blob, word in damaged:
        with pytest.raises(pkg.SphError, match="error -1:.*" + word):
            f.load_state(blob)
        assert f.state_digest() == before, name
    bad = pkg.default_params()
    bad.param_h = -1.0                                                  # intact, but what it carries no set call would take
    with pytest.raises(pkg.SphError, match="param_h"):
        f.load_state(S.build_blob(pkg, rec[:500], bad))
    assert f.state_digest() == before
    same_outputs(outputs(f, list(FEATURES)), out_before, "after refusals")
    f.load_state(good)                                                  # and the intact blob loads: features gone, 500 particles
    assert set(f.state_digest()) == {"core", "particles"} and f.GetNumFluids() == 500 and f.num_tracers() == 0
    f.close()


def test_slab_engines_and_linked_list_grids_refuse(pkg, scene):
    rec, sp = scene
    blob = S.build_blob(pkg, rec, sp)
    L = pkg.load_library()
    import ctypes as C
    with T.slab_engine(pkg, rec, sp) as slab:
        need = C.c_size_t()
        assert L.sph_state_size(slab._h, C.byref(need)) == -3
        assert L.sph_state_save(slab._h, None, 0, C.byref(need)) == -3
        assert L.sph_state_load(slab._h, blob.ctypes.data_as(C.c_void_p), blob.size) == -3 and b"slab" in L.sph_last_error()
    f = T.engine(pkg, rec, sp)
    need = C.c_size_t()
    assert L.sph_state_save(f._h, None, 0, C.byref(need)) == -4 and need.value == len(f.save_state())      # SPH_ERR_CAPACITY, and the need
    f.close()
    f = T.engine(pkg, rec, sp)
    tracers_on(pkg, f, rec)
    with_tracers = f.save_state()
    with T.linked_list_grid(pkg, f):
        before = f.state_digest()
        with pytest.raises(pkg.SphError, match="error -3:.*SPH_OPT_GRID_BUILD"):
            f.load_state(with_tracers)
        assert f.state_digest() == before
        f.load_state(blob)                                              # no feature sections: the linked-list engine takes it
    f.close()


def test_a_load_drops_query_results(pkg, scene):
    """Every query family's result is "no result" after a load, as after a reset: the *_info getters say so."""
    rec, sp = scene
    f = T.engine(pkg, rec, sp)
    blob = f.save_state()
    c, ext = T.fluid_block(rec)
    rays = pkg.parallel_rays(c + np.float32([0, ext, 0]), (0.3 * ext, 0, 0), (0, 0, 0.3 * ext), (0, -1, 0), 4, 4)
    f.neighbors(count_only=True)
    f.components()
    f.knn(4)
    f.raycast(rays)
    f.ray_spans(rays)
    f.shell()
    f.anisotropy()
    f.surface()
    getters = (f.component_info, f.knn_info, f.rays_info, f.ray_spans_info, f.shell_info, f.aniso_info)
    assert f.neighbor_info().kind != 0
    for get in getters:
        get()
    L = pkg.load_library()
    assert L.sph_surface_download(f._h, None, 0, None, 0) != -3             # (a surface exists: too small a capacity is another refusal)
    f.load_state(blob)
    assert f.neighbor_info().kind == 0
    for get in getters:
        with pytest.raises(pkg.SphError):
            get()
    assert L.sph_surface_download(f._h, None, 0, None, 0) == -3 and b"no surface" in L.sph_last_error()
    f.close()


def test_checkpoint_resume_example(pkg, tmp_path):
    exe = T.build_example(pkg, "checkpoint_resume", tmp_path, werror=True)
    res = T.run_example(exe, [21, 19, 6000, tmp_path / "resume.sphstate"], timeout=120)
    assert res.returncode == 0 and "checkpoint_resume OK" in res.stdout, res.stdout + res.stderr


def test_from_state_and_files(pkg, scene, tmp_path):
    rec, sp = scene
    f = T.engine(pkg, rec, sp)
    gates_on(pkg, f, rec)
    run_a(f, A)
    path = str(tmp_path / "run.sphstate")
    blob = f.save_state(path)
    g = pkg.SPHFluidGPU.from_state(path)
    assert g.state_digest() == f.state_digest() and bytes(g.params) == bytes(f.params) and g.numParticles == len(rec)
    run_a(f, B)
    run_a(g, B)
    same_outputs(outputs(f, ["gates"]), outputs(g, ["gates"]), "from_state")
    assert np.array_equal(np.fromfile(path, np.uint8), blob)
    f.close(); g.close()
