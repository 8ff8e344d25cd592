"""Field monitors without a GPU (include/sph_abi.h "field monitors"): the host twins sph_monitor_accumulate_host
and sph_monitor_field_host run the __host__ __device__ functions the kernels run, and must give the bytes of the numpy restatement
(tests/monitor_ref.py); the counters' rule as a pure function; the record layouts against C99."""
import numpy as np
import pytest

import monitor_ref as MR
from support import c_layout, same_bits

FIELDS = list(range(10))
VARIANCES = (MR.VAR_FRACTION, MR.VAR_PRESSURE, MR.TKE)


def test_dtypes_and_constants(pkg):
    assert pkg.MONITOR_ROW_DTYPE.itemsize == 128 and pkg.SPH_MONITOR_FIELDS == 10
    assert [pkg.MONITOR_ROW_DTYPE.fields[n][1] for n in MR.ROW_DTYPE.names] == [MR.ROW_DTYPE.fields[n][1] for n in MR.ROW_DTYPE.names]
    assert (pkg.SPH_MONITOR_WET_SHARE, pkg.SPH_MONITOR_MEAN_FRACTION, pkg.SPH_MONITOR_VAR_FRACTION, pkg.SPH_MONITOR_MEAN_DENSITY,
            pkg.SPH_MONITOR_MEAN_PRESSURE, pkg.SPH_MONITOR_VAR_PRESSURE, pkg.SPH_MONITOR_MEAN_VEL_X, pkg.SPH_MONITOR_MEAN_VEL_Y,
            pkg.SPH_MONITOR_MEAN_VEL_Z, pkg.SPH_MONITOR_TKE) == tuple(FIELDS)
    cfg = pkg.monitor_config()
    assert (cfg.every, cfg.wetFraction, cfg.history, cfg.stride, cfg.ringPoints) == (1, 0.5, 0, 1, 0)
    assert pkg.monitor_config(every=3, history=7).every == 3
    with pytest.raises(pkg.SphError):
        pkg.monitor_config(nosuch=1)


@pytest.mark.parametrize("wet_fraction", [0.5, 0.0, 0.93])
def test_twins_give_the_restatements_bytes(pkg, wet_fraction):
    """20 acting substeps of 700 random samples with every hard case: rows and all ten fields, byte for byte, after each."""
    rng = np.random.default_rng(11)
    twin = ref = None
    for step in range(20):
        s = MR.random_samples(rng, 700, wet_fraction)
        twin = pkg.monitor_accumulate_host(twin, s.view(pkg.SAMPLE_DTYPE), wet_fraction)
        ref = MR.update(ref, s, wet_fraction)
        same_bits(twin.view(np.uint8), ref.view(np.uint8), f"rows after {step + 1}")
        if step in (0, 1, 19):
            for which in FIELDS:
                same_bits(pkg.monitor_field_host(twin, which).view(np.uint32), MR.field(ref, which).view(np.uint32), f"field {which} after {step + 1}")
    assert (ref["samples"] < 20).any() and (ref["samples"] > 0).all()           # skipped samples show in the row's count
    mixed = (ref["wet"] > 0) & (ref["wet"] < ref["samples"])
    assert mixed.mean() > 0.3 or wet_fraction == 0.0


def test_hard_cases_by_hand(pkg):
    s = np.zeros(8, MR.SAMPLE_DTYPE)
    s["fraction"] = [0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.75, 0.75, 0.75, 0.0, 0.75, 1.0]
    s["density"] = [1, 2, 3, np.nan, 5, 0, 7, 8]
    s["pressure"] = [10, 20, -0.0, 40, np.inf, 0, 70, 80]
    s["vel"][:, 0] = [1, 2, -0.0, 4, 5, 0, 7, 3 * 2.0 ** 60]
    s["vel"][6, 2] = -np.inf
    s["count"] = 0xFFFFFFFF                                                     # (not a float: any value is fine)
    s["pad"] = np.nan                                                           # (nor is the pad read)
    r = pkg.monitor_accumulate_host(None, s.view(pkg.SAMPLE_DTYPE))
    assert r["samples"].tolist() == [1, 1, 1, 0, 0, 1, 0, 1]                     # NaN / inf anywhere: skipped whole
    assert r["wet"].tolist() == [1, 0, 1, 0, 0, 0, 0, 1]                         # the tie is wet, one ulp below is not, a zero record is dry
    assert r["sumPressure"][1] == 0.0 and r["sumDensity"][1] == 2.0              # a dry sample adds to the all-sample sums only
    assert not r[3].tobytes().strip(b"\0") and not r[4].tobytes().strip(b"\0") and not r[6].tobytes().strip(b"\0")
    assert r["sumVelVel"][7, 0] == 9 * 2.0 ** 120                                # an fp32 product is exact in fp64
    assert np.signbit(r["sumPressure"][2]) == np.signbit(np.float64(0.0) + np.float64(-0.0))
    same_bits(r.view(np.uint8), MR.update(None, s).view(np.uint8), "hand cases")


def test_one_sample_has_no_variance(pkg):
    """After one acting substep every variance and the TKE are exactly 0 and every mean is the sample (wet points)."""
    s = MR.random_samples(np.random.default_rng(5), 500, hard=False)
    s["fraction"][::2] = np.maximum(s["fraction"][::2], np.float32(0.5))
    r = pkg.monitor_accumulate_host(None, s.view(pkg.SAMPLE_DTYPE))
    wet = r["wet"] == 1
    assert wet.sum() > 250 and (r["samples"] == 1).all()
    for which in VARIANCES:
        v = pkg.monitor_field_host(r, which)
        assert (v == 0).all(), which
    same_bits(pkg.monitor_field_host(r, MR.MEAN_FRACTION), s["fraction"], "mean fraction")
    same_bits(pkg.monitor_field_host(r, MR.MEAN_DENSITY), s["density"], "mean density")
    same_bits(pkg.monitor_field_host(r, MR.MEAN_PRESSURE)[wet], s["pressure"][wet], "mean pressure")
    for a in range(3):
        same_bits(pkg.monitor_field_host(r, MR.MEAN_VEL_X + a)[wet], s["vel"][wet, a], f"mean velocity {a}")
    assert (pkg.monitor_field_host(r, MR.MEAN_PRESSURE)[~wet] == 0).all()       # 0 where the dividing count is 0
    assert (pkg.monitor_field_host(r, MR.WET_SHARE) == wet).all()
    empty = np.zeros(3, pkg.MONITOR_ROW_DTYPE)
    for which in FIELDS:
        assert (pkg.monitor_field_host(empty, which) == 0).all()


def test_shapes_and_refusals(pkg):
    s = MR.random_samples(np.random.default_rng(1), 24).reshape(2, 3, 4)
    r = pkg.monitor_accumulate_host(None, s.view(pkg.SAMPLE_DTYPE))
    assert r.shape == (2, 3, 4) and pkg.monitor_field_host(r, MR.TKE).shape == (2, 3, 4)
    m = pkg.monitor_means(r)
    assert m["vel"].shape == (2, 3, 4, 3) and m["reynolds"].shape == (2, 3, 4, 3, 3)
    L = pkg.load_library()
    assert L.sph_monitor_field_host(r.ctypes.data, r.size, 10, r.ctypes.data) == -1
    assert L.sph_monitor_field_host(None, 3, 0, None) == -1
    assert L.sph_monitor_accumulate_host(None, None, 5, 0.5) == -1
    assert L.sph_monitor_accumulate_host(r.ctypes.data, s.ctypes.data, s.size, float("nan")) == -1
    with pytest.raises(pkg.SphError):
        pkg.monitor_accumulate_host(r, s.reshape(-1)[:5].view(pkg.SAMPLE_DTYPE))


def test_which_substeps_act_and_which_ring_row_they_write(pkg):
    """The rule as a pure function over every, stride and history, with rings that wrap, against the function k_monitor_tick runs."""
    assert [c for c in range(10) if MR.acts(c, 3)] == [0, 3, 6, 9]
    assert [MR.ring_row(a, 4, 2) for a in range(12)] == [0, MR.NO_ROW, 1, MR.NO_ROW, 2, MR.NO_ROW, 3, MR.NO_ROW, 0, MR.NO_ROW, 1, MR.NO_ROW]
    assert MR.ring_row(5, 0, 1) == MR.NO_ROW
    for every in (1, 2, 3, 5, 8):
        for stride in (1, 2, 3):
            for history in (0, 1, 4, 7):
                acts, rows = pkg.monitor_schedule_host(every, stride, history, 200)
                want = MR.schedule(every, stride, history, 200)
                assert acts.tolist() == want[0].tolist() and rows.tolist() == want[1].tolist(), (every, stride, history)
                assert acts[0] == 1 and int(acts.sum()) == (200 + every - 1) // every
                if history:
                    assert rows[0] == 0 and MR.ring_span(int(acts.sum()), history, stride)[1] == min(history, (int(acts.sum()) + stride - 1) // stride)
    acts, rows = pkg.monitor_schedule_host(5, 2, 4, 48)                         # the GPU test's ring: 10 acting, rows 0 1 2 3 0
    assert [int(r) for r in rows[acts == 1]] == [0, MR.NO_ROW, 1, MR.NO_ROW, 2, MR.NO_ROW, 3, MR.NO_ROW, 0, MR.NO_ROW]
    assert MR.ring_span(10, 4, 2) == (1, 4)
    L = pkg.load_library()
    assert L.sph_monitor_schedule_host(0, 1, 0, 0, None, None) == -1 and L.sph_monitor_schedule_host(1, 0, 0, 0, None, None) == -1
    assert L.sph_monitor_schedule_host(1, 1, 4097, 0, None, None) == -1


def test_record_layouts_against_c99(pkg, tmp_path):
    size, offsets, extra = c_layout("SphMonitorRow", pkg.SphMonitorRow, [
        'printf("%d %d %d\\n", SPH_MAX_MONITORS, SPH_MAX_MONITOR_POINTS, SPH_MAX_MONITOR_HISTORY);',
        'printf("%d %d %d %d %d\\n", SPH_MONITOR_NONE, SPH_MONITOR_POINTS, SPH_MONITOR_LATTICE, SPH_MONITOR_WET_SHARE, SPH_MONITOR_TKE);'], tmp_path)
    assert size == 128 and offsets == [(n, getattr(pkg.SphMonitorRow, n).offset) for n, _ in pkg.SphMonitorRow._fields_]
    assert extra[0].split() == [str(pkg.SPH_MAX_MONITORS), str(pkg.SPH_MAX_MONITOR_POINTS), str(pkg.SPH_MAX_MONITOR_HISTORY)] == ["4", "4194304", "4096"]
    assert [int(x) for x in extra[1].split()] == [pkg.SPH_MONITOR_NONE, pkg.SPH_MONITOR_POINTS, pkg.SPH_MONITOR_LATTICE, pkg.SPH_MONITOR_WET_SHARE, pkg.SPH_MONITOR_TKE]
    for name, kind, want in (("SphMonitorConfig", pkg.SphMonitorConfig, 24), ("SphMonitorInfo", pkg.SphMonitorInfo, 112)):
        size, offsets, _ = c_layout(name, kind, [], tmp_path)
        assert size == want == __import__("ctypes").sizeof(kind)
        assert offsets == [(n, getattr(kind, n).offset) for n, _ in kind._fields_], name
