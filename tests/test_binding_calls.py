"""The C calls behind the numpy paths of the spatial queries of SPHFluidGPU, in order and with their scalar arguments: neighbors(),
components(), knn(), raycast(numpy rays), shell() and the five *_info getters, with a recording stand-in in place of the loaded
library.  The expectations are written down from the binding as it stood when the five families each spelled their calls out; they pin
the _push_params() before every build, the info call before every download and the null pointer that stands for an empty array.
No GPU."""
import ctypes as C

import numpy as np
import pytest

F = np.float32
HANDLE = 0x5EED
H = "handle"
P = "pointer"
# what the stand-in writes into the info struct a call is given
INFO = dict(SphNeighborInfo=dict(rows=5, total=7, flags=0), SphComponentInfo=dict(rows=5, numComponents=2), SphKnnInfo=dict(rows=5, k=8),
            SphRaysInfo=dict(rays=3), SphShellInfo=dict(rows=5, numShell=2))
EMPTY = {name: {} for name in INFO}


class Recorder:
    """Stands in for the library: every attribute is a function that records (name, arguments) and returns 0.  A handle is recorded as
    H, any other address as P, a null pointer as None, a struct by reference as "&" and its type, or, for SphShellConfig, its fields."""

    def __init__(self, info):
        self.calls, self.info = [], info

    def _seen(self, a):
        if isinstance(a, C.c_void_p):
            return None if not a.value else H if a.value == HANDLE else P
        if a is None or isinstance(a, (int, float)):
            return a
        obj = a._obj                                                              # (ctypes.byref)
        if isinstance(obj, C.c_void_p):
            obj.value = 0x1000                                                    # (sph_neighbors_device lends two addresses)
            return "&address"
        name = type(obj).__name__
        if name == "SphShellConfig":
            return (name, obj.radius, obj.offset, obj.minCount, obj.flags)
        for field, value in self.info.get(name, {}).items():
            setattr(obj, field, value)
        return "&" + name

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, *[self._seen(a) for a in args]))
            return 0
        return call


@pytest.fixture
def engine(pkg):
    """(make, h): make(info) is an SPHFluidGPU around a Recorder, with no device behind it; h is its param_h."""
    made = []

    def make(info=INFO):
        f = object.__new__(pkg.SPHFluidGPU)
        f._L, f._p, f._h = Recorder(info), pkg.default_params(), C.c_void_p(HANDLE)
        made.append(f)
        return f
    yield make, pkg.default_params().param_h
    for f in made:
        f._h = C.c_void_p()                                                       # (nothing for close() to destroy)


PUSH = ("sph_set_params", H, "&SphParams")


def test_neighbors(pkg, engine):
    make, h = engine
    lists = [("sph_neighbors_info", H, "&SphNeighborInfo"), ("sph_neighbors_device", H, "&address", "&address")]
    f = make()
    off, idx = f.neighbors()
    assert f._L.calls == [PUSH, ("sph_neighbors_build", H, h, 0, 0, "&SphNeighborInfo"), *lists, ("sph_neighbors_download", H, P, P, 7)]
    assert (off.dtype, off.shape, idx.dtype, idx.shape) == (np.int64, (6,), np.int32, (7,))
    f = make()
    f.neighbors(0.5, half=True, max_pairs=9)
    assert f._L.calls[1] == ("sph_neighbors_build", H, 0.5, pkg.SPH_NEIGHBORS_HALF, 9, "&SphNeighborInfo")
    f = make(dict(INFO, SphNeighborInfo=dict(rows=5, total=7, flags=pkg.SPH_NEIGHBORS_COUNT_ONLY)))
    off, idx = f.neighbors(self_=True, count_only=True)
    assert f._L.calls == [PUSH, ("sph_neighbors_build", H, h, pkg.SPH_NEIGHBORS_SELF | pkg.SPH_NEIGHBORS_COUNT_ONLY, 0, "&SphNeighborInfo"), *lists,
                          ("sph_neighbors_download", H, P, None, 7)]
    assert idx is None
    f = make(dict(INFO, SphNeighborInfo=dict(rows=0, total=0, flags=0)))          # no pair: the empty index array still goes as it is
    off, idx = f.neighbors()
    assert f._L.calls[-1] == ("sph_neighbors_download", H, P, P, 0) and off.shape == (1,) and idx.shape == (0,)


def test_components(pkg, engine):
    make, h = engine
    f = make()
    labels, roots, table = f.components()
    assert f._L.calls == [PUSH, ("sph_components_build", H, h, 0, "&SphComponentInfo"), ("sph_components_download", H, P, P, P, 2)]
    assert (labels.dtype, labels.shape, roots.dtype, roots.shape, table.dtype, table.shape) == (np.int32, (5,), np.int32, (5,), pkg.COMPONENT_DTYPE, (2,))
    f = make(EMPTY)
    res = f.components(0.25, fluid_only=True)
    assert f._L.calls == [PUSH, ("sph_components_build", H, 0.25, pkg.SPH_COMPONENTS_FLUID_ONLY, "&SphComponentInfo"),
                          ("sph_components_download", H, None, None, None, 0)]
    assert isinstance(res, tuple) and [len(x) for x in res] == [0, 0, 0]


def test_knn(pkg, engine):
    make, h = engine
    f = make()
    idx, d2, cnt = f.knn(8)
    assert f._L.calls == [PUSH, ("sph_knn_build", H, 8, h, 0, "&SphKnnInfo"), ("sph_knn_info", H, "&SphKnnInfo"), ("sph_knn_download", H, P, P, P)]
    assert (idx.dtype, idx.shape, d2.dtype, d2.shape, cnt.dtype, cnt.shape) == (np.int32, (5, 8), F, (5, 8), np.uint32, (5,))
    f = make(dict(INFO, SphKnnInfo=dict(rows=0, k=4)))
    res = f.knn(4, 0.5, self_=True, fluid_only=True)
    assert f._L.calls[1] == ("sph_knn_build", H, 4, 0.5, pkg.SPH_KNN_SELF | pkg.SPH_KNN_FLUID_ONLY, "&SphKnnInfo")
    assert f._L.calls[-1] == ("sph_knn_download", H, None, None, None) and isinstance(res, tuple) and res[0].shape == (0, 4)


def test_raycast_of_numpy_rays(pkg, engine):
    make, h = engine
    f = make()
    t, ids, pos, nrm = f.raycast(np.zeros((3, 8), F))
    assert f._L.calls == [PUSH, ("sph_rays_cast", H, P, 3, 0.25 * h, 0, "&SphRaysInfo"), ("sph_rays_info", H, "&SphRaysInfo"), ("sph_rays_download", H, P)]
    assert (t.dtype, t.shape, ids.dtype, ids.shape, pos.shape, nrm.shape) == (F, (3,), np.int32, (3,), (3, 3), (3, 3))
    f = make(EMPTY)
    f.raycast(np.zeros((0, 8), F), 0.125, fluid_only=True, any_hit=True)
    assert f._L.calls == [PUSH, ("sph_rays_cast", H, None, 0, 0.125, pkg.SPH_RAYS_FLUID_ONLY | pkg.SPH_RAYS_ANY_HIT, "&SphRaysInfo"),
                          ("sph_rays_info", H, "&SphRaysInfo"), ("sph_rays_download", H, None)]


def test_shell(pkg, engine):
    make, h = engine
    f = make()
    rows, ids = f.shell()
    assert f._L.calls == [PUSH, ("sph_shell_build", H, ("SphShellConfig", 0.0, F(0.10), 0, 0), "&SphShellInfo"), ("sph_shell_info", H, "&SphShellInfo"),
                          ("sph_shell_download", H, P, P)]
    assert (rows.dtype, rows.shape, ids.dtype, ids.shape) == (pkg.SHELL_DTYPE, (5,), np.int32, (2,))
    f = make(dict(INFO, SphShellInfo=dict(rows=5, numShell=0)))
    f.shell(0.5, offset=0.25, min_count=3, fluid_only=True)
    assert f._L.calls[1] == ("sph_shell_build", H, ("SphShellConfig", 0.5, 0.25, 3, pkg.SPH_SHELL_FLUID_ONLY), "&SphShellInfo")
    assert f._L.calls[-1] == ("sph_shell_download", H, P, None)


def test_info_getters(pkg, engine):
    make, _ = engine
    f = make()
    for method, kind in (("neighbor_info", "SphNeighborInfo"), ("component_info", "SphComponentInfo"), ("knn_info", "SphKnnInfo"),
                         ("rays_info", "SphRaysInfo"), ("shell_info", "SphShellInfo")):
        info = getattr(f, method)()
        assert type(info).__name__ == kind and all(getattr(info, k) == v for k, v in INFO[kind].items())
    assert f._L.calls == [("sph_neighbors_info", H, "&SphNeighborInfo"), ("sph_components_info", H, "&SphComponentInfo"), ("sph_knn_info", H, "&SphKnnInfo"),
                          ("sph_rays_info", H, "&SphRaysInfo"), ("sph_shell_info", H, "&SphShellInfo")]
