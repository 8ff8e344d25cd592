"""The C calls behind the numpy paths of the anisotropic kernels of SPHFluidGPU, in order and with their scalar arguments:
anisotropy(), aniso_rows(), aniso_info() and aniso_surface(), with a recording stand-in in place of the loaded library, in the manner
of test_binding_calls.py: the _push_params() before every build, the info call before the download, the null pointer that stands for an
empty array, and the config as the library receives it.  No GPU."""
import ctypes as C

import numpy as np
import pytest

F = np.float32
HANDLE = 0x5EED
H = "handle"
P = "pointer"
INFO = dict(SphAnisoInfo=dict(rows=5, numSparse=1, numClamped=2, maxCount=40), SphSurface=dict(numVertices=4, numTriangles=2))


class Recorder:
    """Stands in for the library: every attribute is a function that records (name, arguments) and returns 0.  A handle is recorded as
    H, any other address as P, a null pointer as None, an array of three as its tuple, a struct by reference as "&" and its type, or,
    for SphAnisoConfig, its fields."""

    def __init__(self, info):
        self.calls, self.info = [], info

    def _seen(self, a):
        if isinstance(a, C.c_void_p):
            return None if not a.value else H if a.value == HANDLE else P
        if a is None or isinstance(a, (int, float)):
            return a
        if isinstance(a, C.Array):
            return tuple(a)
        obj = a._obj                                                              # (ctypes.byref)
        name = type(obj).__name__
        if name == "SphAnisoConfig":
            return (name, obj.radius, obj.support, obj.smoothing, obj.maxRatio, obj.maxStretch, obj.sparseScale, obj.minCount, obj.flags)
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
    made = []

    def make(info=INFO):
        f = object.__new__(pkg.SPHFluidGPU)
        f._L, f._p, f._h = Recorder(info), pkg.default_params(), C.c_void_p(HANDLE)
        made.append(f)
        return f
    yield make
    for f in made:
        f._h = C.c_void_p()                                                       # (nothing for close() to destroy)


PUSH = ("sph_set_params", H, "&SphParams")
DEFAULT = ("SphAnisoConfig", 0.0, 0.0, F(0.9), 4.0, 1.5, 0.5, 25, 0)


def test_anisotropy(pkg, engine):
    f = engine()
    rows = f.anisotropy()
    assert f._L.calls == [PUSH, ("sph_aniso_build", H, DEFAULT, "&SphAnisoInfo"), ("sph_aniso_info", H, "&SphAnisoInfo"), ("sph_aniso_download", H, P)]
    assert (rows.dtype, rows.shape) == (pkg.ANISO_DTYPE, (5,))
    f = engine(dict(INFO, SphAnisoInfo=dict(rows=0)))
    rows = f.anisotropy(0.5, support=0.25, smoothing=0.5, max_ratio=2.0, max_stretch=1.25, min_count=3, sparse_scale=0.75, fluid_only=True)
    assert f._L.calls[1] == ("sph_aniso_build", H, ("SphAnisoConfig", 0.5, 0.25, 0.5, 2.0, 1.25, 0.75, 3, pkg.SPH_ANISO_FLUID_ONLY), "&SphAnisoInfo")
    assert f._L.calls[-1] == ("sph_aniso_download", H, None) and rows.shape == (0,)


def test_rows_and_info(pkg, engine):
    f = engine()
    info = f.aniso_info()
    assert type(info).__name__ == "SphAnisoInfo" and (info.rows, info.numSparse, info.numClamped, info.maxCount) == (5, 1, 2, 40)
    rows = f.aniso_rows()
    assert f._L.calls == [("sph_aniso_info", H, "&SphAnisoInfo"), ("sph_aniso_info", H, "&SphAnisoInfo"), ("sph_aniso_download", H, P)]
    assert rows.shape == (5,)


def test_aniso_surface(pkg, engine):
    f = engine()
    v, t = f.aniso_surface((0.5, 1.0, 1.5), 0.25, (4, 5, 6), iso=0.75, min_count=7)
    cfg = ("SphAnisoConfig", 0.0, 0.0, F(0.9), 4.0, 1.5, 0.5, 7, 0)
    assert f._L.calls == [PUSH, ("sph_aniso_surface", H, cfg, (0.5, 1.0, 1.5), (0.25, 0.25, 0.25), (4, 5, 6), 0.75, "&SphSurface", "&SphAnisoInfo"),
                          ("sph_surface_download", H, P, 4, P, 2)]
    assert (v.dtype, v.shape, t.dtype, t.shape) == (pkg.SURFACE_VERTEX_DTYPE, (4,), np.uint32, (2, 3))


def test_config_and_twin_arguments(pkg):
    cfg = pkg.aniso_config(maxRatio=2.0, minCount=9)
    assert (cfg.maxRatio, cfg.minCount, cfg.maxStretch) == (2.0, 9, 1.5)
    with pytest.raises(TypeError):
        pkg.aniso_host(np.zeros(0, pkg.PARTICLE_DTYPE), pkg.default_params(), nothing=1)
