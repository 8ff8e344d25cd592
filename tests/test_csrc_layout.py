"""The two rules of csrc/ that are text: the build watches every header, and the headers include each other by layer.  No GPU."""
import os
import re

from conftest import PKG_NAME, ROOT

CSRC = os.path.join(ROOT, PKG_NAME, "csrc")

# The layers of csrc/ (DESIGN.md "Headers"): a feature header is every header not named here.
BASE = {"sph_device.h", "sph_host.h", "sph_shapes_ext.h", "sph_wave.h"}     # and include/sph_abi.h
SUBSTEP = {"sph_kernels.h", "sph_pass.h", "sph_walk.h"}
SHARED = {"sph_sample.h", "sph_query.h"}
# A feature built on another feature: including header -> the features it may include.  Each is named in that header's comment.
BUILT_ON = {"sph_couple.h": {"sph_scalar.h", "sph_obstacle.h"}, "sph_obstacle.h": {"sph_volume.h"}, "sph_diffuse.h": {"sph_tracer.h"}}


def headers():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))


def test_build_watches_every_header(pkg):
    listed = {os.path.basename(h) for h in pkg.build.HEADERS}
    assert set(headers()) <= listed, sorted(set(headers()) - listed)
    assert "sph_abi.h" in listed


def test_feature_headers_include_by_layer():
    features = set(headers()) - BASE - SUBSTEP - SHARED
    assert BASE | SUBSTEP | SHARED <= set(headers())
    for name in sorted(features):
        with open(os.path.join(CSRC, name)) as fh:
            included = {os.path.basename(m) for m in re.findall(r'^#include "([^"]+)"', fh.read(), re.M)}
        others = (included & features) - BUILT_ON.get(name, set())
        assert not others, f"{name} includes the feature header(s) {sorted(others)}"
