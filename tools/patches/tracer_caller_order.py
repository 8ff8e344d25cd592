"""Variant patch: the tracers are processed in the caller's order (the processing order stays the identity k_tracer_seed writes; no cell
sort), i.e. k_sample_points plus an update.  The shipped engine sorts the processing order by cell every kTracerRefresh substeps.
usage: tracer_caller_order.py <csrc dir>"""
import os, sys
d = sys.argv[1]
p = os.path.join(d, "sph_engine.hip")
s = open(p).read()
a = "    if (!e->trM || e->capturing) return SPH_OK;\n"
assert s.count(a) == 1
s = s.replace(a, "    return SPH_OK;                                   // variant: caller order\n" + a)
open(p, "w").write(s)
