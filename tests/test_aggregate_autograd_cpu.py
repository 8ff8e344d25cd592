"""Autograd through the fused neighbourhood reductions on the CPU: the backward formulas of autograd.py over HostAggregateBackend (the
host twins) against the float64 dense Jacobian of aggregate_adjoint_ref.  values.grad after (y * g).sum().backward() must agree with
J^T g within (kmax + 8) * 2^-23 times the magnitudes of the terms the adjoint adds (aggregate_adjoint_ref: the bound of an fp32
recursive sum, per element here); for mean the bound is divided by the smallest non-zero W, because the adjoint is applied to g / W (the
fp32 W of the forward, itself within k u of the float64 W: (k + 3) u for the sums and k u for W stay below (k + 8) * 2^-23).  For max / min
the gradient is exact on integer-valued g.  No GPU."""
import numpy as np
import pytest

import aggregate_adjoint_ref as AJ
import query_scenes as QS

torch = pytest.importorskip("torch")
F = np.float32
R = 1.0                                    # two cells at h = 0.5


def scene(pkg):
    return QS.uniform(pkg, 300, 5)


def backward(pkg, rec, sp, x, g, points=None, **kw):
    """(y, values.grad) through the host backend."""
    xt = torch.from_numpy(x).requires_grad_(True)
    y = pkg.aggregate_autograd(pkg.HostAggregateBackend(rec, sp), points, xt, R, **kw)
    (y * torch.from_numpy(g)).sum().backward()
    return y.detach().numpy(), xt.grad.numpy()


SUM_MEAN = [dict(op="sum"), dict(op="sum", weight="poly6", self_=True), dict(op="sum", delta=True), dict(op="sum", moments=True),
            dict(op="sum", weight="poly6", self_=True, delta=True, moments=True), dict(op="mean"), dict(op="mean", weight="poly6"),
            dict(op="mean", delta=True), dict(op="mean", weight="poly6", self_=True, delta=True)]


@pytest.mark.parametrize("kw", SUM_MEAN, ids=str)
def test_sum_and_mean_against_the_dense_jacobian(pkg, kw):
    rec, sp = scene(pkg)
    n, c = len(rec), 3
    x = np.random.default_rng(1).normal(0.0, 1.0, (n, c)).astype(F)
    moments = kw.get("moments", False)
    g = np.random.default_rng(2).normal(0.0, 1.0, (n, 4, c) if moments else (n, c)).astype(F)
    y, grad = backward(pkg, rec, sp, x, g, **kw)
    host = {k: v for k, v in kw.items() if k != "op"}
    assert y.tobytes() == pkg.aggregate_host(rec, sp, x, R, op=kw["op"], **host).tobytes()          # the forward is aggregate()'s bytes
    A = AJ.dense(pkg, rec, sp, R, **host)
    g64 = g.astype(np.float64)
    scale = 1.0
    if kw["op"] == "mean":
        W = AJ.dense(pkg, rec, sp, R, weight=kw.get("weight", "one"), self_=kw.get("self_", False))[0].sum(axis=1)
        assert (W > 0).any()
        g64 = np.where((W > 0)[:, None], g64 / np.where(W > 0, W, 1.0)[:, None], 0.0)
        scale = 1.0 / W[W > 0].min()
    want = AJ.transpose_apply(A, g64)
    mag, k = AJ.adjoint_magnitudes(pkg, rec, sp, g, R, **host)
    bound = AJ.dot_bound(mag, int(k.max())) * scale
    err = np.abs(grad.astype(np.float64) - want)
    print(f"{kw}: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}, kmax {int(k.max())}")
    assert grad.dtype == F and grad.shape == (n, c) and np.abs(want).max() > 0 and (err <= bound).all()


@pytest.mark.parametrize("kw", [dict(op="max"), dict(op="min", self_=True), dict(op="max", delta=True), dict(op="min", self_=True, delta=True)], ids=str)
def test_max_and_min_are_exact_on_integer_gradients(pkg, kw):
    rec, sp = scene(pkg)
    n, c = len(rec), 4
    x = np.random.default_rng(3).integers(0, 4, (n, c)).astype(F)                       # few levels: ties everywhere, the id decides
    g = AJ.small_integers((n, c), 4)
    y, grad = backward(pkg, rec, sp, x, g, **kw)
    host = {k: v for k, v in kw.items() if k != "op"}
    assert y.tobytes() == pkg.aggregate_host(rec, sp, x, R, op=kw["op"], **host).tobytes()
    arg = AJ.winners(pkg, rec, sp, x, R, op=kw["op"], **host)
    want = AJ.route(arg, g, n)
    if kw.get("delta"):
        want -= np.where(arg >= 0, g.astype(np.float64), 0.0)
    assert (arg >= 0).any() and np.array_equal(grad.astype(np.float64), want)


def test_query_targets(pkg):
    rec, sp, pts = QS.query_cloud(pkg)
    n, m, c = len(rec), len(pts), 2
    x = np.random.default_rng(5).normal(0.0, 1.0, (n, c)).astype(F)
    for kw in (dict(op="sum", weight="poly6", moments=True), dict(op="mean")):
        moments = kw.get("moments", False)
        g = np.random.default_rng(6).normal(0.0, 1.0, (m, 4, c) if moments else (m, c)).astype(F)
        y, grad = backward(pkg, rec, sp, x, g, points=pts, **kw)
        host = {k: v for k, v in kw.items() if k != "op"}
        A = AJ.dense(pkg, rec, sp, R, points=pts, **host)
        g64, scale = g.astype(np.float64), 1.0
        if kw["op"] == "mean":
            W = A[0].sum(axis=1)
            g64 = np.where((W > 0)[:, None], g64 / np.where(W > 0, W, 1.0)[:, None], 0.0)
            scale = 1.0 / W[W > 0].min()
        mag, k = AJ.adjoint_magnitudes(pkg, rec, sp, g, R, points=pts, **host)
        err = np.abs(grad.astype(np.float64) - AJ.transpose_apply(A, g64))
        assert (err <= AJ.dot_bound(mag, int(k.max())) * scale).all() and grad.any(), kw
    xi = np.random.default_rng(7).integers(0, 3, (n, c)).astype(F)
    gi = AJ.small_integers((m, c), 8)
    y, grad = backward(pkg, rec, sp, xi, gi, points=pts, op="max")
    assert np.array_equal(grad.astype(np.float64), AJ.route(AJ.winners(pkg, rec, sp, xi, R, points=pts), gi, n))


def test_once_differentiable_state_check_and_arguments(pkg):
    rec, sp = scene(pkg)
    x = np.random.default_rng(1).normal(0.0, 1.0, (len(rec), 2)).astype(F)
    host = pkg.HostAggregateBackend(rec.copy(), sp)
    xt = torch.from_numpy(x).requires_grad_(True)
    y = pkg.aggregate_autograd(host, None, xt, R)
    w = torch.ones_like(y, requires_grad=True)
    (gx,) = torch.autograd.grad((y * w).sum(), xt, create_graph=True)
    with pytest.raises(RuntimeError, match="twice|once_differentiable"):
        gx.sum().backward()                                                             # once differentiable: a double backward raises
    # a changed state between forward and backward raises; check_state=False does not look
    xt = torch.from_numpy(x).requires_grad_(True)
    y = pkg.aggregate_autograd(host, None, xt, R)
    host.records["pos"][0, 0] += F(0.01)
    with pytest.raises(pkg.SphError, match="changed"):
        y.sum().backward()
    xt = torch.from_numpy(x).requires_grad_(True)
    y = pkg.aggregate_autograd(host, None, xt, R, check_state=False)
    host.records["pos"][0, 0] += F(0.01)
    y.sum().backward()
    assert xt.grad is not None
    # a tensor that does not require grad gets no graph
    assert not pkg.aggregate_autograd(host, None, torch.from_numpy(x), R).requires_grad
    for bad in (dict(op="median"), dict(weight="cubic"), dict(op="mean", moments=True)):
        with pytest.raises(pkg.SphError):
            pkg.aggregate_autograd(host, None, torch.from_numpy(x), R, **bad)
    with pytest.raises(pkg.SphError):
        pkg.aggregate_autograd(host, np.zeros((3, 3), F), torch.from_numpy(x), R, delta=True)
    with pytest.raises(pkg.SphError):
        pkg.aggregate_autograd(host, None, torch.from_numpy(x.astype(np.float64)), R)
