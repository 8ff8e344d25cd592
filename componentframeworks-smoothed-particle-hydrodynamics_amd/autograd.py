"""Autograd through the fused neighbourhood reductions: torch.autograd.Functions whose backward is the engine's
own adjoint, so that a loss over aggregate() needs no edge list.

Differentiable in `values` only: the positions are the engine's state, not a tensor.  Once differentiable.  The backward formulas are
written against a small backend (forward, adjoint, arg, route) that the engine implements on the device (EngineAggregateBackend) and
the host twins implement on the CPU (HostAggregateBackend), so that they can be checked without a GPU:

  sum        grad = adjoint(g)
  mean       grad = adjoint(g / W), 0 where W == 0; W is the counts output for weight "one" and a one-channel SUM of ones otherwise
             (acc = acc + w * 1 in the forward's order: MEAN's own W bits)
  max / min  grad = route(arg, g); with delta additionally -g[i][c] goes to row i wherever arg[i][c] >= 0
"""
from __future__ import annotations

import zlib

import numpy as np

from .engine import (SphError, aggregate_adjoint_host, aggregate_arg_host, aggregate_host, aggregate_route_host)

__all__ = ["EngineAggregateBackend", "HostAggregateBackend", "aggregate_autograd"]


class EngineAggregateBackend:
    """The four calls on an SPHFluidGPU: torch device tensors in and out.  points: None, or (m, 3) / (m, 4) query points."""

    def __init__(self, engine):
        self.f = engine

    def state(self):
        return self.f.state_digest(["particles"])

    def forward(self, points, values, radius, op, weight, self_, fluid_only, delta, moments, counts):
        if points is None:
            return self.f.aggregate(values, radius, op=op, weight=weight, self_=self_, fluid_only=fluid_only, delta=delta, moments=moments,
                                    counts=counts, device=True)
        return self.f.query_aggregate(points, values, radius, op=op, weight=weight, fluid_only=fluid_only, moments=moments, counts=counts, device=True)

    def adjoint(self, points, grad, radius, weight, self_, fluid_only, delta, moments):
        if points is None:
            return self.f.aggregate_adjoint(grad, radius, weight=weight, self_=self_, fluid_only=fluid_only, delta=delta, moments=moments, device=True)
        return self.f.query_aggregate_adjoint(points, grad, radius, weight=weight, fluid_only=fluid_only, moments=moments, device=True)

    def arg(self, points, values, radius, op, self_, fluid_only, delta):
        if points is None:
            return self.f.aggregate_arg(values, radius, op=op, self_=self_, fluid_only=fluid_only, delta=delta, device=True)
        return self.f.query_aggregate_arg(points, values, radius, op=op, fluid_only=fluid_only, device=True)

    def route(self, points, arg, grad, radius, op, self_, fluid_only, delta):
        if points is None:
            return self.f.aggregate_route(arg, grad, radius, op=op, self_=self_, fluid_only=fluid_only, delta=delta, device=True)
        return self.f.query_aggregate_route(points, arg, grad, radius, op=op, fluid_only=fluid_only, device=True)


class HostAggregateBackend:
    """The same four calls over the host twins on (records, params): CPU torch tensors in and out, the bytes the device gives.  No GPU."""

    def __init__(self, records, params):
        self.records, self.params = records, params

    def state(self):
        return zlib.crc32(np.ascontiguousarray(self.records).tobytes())

    @staticmethod
    def _np(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    @staticmethod
    def _t(a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a))

    def forward(self, points, values, radius, op, weight, self_, fluid_only, delta, moments, counts):
        res = aggregate_host(self.records, self.params, self._np(values), radius, points=points, op=op, weight=weight, self_=self_, fluid_only=fluid_only,
                             delta=delta, moments=moments, counts=counts)
        return (self._t(res[0]), self._t(res[1])) if counts else self._t(res)

    def adjoint(self, points, grad, radius, weight, self_, fluid_only, delta, moments):
        return self._t(aggregate_adjoint_host(self.records, self.params, self._np(grad), radius, points=points, weight=weight, self_=self_,
                                              fluid_only=fluid_only, delta=delta, moments=moments))

    def arg(self, points, values, radius, op, self_, fluid_only, delta):
        out, arg = aggregate_arg_host(self.records, self.params, self._np(values), radius, points=points, op=op, self_=self_, fluid_only=fluid_only, delta=delta)
        return self._t(out), self._t(arg)

    def route(self, points, arg, grad, radius, op, self_, fluid_only, delta):
        return self._t(aggregate_route_host(self.records, self.params, self._np(arg), self._np(grad), radius, points=points, op=op, self_=self_,
                                            fluid_only=fluid_only, delta=delta))


def _function():
    """The torch.autograd.Function, made on first use so that importing the package does not import torch."""
    global _FN
    if _FN is not None:
        return _FN
    import torch
    from torch.autograd.function import once_differentiable

    class AggregateFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, values, backend, points, radius, op, weight, self_, fluid_only, delta, moments, check_state):
            ctx.backend, ctx.points, ctx.radius = backend, points, radius
            ctx.cfg = (op, weight, self_, fluid_only, delta, moments)
            ctx.digest = backend.state() if check_state else None
            ctx.check_state = check_state
            v = values.detach()
            if op in ("max", "min"):
                out, arg = backend.arg(points, v, radius, op, self_, fluid_only, delta)
                ctx.save_for_backward(arg)
            elif op == "mean":
                if weight == "one":
                    out, cnt = backend.forward(points, v, radius, op, weight, self_, fluid_only, delta, False, True)
                    W = cnt.to(torch.float32)
                else:
                    out = backend.forward(points, v, radius, op, weight, self_, fluid_only, delta, False, False)
                    ones = torch.ones((v.shape[0], 1), dtype=torch.float32, device=v.device)
                    W = backend.forward(points, ones, radius, "sum", weight, self_, fluid_only, False, False, False).reshape(-1)
                ctx.save_for_backward(W)
            else:
                out = backend.forward(points, v, radius, op, weight, self_, fluid_only, delta, moments, False)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            op, weight, self_, fluid_only, delta, moments = ctx.cfg
            backend, points, radius = ctx.backend, ctx.points, ctx.radius
            if ctx.check_state and backend.state() != ctx.digest:
                raise SphError("aggregate_autograd: the particle state changed between forward and backward (a dispatch, an upload or an impulse): "
                               "the adjoint would be that of another neighbour relation")
            g = g.contiguous()
            if op in ("max", "min"):
                (arg,) = ctx.saved_tensors
                grad = backend.route(points, arg, g, radius, op, self_, fluid_only, delta)
                if delta:
                    grad = grad - torch.where(arg >= 0, g, torch.zeros_like(g))
            elif op == "mean":
                (W,) = ctx.saved_tensors
                ok = (W != 0)[:, None]
                gW = torch.where(ok, g / torch.where(ok, W[:, None], torch.ones_like(W[:, None])), torch.zeros_like(g))
                grad = backend.adjoint(points, gW.contiguous(), radius, weight, self_, fluid_only, delta, False)
            else:
                grad = backend.adjoint(points, g, radius, weight, self_, fluid_only, delta, moments)
            return (grad,) + (None,) * 10

    _FN = AggregateFunction
    return _FN


_FN = None


def aggregate_autograd(backend, points, values, radius, op="sum", weight="one", self_=False, fluid_only=False, delta=False, moments=False,
                       check_state=True):
    """aggregate() (points None) or query_aggregate() of `backend` as a differentiable function of `values`, a float32 torch tensor of
    (n, C) on the backend's device.  The forward output has the bytes of aggregate(..., device=True).  Differentiable in values only, and
    once differentiable: a double backward raises.  check_state: the forward stores the backend's digest of the particle state and the
    backward raises SphError if it has changed; False skips both reads."""
    import torch
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 2:
        raise SphError("aggregate_autograd: values must be a float32 torch tensor of shape (n, C)")
    if op not in ("sum", "mean", "max", "min") or weight not in ("one", "poly6"):
        raise SphError(f"aggregate_autograd: op {op!r}, weight {weight!r}")
    if moments and op != "sum":
        raise SphError("aggregate_autograd: moments go with op 'sum' only")
    if points is not None and (self_ or delta):
        raise SphError("aggregate_autograd: self_ and delta apply to particle targets only")
    return _function().apply(values, backend, points, float(radius), op, weight, bool(self_), bool(fluid_only), bool(delta), bool(moments), bool(check_state))
