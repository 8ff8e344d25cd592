"""Autograd through the fused neighbourhood reductions: torch.autograd.Functions whose backward is the engine's
own adjoint, so that a loss over aggregate() needs no edge list.

Differentiable in `values`, and with the keyword `positions` (and `points_grad` for query points) in the positions too (DESIGN.md
section 3x), continuous_conv included.  Once differentiable.  The backward formulas are written
against a small backend (forward, adjoint, arg, route, posgrad) that the engine implements on the device (EngineAggregateBackend) and
the host twins implement on the CPU (HostAggregateBackend), so that they can be checked without a GPU:

  sum        grad = adjoint(g)
  mean       grad = adjoint(g / W), 0 where W == 0; W is the counts output for weight "one" and a one-channel SUM of ones otherwise
             (acc = acc + w * 1 in the forward's order: MEAN's own W bits)
  max / min  grad = route(arg, g); with delta additionally -g[i][c] goes to row i wherever arg[i][c] >= 0

and the gradient of the positions (posgrad returns the pair (points' rows or None, particles' rows); the cutoff is not differentiated):

  sum        posgrad(values, g)
  mean       with g' = g / W (0 where W == 0): posgrad(values, g'), and for weight "poly6" plus the gradient through W, a one-channel
             posgrad of ones with the upstream -sum_c g'[i][c] * out[i][c] (for weight "one" W is a count: that term is zero)
  max / min  zeros (weight "one": piecewise constant); no engine call

continuous_conv stands on two more backend calls, basis and basis_adjoint.  With A the basis sums of a block of
input channels, (rows, B, cw), and F the block's filters as a (B * cw, Cout) matrix:

  forward    out = sum over the blocks of A.reshape(rows, B * cw) @ F;  with normalize out / W, 0 where W == 0 (MEAN's own W, as above)
  backward   g' = g (g / W with normalize);  grad_filters = A^T @ g' per block, A recomputed rather than saved;
             grad_x = basis_adjoint((g' @ F^T).reshape(rows, B, cw)) per block
The basis tensors and the adjoint have fixed bytes; the two matrix products are torch's, and no byte claim is made for them.

With positions= (and points_grad= for query points) a second Function with the same forward calls adds, through the backend call
basis_posgrad (the pair (points' rows or None, particles' rows), as posgrad):

  positions  sum over the blocks of basis_posgrad(x[:, c0:c1], h_block), h_block the (g' @ F_block^T) tensor of grad_x;
             with normalize and weight "poly6" plus the gradient through W: the one-channel posgrad of ones with the upstream
             -sum_o g'[i][o] * out[i][o] (for weight "one" W is a count: that term is zero)
With one block and no normalize the gradient is basis_posgrad's bytes; otherwise the parts are added by torch in block order.
"""
from __future__ import annotations

import zlib

import numpy as np

from .engine import (SPH_AGGREGATE_MAX_CHANNELS, SphError, aggregate_adjoint_host, aggregate_arg_host, aggregate_basis_adjoint_host, aggregate_basis_host,
                     aggregate_basis_position_grad_host, aggregate_host, aggregate_position_grad_host, aggregate_route_host)

__all__ = ["EngineAggregateBackend", "HostAggregateBackend", "aggregate_autograd", "continuous_conv"]


class EngineAggregateBackend:
    """The backend calls on an SPHFluidGPU: torch device tensors in and out.  points: None, or (m, 3) / (m, 4) query points."""

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

    def positions(self):
        return self.f.positions(device=True)

    def posgrad(self, points, values, grad, radius, weight, self_, fluid_only, delta, moments, want_points=True, want_particles=True):
        if points is None:
            return None, self.f.aggregate_position_grad(values, grad, radius, weight=weight, self_=self_, fluid_only=fluid_only, delta=delta, moments=moments,
                                                        device=True)
        return self.f.query_aggregate_position_grad(points, values, grad, radius, weight=weight, fluid_only=fluid_only, moments=moments, device=True,
                                                    want_points=want_points, want_particles=want_particles)

    def basis(self, points, x, radius, size, weight, self_, fluid_only):
        if points is None:
            return self.f.aggregate_basis(x, radius, size=size, weight=weight, self_=self_, fluid_only=fluid_only, device=True)
        return self.f.query_aggregate_basis(points, x, radius, size=size, weight=weight, fluid_only=fluid_only, device=True)

    def basis_adjoint(self, points, h, radius, size, weight, self_, fluid_only):
        if points is None:
            return self.f.aggregate_basis_adjoint(h, radius, size=size, weight=weight, self_=self_, fluid_only=fluid_only, device=True)
        return self.f.query_aggregate_basis_adjoint(points, h, radius, size=size, weight=weight, fluid_only=fluid_only, device=True)

    def basis_posgrad(self, points, x, grad, radius, size, weight, self_, fluid_only, want_points=True, want_particles=True):
        if points is None:
            return None, self.f.aggregate_basis_position_grad(x, grad, radius, size=size, weight=weight, self_=self_, fluid_only=fluid_only, device=True)
        return self.f.query_aggregate_basis_position_grad(points, x, grad, radius, size=size, weight=weight, fluid_only=fluid_only, device=True,
                                                          want_points=want_points, want_particles=want_particles)


class HostAggregateBackend:
    """The same calls over the host twins on (records, params): CPU torch tensors in and out, the bytes the device gives.  No GPU."""

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

    def positions(self):
        return self._t(np.ascontiguousarray(self.records["pos"][:, :3], np.float32))

    def posgrad(self, points, values, grad, radius, weight, self_, fluid_only, delta, moments, want_points=True, want_particles=True):
        res = aggregate_position_grad_host(self.records, self.params, self._np(values), self._np(grad), radius, points=None if points is None else self._np(points),
                                           weight=weight, self_=self_, fluid_only=fluid_only, delta=delta, moments=moments)
        if points is None:
            return None, self._t(res)
        return (self._t(res[0]) if want_points else None), (self._t(res[1]) if want_particles else None)

    def basis(self, points, x, radius, size, weight, self_, fluid_only):
        return self._t(aggregate_basis_host(self.records, self.params, self._np(x), radius, points=points, size=size, weight=weight, self_=self_,
                                            fluid_only=fluid_only))

    def basis_adjoint(self, points, h, radius, size, weight, self_, fluid_only):
        return self._t(aggregate_basis_adjoint_host(self.records, self.params, self._np(h), radius, points=points, size=size, weight=weight, self_=self_,
                                                    fluid_only=fluid_only))

    def basis_posgrad(self, points, x, grad, radius, size, weight, self_, fluid_only, want_points=True, want_particles=True):
        res = aggregate_basis_position_grad_host(self.records, self.params, self._np(x), self._np(grad), radius, points=None if points is None else self._np(points),
                                                 size=size, weight=weight, self_=self_, fluid_only=fluid_only, want_points=want_points,
                                                 want_particles=want_particles)
        if points is None:
            return None, self._t(res)
        return (None if res[0] is None else self._t(res[0])), (None if res[1] is None else self._t(res[1]))


def _function():
    """The two torch.autograd.Functions (values only; values and positions), made on first use so that importing the package does not
    import torch."""
    global _FN
    if _FN is not None:
        return _FN
    import torch
    from torch.autograd.function import once_differentiable

    def values_forward(ctx, values, backend, points, radius, op, weight, self_, fluid_only, delta, moments, check_state):
        """The forward of both Functions: (out, the tensors the values' backward needs)."""
        ctx.backend, ctx.points, ctx.radius = backend, points, radius
        ctx.cfg = (op, weight, self_, fluid_only, delta, moments)
        ctx.digest = backend.state() if check_state else None
        ctx.check_state = check_state
        v = values.detach()
        saved = ()
        if op in ("max", "min"):
            out, arg = backend.arg(points, v, radius, op, self_, fluid_only, delta)
            saved = (arg,)
        elif op == "mean":
            if weight == "one":
                out, cnt = backend.forward(points, v, radius, op, weight, self_, fluid_only, delta, False, True)
                W = cnt.to(torch.float32)
            else:
                out = backend.forward(points, v, radius, op, weight, self_, fluid_only, delta, False, False)
                ones = torch.ones((v.shape[0], 1), dtype=torch.float32, device=v.device)
                W = backend.forward(points, ones, radius, "sum", weight, self_, fluid_only, False, False, False).reshape(-1)
            saved = (W,)
        else:
            out = backend.forward(points, v, radius, op, weight, self_, fluid_only, delta, moments, False)
        return out, saved

    def check(ctx):
        if ctx.check_state and ctx.backend.state() != ctx.digest:
            raise SphError("aggregate_autograd: the particle state changed between forward and backward (a dispatch, an upload or an impulse): "
                           "the adjoint would be that of another neighbour relation")

    def mean_upstream(g, W):
        ok = (W != 0)[:, None]
        return torch.where(ok, g / torch.where(ok, W[:, None], torch.ones_like(W[:, None])), torch.zeros_like(g))

    def values_backward(ctx, g, saved):
        op, weight, self_, fluid_only, delta, moments = ctx.cfg
        backend, points, radius = ctx.backend, ctx.points, ctx.radius
        if op in ("max", "min"):
            (arg,) = saved
            grad = backend.route(points, arg, g, radius, op, self_, fluid_only, delta)
            if delta:
                grad = grad - torch.where(arg >= 0, g, torch.zeros_like(g))
        elif op == "mean":
            (W,) = saved
            grad = backend.adjoint(points, mean_upstream(g, W).contiguous(), radius, weight, self_, fluid_only, delta, False)
        else:
            grad = backend.adjoint(points, g, radius, weight, self_, fluid_only, delta, moments)
        return grad

    def positions_backward(ctx, g, saved, v, out, want_points, want_particles):
        """(the points' rows or None, the particles' rows or None) of the position gradient (module docstring)."""
        op, weight, self_, fluid_only, delta, moments = ctx.cfg
        backend, points, radius = ctx.backend, ctx.points, ctx.radius
        rows = int(out.shape[0])
        if op in ("max", "min"):
            return (torch.zeros((rows, 3), dtype=torch.float32, device=v.device) if want_points else None,
                    torch.zeros((int(v.shape[0]), 3), dtype=torch.float32, device=v.device) if want_particles else None)
        if op == "sum":
            return backend.posgrad(points, v, g, radius, weight, self_, fluid_only, delta, moments, want_points, want_particles)
        (W,) = saved
        gW = mean_upstream(g, W).contiguous()
        pts, par = backend.posgrad(points, v, gW, radius, weight, self_, fluid_only, delta, False, want_points, want_particles)
        if weight != "one":                                                         # the gradient through W = sum w * 1
            up = (-(gW * out).sum(dim=1, keepdim=True)).contiguous()
            ones = torch.ones((int(v.shape[0]), 1), dtype=torch.float32, device=v.device)
            pts2, par2 = backend.posgrad(points, ones, up, radius, weight, self_, fluid_only, False, False, want_points, want_particles)
            pts = None if pts is None else pts + pts2
            par = None if par is None else par + par2
        return pts, par

    class AggregateFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, values, backend, points, radius, op, weight, self_, fluid_only, delta, moments, check_state):
            out, saved = values_forward(ctx, values, backend, points, radius, op, weight, self_, fluid_only, delta, moments, check_state)
            if saved:
                ctx.save_for_backward(*saved)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            check(ctx)
            return (values_backward(ctx, g.contiguous(), ctx.saved_tensors),) + (None,) * 10

    class AggregatePositionFunction(torch.autograd.Function):
        """The same forward with two more tensor inputs: positions (n, 3), which must hold the backend's positions, and the query points
        as a tensor (or None).  The backward adds the position gradient."""

        @staticmethod
        def forward(ctx, values, positions, points_leaf, backend, points, radius, op, weight, self_, fluid_only, delta, moments, check_state):
            if positions is not None and check_state:
                mine = backend.positions()
                theirs = positions.detach().contiguous()
                if tuple(theirs.shape) != tuple(mine.shape) or not torch.equal(theirs.view(torch.int32), mine.view(torch.int32)):
                    raise SphError("aggregate_autograd: positions does not hold the engine's positions byte for byte: the gradient would be that of "
                                   "another configuration")
            out, saved = values_forward(ctx, values, backend, points, radius, op, weight, self_, fluid_only, delta, moments, check_state)
            ctx.nsaved = len(saved)
            ctx.leaf_width = 0 if points_leaf is None else int(points_leaf.shape[1])
            ctx.save_for_backward(*saved, values.detach(), out)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            check(ctx)
            g = g.contiguous()
            saved, (v, out) = ctx.saved_tensors[:ctx.nsaved], ctx.saved_tensors[ctx.nsaved:]
            need_v, need_x, need_p = ctx.needs_input_grad[:3]
            grad_v = values_backward(ctx, g, saved) if need_v else None
            grad_x = grad_p = None
            if need_x or need_p:
                grad_p, grad_x = positions_backward(ctx, g, saved, v, out, need_p, need_x or ctx.points is None)
                if not need_x:
                    grad_x = None
                if need_p and ctx.leaf_width == 4:
                    grad_p = torch.cat([grad_p, torch.zeros_like(grad_p[:, :1])], dim=1)
            return (grad_v, grad_x, grad_p) + (None,) * 10

    _FN = (AggregateFunction, AggregatePositionFunction)
    return _FN


_FN = None


def aggregate_autograd(backend, points, values, radius, op="sum", weight="one", self_=False, fluid_only=False, delta=False, moments=False,
                       check_state=True, positions=None, points_grad=False, points_leaf=None):
    """aggregate() (points None) or query_aggregate() of `backend` as a differentiable function of `values`, a float32 torch tensor of
    (n, C) on the backend's device.  The forward output has the bytes of aggregate(..., device=True).  Once differentiable: a double
    backward raises.  check_state: the forward stores the backend's digest of the particle state and the backward raises SphError if it
    has changed; False skips both reads.
    positions: None (differentiable in values only: the same Function, calls and bytes as without the keyword), or an (n, 3) float32
    tensor on the backend's device that holds the backend's positions (backend.positions()); it takes part in the graph and receives
    dL/dx (module docstring).  With check_state the forward verifies that it holds the backend's positions byte for byte and raises
    SphError otherwise.  points_grad (query targets): `points` must be a float32 torch tensor of (m, 3) or (m, 4) and receives the points'
    gradient (a fourth column gets zeros); without it a points tensor that requires grad still gets None.  points_leaf: the tensor
    that receives it where `points` is a copy in the backend's layout (SPHFluidGPU.query_aggregate_autograd passes both)."""
    import torch
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 2:
        raise SphError("aggregate_autograd: values must be a float32 torch tensor of shape (n, C)")
    if op not in ("sum", "mean", "max", "min") or weight not in ("one", "poly6"):
        raise SphError(f"aggregate_autograd: op {op!r}, weight {weight!r}")
    if moments and op != "sum":
        raise SphError("aggregate_autograd: moments go with op 'sum' only")
    if points is not None and (self_ or delta):
        raise SphError("aggregate_autograd: self_ and delta apply to particle targets only")
    args = (float(radius), op, weight, bool(self_), bool(fluid_only), bool(delta), bool(moments), bool(check_state))
    if positions is None and not points_grad:
        return _function()[0].apply(values, backend, points, *args)
    if positions is not None and (not isinstance(positions, torch.Tensor) or positions.dtype != torch.float32 or tuple(positions.shape) != (int(values.shape[0]), 3)
                                  or positions.device != values.device):
        raise SphError("aggregate_autograd: positions must be a float32 torch tensor of shape (n, 3) on the device of values")
    leaf = None
    if points_grad:
        points_leaf = points if points_leaf is None else points_leaf
        if points is None or not isinstance(points_leaf, torch.Tensor) or points_leaf.dtype != torch.float32 or points_leaf.dim() != 2 or int(points_leaf.shape[1]) not in (3, 4):
            raise SphError("aggregate_autograd: points_grad takes the query points as a float32 torch tensor of shape (m, 3) or (m, 4)")
        leaf = points_leaf
    plain = points.detach() if isinstance(points, torch.Tensor) else points
    return _function()[1].apply(values, positions, leaf, backend, plain, *args)


def _conv_blocks(rows, planes, cin, max_basis_bytes):
    """The blocks [c0, c1) of input channels: the widest of at most SPH_AGGREGATE_MAX_CHANNELS channels whose basis tensor of
    rows * planes * width floats stays under max_basis_bytes (one channel where even that does not)."""
    width = max(1, min(cin, SPH_AGGREGATE_MAX_CHANNELS, int(max_basis_bytes) // max(1, rows * planes * 4)))
    return [(c0, min(cin, c0 + width)) for c0 in range(0, cin, width)]


def _conv_function():
    """continuous_conv's torch.autograd.Function, made on first use as _function()."""
    global _CONV
    if _CONV is not None:
        return _CONV
    import torch
    from torch.autograd.function import once_differentiable

    def weight_sum(backend, points, n, like, radius, weight, self_, fluid_only):
        ones = torch.ones((n, 1), dtype=torch.float32, device=like.device)
        return backend.forward(points, ones, radius, "sum", weight, self_, fluid_only, False, False, False).reshape(-1)

    def divide(t, W):
        ok = (W != 0)[:, None]
        return torch.where(ok, t / torch.where(ok, W[:, None], torch.ones_like(W[:, None])), torch.zeros_like(t))

    def conv_forward(ctx, x, filters, backend, points, radius, weight, self_, fluid_only, normalize, check_state, blocks):
        """The forward of both Functions: (out, the tensors the backward of x and the filters needs)."""
        ctx.backend, ctx.points, ctx.radius, ctx.blocks = backend, points, radius, blocks
        ctx.cfg = (weight, self_, fluid_only, normalize)
        ctx.digest = backend.state() if check_state else None
        ctx.check_state = check_state
        xd, fd = x.detach(), filters.detach()
        K, cout = int(fd.shape[0]), int(fd.shape[4])
        out = None
        for c0, c1 in blocks:
            A = backend.basis(points, xd[:, c0:c1].contiguous(), radius, K, weight, self_, fluid_only)
            part = A.reshape(A.shape[0], -1) @ fd[:, :, :, c0:c1, :].reshape(-1, cout)
            out = part if out is None else out + part
        W = weight_sum(backend, points, xd.shape[0], xd, radius, weight, self_, fluid_only) if normalize else xd.new_zeros(0)
        return (divide(out, W) if normalize else out), (xd, fd, W)

    class ContinuousConvFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, filters, backend, points, radius, weight, self_, fluid_only, normalize, check_state, blocks):
            out, saved = conv_forward(ctx, x, filters, backend, points, radius, weight, self_, fluid_only, normalize, check_state, blocks)
            ctx.save_for_backward(*saved)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            return conv_backward(ctx, g, ctx.saved_tensors, False, False)[:2] + (None,) * 9

    def conv_backward(ctx, g, saved, need_pos, need_pts):
        """(grad_x, grad_filters, the points' rows or None, the particles' rows or None); the last two are asked for by need_pts / need_pos."""
        weight, self_, fluid_only, normalize = ctx.cfg
        backend, points, radius = ctx.backend, ctx.points, ctx.radius
        if ctx.check_state and backend.state() != ctx.digest:
            raise SphError("continuous_conv: the particle state changed between forward and backward (a dispatch, an upload or an impulse): "
                           "the adjoint would be that of another neighbour relation")
        x, filters, W = saved[:3]
        K, cout = int(filters.shape[0]), int(filters.shape[4])
        g = divide(g, W) if normalize else g
        g = g.contiguous()
        need_x, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        grad_x = torch.zeros_like(x) if need_x else None
        grad_f = torch.zeros_like(filters) if need_f else None
        grad_pts = grad_par = None
        geometry = need_pos or need_pts
        for c0, c1 in ctx.blocks:
            fblock = filters[:, :, :, c0:c1, :].reshape(-1, cout)
            if need_f:
                A = backend.basis(points, x[:, c0:c1].contiguous(), radius, K, weight, self_, fluid_only)
                grad_f[:, :, :, c0:c1, :] = (A.reshape(A.shape[0], -1).t() @ g).reshape(K, K, K, c1 - c0, cout)
            if need_x or geometry:
                h = (g @ fblock.t()).reshape(g.shape[0], K ** 3, c1 - c0).contiguous()
            if need_x:
                grad_x[:, c0:c1] = backend.basis_adjoint(points, h, radius, K, weight, self_, fluid_only)
            if geometry:
                pts, par = backend.basis_posgrad(points, x[:, c0:c1].contiguous(), h, radius, K, weight, self_, fluid_only, need_pts,
                                                 need_pos or points is None)
                grad_pts = pts if grad_pts is None or pts is None else grad_pts + pts
                grad_par = par if grad_par is None or par is None else grad_par + par
        if geometry and normalize and weight != "one":                              # the gradient through W = sum w * 1
            out = saved[3]
            up = (-(g * out).sum(dim=1, keepdim=True)).contiguous()
            ones = torch.ones((int(x.shape[0]), 1), dtype=torch.float32, device=x.device)
            pts, par = backend.posgrad(points, ones, up, radius, weight, self_, fluid_only, False, False, need_pts, need_pos or points is None)
            grad_pts = None if grad_pts is None else grad_pts + pts
            grad_par = None if grad_par is None else grad_par + par
        return grad_x, grad_f, grad_pts, (grad_par if need_pos else None)

    class ContinuousConvPositionFunction(torch.autograd.Function):
        """The same forward with two more tensor inputs: positions (n, 3), which must hold the backend's positions, and the query points
        as a tensor (or None).  The backward adds the position gradient."""

        @staticmethod
        def forward(ctx, x, filters, positions, points_leaf, backend, points, radius, weight, self_, fluid_only, normalize, check_state, blocks):
            if positions is not None and check_state:
                mine = backend.positions()
                theirs = positions.detach().contiguous()
                if tuple(theirs.shape) != tuple(mine.shape) or not torch.equal(theirs.view(torch.int32), mine.view(torch.int32)):
                    raise SphError("continuous_conv: positions does not hold the engine's positions byte for byte: the gradient would be that of another "
                                   "configuration")
            out, saved = conv_forward(ctx, x, filters, backend, points, radius, weight, self_, fluid_only, normalize, check_state, blocks)
            ctx.leaf_width = 0 if points_leaf is None else int(points_leaf.shape[1])
            ctx.save_for_backward(*saved, *((out,) if normalize else ()))           # (out enters the gradient through W)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            need_pos, need_pts = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
            grad_x, grad_f, grad_pts, grad_par = conv_backward(ctx, g, ctx.saved_tensors, need_pos, need_pts)
            if need_pts and ctx.leaf_width == 4:
                grad_pts = torch.cat([grad_pts, torch.zeros_like(grad_pts[:, :1])], dim=1)
            return (grad_x, grad_f, grad_par, grad_pts) + (None,) * 9

    _CONV = (ContinuousConvFunction, ContinuousConvPositionFunction)
    return _CONV


_CONV = None


def continuous_conv(backend, points, x, filters, radius, weight="poly6", self_=True, fluid_only=False, normalize=False, check_state=True,
                    max_basis_bytes=2 ** 31, positions=None, points_grad=False, points_leaf=None):
    """The continuous convolution of `backend` (points None: particle targets) as a differentiable function of x, float32 (n, Cin), and
    filters, float32 (K, K, K, Cin, Cout) with axes (z, y, x) and K in 2 .. 4, both on the backend's device: (rows, Cout).  Once
    differentiable in both.  positions, points_grad, points_leaf as aggregate_autograd(): with them the positions (and the query points)
    take part in the graph; with both at their defaults the Function, the backend calls and the bytes are those of a call without
    them.  The module docstring has the formulas; SPHFluidGPU.continuous_conv the arguments."""
    import torch
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise SphError("continuous_conv: x must be a float32 torch tensor of shape (n, Cin)")
    if not isinstance(filters, torch.Tensor) or filters.dtype != torch.float32 or filters.dim() != 5 or filters.device != x.device:
        raise SphError("continuous_conv: filters must be a float32 torch tensor of shape (K, K, K, Cin, Cout) on the device of x")
    K, cin, cout = int(filters.shape[0]), int(filters.shape[3]), int(filters.shape[4])
    if tuple(filters.shape[:3]) != (K, K, K) or K < 2 or K > 4 or cin != int(x.shape[1]) or cin < 1 or cout < 1:
        raise SphError(f"continuous_conv: filters of shape {tuple(filters.shape)} for x of shape {tuple(x.shape)} (K, K, K, Cin, Cout with K in 2 .. 4)")
    if weight not in ("one", "poly6"):
        raise SphError(f"continuous_conv: weight {weight!r}")
    if points is not None and self_:
        raise SphError("continuous_conv: self_ applies to particle targets only")
    rows = int(x.shape[0]) if points is None else int(points.shape[0])
    blocks = _conv_blocks(rows, K ** 3, cin, max_basis_bytes)
    args = (float(radius), weight, bool(self_), bool(fluid_only), bool(normalize), bool(check_state), blocks)
    if positions is None and not points_grad:
        return _conv_function()[0].apply(x, filters, backend, points, *args)
    if positions is not None and (not isinstance(positions, torch.Tensor) or positions.dtype != torch.float32 or tuple(positions.shape) != (int(x.shape[0]), 3)
                                  or positions.device != x.device):
        raise SphError("continuous_conv: positions must be a float32 torch tensor of shape (n, 3) on the device of x")
    leaf = None
    if points_grad:
        points_leaf = points if points_leaf is None else points_leaf
        if points is None or not isinstance(points_leaf, torch.Tensor) or points_leaf.dtype != torch.float32 or points_leaf.dim() != 2 or int(points_leaf.shape[1]) not in (3, 4):
            raise SphError("continuous_conv: points_grad takes the query points as a float32 torch tensor of shape (m, 3) or (m, 4)")
        leaf = points_leaf
    plain = points.detach() if isinstance(points, torch.Tensor) else points
    return _conv_function()[1].apply(x, filters, positions, leaf, backend, plain, *args)
