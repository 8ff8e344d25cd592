"""continuous_conv over HostAggregateBackend (autograd.py): the forward, x.grad and filters.grad against a dense
float64 torch reference built from pkg.neighbors_host's edge list (conv_ref.dense), with and without normalize, in one block of input
channels and in three; once differentiable; the state check; the arguments.  No GPU is needed.

The bounds.  u = 2^-24, gamma_m = m u / (1 - m u), elementwise and with every factor replaced by its absolute value.  T[i][b][k] are
the fp32 coefficients (the reference holds the very same numbers in float64), kf the most candidates of a row, ka the most rows that
accept a particle, g' = g, or g / W with normalize.  Any order of summation and any fusing inside a matrix product of m terms stays
within gamma_m of the magnitudes.
    out[i][o]   = sum_(b, c) A[i][b][c] F[b][c][o]: the basis accumulators gamma_kf, a product of B Cin terms, the sums of up to three
                  blocks: gamma_(kf + B Cin + 3); with normalize W (gamma_kf, its terms are positive) and the division: kf + 1 more.
    x.grad      = sum_(i, b) T[i][b][k] h[i][b][c], h = g' F^T a product of Cout terms, the adjoint's accumulator 8 ka terms:
                  gamma_(8 ka + Cout); with normalize g' carries kf + 1 more.
    filters.grad = sum_i A[i][b][c] g'[i][o]: gamma_(kf + rows); with normalize kf + 1 more.
Two spare units each cover the float64 reference and the 1 / (1 - m u) of the composition."""
import numpy as np
import pytest
import torch

from aggregate_ref import radius_of
import conv_ref as CR
from conv_ref import gamma
import query_scenes as QS

F = np.float32


def scene(pkg):
    return QS.uniform(pkg, 300, 31)


def reference(pkg, rec, sp, R, x, filt, g, points, weight, self_, normalize):
    """(out, x.grad, filters.grad, bounds of the three) from the dense float64 operator."""
    K, cin, cout = filt.shape[0], filt.shape[3], filt.shape[4]
    B = K ** 3
    kw = dict(points=points, size=K, weight=weight, self_=self_)
    T = torch.from_numpy(CR.dense(pkg, rec, sp, R, **kw))                               # (rows, B, n)
    rows_, recv, send, b, coef, w = CR.terms(pkg, rec, sp, R, **kw)
    rows = T.shape[0]
    W = torch.from_numpy(np.bincount(recv, weights=w.astype(np.float64), minlength=rows))
    kf, ka = int(np.bincount(recv, minlength=1).max()), int(np.bincount(send, minlength=1).max())
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    ft = torch.from_numpy(filt.astype(np.float64)).requires_grad_(True)
    out = torch.einsum("ibk,kc->ibc", T, xt).reshape(rows, B * cin) @ ft.reshape(B * cin, cout)
    scale = torch.where(W > 0, 1.0 / torch.where(W > 0, W, torch.ones_like(W)), torch.zeros_like(W)) if normalize else torch.ones_like(W)
    out = out * scale[:, None]
    gt = torch.from_numpy(g.astype(np.float64))
    (out * gt).sum().backward()
    # the magnitudes
    Ta, xa, fa = T.abs(), xt.detach().abs(), ft.detach().abs().reshape(B * cin, cout)
    ga = gt.abs() * scale[:, None]
    Aa = torch.einsum("ibk,kc->ibc", Ta, xa)
    extra = kf + 1 if normalize else 0
    b_out = gamma(kf + B * cin + 3 + extra + 2.0) * ((Aa.reshape(rows, -1) @ fa) * scale[:, None]).numpy()
    b_x = gamma(8 * ka + cout + extra + 2.0) * torch.einsum("ibk,ibc->kc", Ta, (ga @ fa.t()).reshape(rows, B, cin)).numpy()
    b_f = gamma(kf + rows + extra + 2.0) * (Aa.reshape(rows, -1).t() @ ga).reshape(K, K, K, cin, cout).numpy()
    return out.detach().numpy(), xt.grad.numpy(), ft.grad.numpy(), (b_out, b_x, b_f)


CASES = [(3, 6, 4, None, "poly6", True), (4, 5, 3, None, "one", False), (2, 7, 2, "points", "poly6", False), (3, 5, 4, "points", "one", False)]


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("K,cin,cout,target,weight,self_", CASES)
def test_gradients_against_the_dense_float64_reference(pkg, K, cin, cout, target, weight, self_, normalize):
    rec, sp = scene(pkg)
    n = len(rec)
    rng = np.random.default_rng(K + cin)
    points = None
    if target == "points":
        points = np.zeros((151, 4), F)
        points[:, :3] = QS.box_cloud(rng, sp, 151)
        points[17, 1] = np.nan                                                          # an empty row: out 0, no gradient through it
    rows = n if points is None else len(points)
    R = radius_of(sp, 2.0)
    x = rng.normal(0.0, 1.0, (n, cin)).astype(F)
    filt = rng.normal(0.0, 1.0, (K, K, K, cin, cout)).astype(F)
    g = rng.normal(0.0, 1.0, (rows, cout)).astype(F)
    want_out, want_x, want_f, (b_out, b_x, b_f) = reference(pkg, rec, sp, R, x, filt, g, points, weight, self_, normalize)
    host = pkg.HostAggregateBackend(rec, sp)
    one_block = 2 ** 31
    three_blocks = rows * K ** 3 * 4 * -(-cin // 3)                                     # a basis tensor of ceil(Cin / 3) channels: three blocks
    assert len(pkg.autograd._conv_blocks(rows, K ** 3, cin, three_blocks)) == 3 and len(pkg.autograd._conv_blocks(rows, K ** 3, cin, one_block)) == 1
    for limit in (one_block, three_blocks):
        xt, ft = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(filt).requires_grad_(True)
        y = pkg.continuous_conv(host, points, xt, ft, R, weight=weight, self_=self_, normalize=normalize, max_basis_bytes=limit)
        assert y.dtype == torch.float32 and tuple(y.shape) == (rows, cout)
        (y * torch.from_numpy(g)).sum().backward()
        ratios = []
        for got, want, bound, what in ((y.detach().numpy(), want_out, b_out, "out"), (xt.grad.numpy(), want_x, b_x, "x.grad"), (ft.grad.numpy(), want_f, b_f, "filters.grad")):
            err = np.abs(got.astype(np.float64) - want)
            ratios.append(float(np.max(err / np.maximum(bound, 1e-300))))
            assert (err <= bound).all() and np.abs(want).max() > 0, (what, limit, ratios)
        print(f"K {K} Cin {cin} Cout {cout} {target} {weight} normalize {normalize} blocks {1 if limit == one_block else 3}: largest error / bound "
              f"out {ratios[0]:.3g}, x.grad {ratios[1]:.3g}, filters.grad {ratios[2]:.3g}")
    if points is not None:
        assert not y.detach().numpy()[17].any()


def test_the_channel_blocks_change_no_basis_byte(pkg):
    """The basis sums of a block of channels are those columns of the whole tensor, byte for byte; so is the adjoint."""
    rec, sp = scene(pkg)
    x = np.random.default_rng(2).normal(0.0, 1.0, (len(rec), 7)).astype(F)
    R = radius_of(sp, 2.0)
    A = pkg.aggregate_basis_host(rec, sp, x, R, size=3, self_=True)
    h = CR.planes_for(len(rec), 3, 7)
    z = pkg.aggregate_basis_adjoint_host(rec, sp, h, R, size=3, self_=True)
    for c0, c1 in ((0, 3), (3, 6), (6, 7)):
        assert pkg.aggregate_basis_host(rec, sp, x[:, c0:c1].copy(), R, size=3, self_=True).tobytes() == A[:, :, c0:c1].tobytes()
        assert pkg.aggregate_basis_adjoint_host(rec, sp, h[:, :, c0:c1].copy(), R, size=3, self_=True).tobytes() == z[:, c0:c1].tobytes()


def test_once_differentiable_state_check_and_arguments(pkg):
    rec, sp = scene(pkg)
    R = radius_of(sp, 1.0)
    rng = np.random.default_rng(1)
    x, filt = rng.normal(0.0, 1.0, (len(rec), 2)).astype(F), rng.normal(0.0, 1.0, (2, 2, 2, 2, 3)).astype(F)
    host = pkg.HostAggregateBackend(rec.copy(), sp)
    xt, ft = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(filt).requires_grad_(True)
    y = pkg.continuous_conv(host, None, xt, ft, R)
    w = torch.ones_like(y, requires_grad=True)
    gx, gf = torch.autograd.grad((y * w).sum(), (xt, ft), create_graph=True)
    with pytest.raises(RuntimeError, match="twice|once_differentiable"):
        (gx.sum() + gf.sum()).backward()                                                # once differentiable: a double backward raises
    # a changed state between forward and backward raises; check_state=False does not look
    xt = torch.from_numpy(x).requires_grad_(True)
    y = pkg.continuous_conv(host, None, xt, torch.from_numpy(filt), R)
    host.records["pos"][0, 0] += F(0.01)
    with pytest.raises(pkg.SphError, match="changed"):
        y.sum().backward()
    xt = torch.from_numpy(x).requires_grad_(True)
    y = pkg.continuous_conv(host, None, xt, torch.from_numpy(filt), R, check_state=False)
    host.records["pos"][0, 0] += F(0.01)
    y.sum().backward()
    assert xt.grad is not None
    # only what requires grad gets one; nothing that requires grad: no graph
    xt, ft = torch.from_numpy(x), torch.from_numpy(filt).requires_grad_(True)
    pkg.continuous_conv(host, None, xt, ft, R).sum().backward()
    assert xt.grad is None and ft.grad is not None
    assert not pkg.continuous_conv(host, None, torch.from_numpy(x), torch.from_numpy(filt), R).requires_grad
    good = (torch.from_numpy(x), torch.from_numpy(filt))
    for bad_x, bad_f, kw in ((good[0].double(), good[1], {}), (good[0], good[1].double(), {}), (good[0][:, 0], good[1], {}), (good[0], good[1][0], {}),
                             (good[0], torch.zeros((2, 2, 3, 2, 3)), {}), (good[0], torch.zeros((5, 5, 5, 2, 3)), {}), (good[0], torch.zeros((2, 2, 2, 3, 3)), {}),
                             (good[0], good[1], dict(weight="cubic"))):
        with pytest.raises(pkg.SphError):
            pkg.continuous_conv(host, None, bad_x, bad_f, R, **kw)
    with pytest.raises(pkg.SphError):
        pkg.continuous_conv(host, np.zeros((3, 4), F), good[0], good[1], R, self_=True)   # SELF applies to particle targets only
