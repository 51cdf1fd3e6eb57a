"""The float64 numpy oracle on rectangular maps (H != W), before any kernel is compared with it:
oracle.numpy_oracle.conv2d_fwd / conv2d_bwd, maxpool2_fwd / maxpool2_bwd and bn_train_fwd /
bn_train_bwd over axes (2, 3) against torch.nn.functional.conv2d / max_pool2d / batch_norm in
float64 with autograd.  Every tensor within 1e-12 max-abs (float64 sums of a few thousand O(1)
terms in another order; measured <= 1.5e-13).  The inputs carry a term monotone in h and a
different one in w, and the second BN group is 10x the first, so an oracle that swapped two axes
or two groups would not pass either."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
F = torch.nn.functional

from oracle import numpy_oracle as O  # noqa: E402

BOUND = 1e-12

CONV_SHAPES = [  # N, Cin, H, W, Cout, K, pad
    (2, 8, 12, 20, 16, 5, 2), (2, 1, 20, 8, 32, 3, 1), (3, 32, 14, 10, 64, 5, 0)]
POOL_SHAPE = (2, 4, 7, 10)


def _planted(g, shape):
    """uniform noise + 0.05 h - 0.03 w: rows and columns are told apart"""
    N, C, H, W = shape
    return (g.uniform(-1, 1, shape) + 0.05 * np.arange(H)[None, None, :, None]
            - 0.03 * np.arange(W)[None, None, None, :])


def _err(a, b):
    a = np.asarray(a, np.float64)
    assert a.shape == tuple(b.shape), (a.shape, tuple(b.shape))
    return float(np.abs(a - b.detach().numpy()).max())


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv2d_rect(shape):
    N, Cin, H, W, Cout, K, pad = shape
    g = np.random.default_rng(H * 100 + W)
    x = _planted(g, (N, Cin, H, W))
    w = g.uniform(-1, 1, (Cout, Cin, K, K)) / np.sqrt(Cin * K * K)
    b = g.uniform(-0.1, 0.1, Cout)
    y, win = O.conv2d_fwd(x, w, b, pad)
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    assert y.shape == (N, Cout, Ho, Wo)
    dy = _planted(g, y.shape)
    dx, dw, db = O.conv2d_bwd(dy, win, w, x.shape, pad)
    xt, wt, bt = (torch.from_numpy(a).requires_grad_() for a in (x, w, b))
    yt = F.conv2d(xt, wt, bt, padding=pad)
    yt.backward(torch.from_numpy(dy))
    errs = {"y": _err(y, yt), "dx": _err(dx, xt.grad), "dw": _err(dw, wt.grad), "db": _err(db, bt.grad)}
    print(shape, errs)
    assert max(errs.values()) <= BOUND, errs


def test_maxpool2_rect():
    g = np.random.default_rng(7)
    x = _planted(g, POOL_SHAPE)
    N, C, H, W = POOL_SHAPE
    # exact ties inside windows: the first element in row-major window order wins
    Hp, Wp = H // 2, W // 2
    p00, p01 = x[:, :, 0:2 * Hp:2, 0:2 * Wp:2], x[:, :, 0:2 * Hp:2, 1:2 * Wp:2]
    p11 = x[:, :, 1:2 * Hp:2, 1:2 * Wp:2]
    tie = g.uniform(size=p00.shape) < 0.3
    p01[tie] = p00[tie]
    p11[tie] = p00[tie]
    y, cache = O.maxpool2_fwd(x)
    assert y.shape == (N, C, H // 2, W // 2)
    dy = _planted(g, y.shape)
    dx = O.maxpool2_bwd(dy, cache)
    xt = torch.from_numpy(x).requires_grad_()
    yt = F.max_pool2d(xt, 2)
    yt.backward(torch.from_numpy(dy))
    errs = {"y": _err(y, yt), "dx": _err(dx, xt.grad)}
    print(errs)
    assert max(errs.values()) <= BOUND, errs
    assert np.all(dx[:, :, 2 * (H // 2):, :] == 0)       # the row the floor-mode pool never saw


@pytest.mark.parametrize("shape", [(s[0] * 2, s[4], s[2], s[3]) for s in CONV_SHAPES] + [POOL_SHAPE])
def test_bn_train_rect(shape):
    """two groups (G = 2): torch's batch_norm in training mode on each group's samples"""
    N, C, H, W = shape
    G = 2
    B = N // G
    g = np.random.default_rng(C * 10 + H)
    x = _planted(g, shape) * 1.5 + 0.3
    x[B:] *= 10.0                                          # group g scaled by 10^g
    gamma, beta = 1 + g.uniform(-0.2, 0.2, C), g.uniform(-0.2, 0.2, C)
    y, cache, stats = O.bn_train_fwd(x, gamma, beta, G, (2, 3))
    dy = _planted(g, shape)
    dx, dgamma, dbeta = O.bn_train_bwd(dy, cache)
    xt, gt, bt = (torch.from_numpy(a).requires_grad_() for a in (x, gamma, beta))
    yt = torch.cat([F.batch_norm(xt[i * B:(i + 1) * B], None, None, gt, bt, True, 0.1, O.BN_EPS) for i in range(G)])
    yt.backward(torch.from_numpy(dy))
    mean_t = torch.stack([xt[i * B:(i + 1) * B].mean((0, 2, 3)) for i in range(G)])
    var_t = torch.stack([xt[i * B:(i + 1) * B].var((0, 2, 3), unbiased=False) for i in range(G)])
    errs = {"y": _err(y, yt), "dx": _err(dx, xt.grad), "dgamma": _err(dgamma, gt.grad),
            "dbeta": _err(dbeta, bt.grad), "mean": _err(stats[0], mean_t),
            "var": _err(stats[1] / np.maximum(stats[1], 1), var_t / var_t.clamp_min(1))}
    assert stats[2] == B * H * W
    print(shape, errs)
    assert max(errs.values()) <= BOUND, errs
