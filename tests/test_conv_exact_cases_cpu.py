"""The case table of the bit-exact conv-block tests (tests/conv_exact_cases.py), checked without
a device: every exactness condition the GPU test relies on is asserted on the float64 reference
alone, per case (a case that misses one is a bad case: replace it), and the reference itself is
held to torch's CPU float32 convolution on the same integers, bit for bit -- float32 is exact
there too -- so that an error in the reference cannot pass for a kernel bug."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import numpy_oracle as O  # noqa: E402
from tests import conv_exact_cases as X  # noqa: E402

F64 = torch.float64
IDS = [X.cid(c) for c in X.ALL]


def test_table_rows_are_distinct_and_small():
    assert len({c[:8] for c in X.ALL}) == len(X.ALL)
    for N, B, Cin, H, W, Cout, K, pad, kinds, rows in X.ALL:
        assert N <= 8 and N % B == 0 and max(H, W) <= 112 and K in (3, 5)
        assert (Cin == 1 or Cin % 8 == 0) and Cout % 8 == 0
        assert ("f" in kinds) == (rows is not None)


def test_kinds_follow_the_served_rule():
    """A row's kinds name an entry point exactly where it serves the row in some type (the rows
    kept for the weight gradient alone aside), and the mirror rows exist: the input gradient
    reaches 24, 40 and 72 output channels, the forward 24, 40 and 72 too."""
    for c in X.ALL:
        if c[8] == "w":
            continue
        for k in "fd":
            assert (k in c[8]) == (X.serves(c, k, False) or X.serves(c, k, True)), (X.cid(c), k)
    assert {c[5] for c in X.having("f")} >= {24, 40, 72}
    assert {c[2] for c in X.having("d")} >= {24, 40, 72}
    assert {c[2] for c in X.having("w")} >= {1, 8, 24} and {c[5] for c in X.having("w")} >= {24, 40, 72}
    assert any(c[0] == 5 for c in X.having("w")) and any(X.out_hw(c)[1] % 8 for c in X.having("w"))


@pytest.mark.parametrize("case", X.having("f", X.ALL), ids=X.cid)
def test_forward_conditions(case):
    N, B = case[:2]
    y, scale = X.fwd_ref(case, "map")
    assert float(scale.max()) < 2 ** 24                       # sum |x||w| + |bias|
    assert bool((y.abs() > 256).any()), "no value above 256: the store's rounding is not exercised"
    assert bool(X.bf16_ties(y).any()), "no exact tie"
    assert not bool(X.bf16_exact(y).all())
    ys, sc = X.fwd_ref(case, "stats")
    assert float(sc.max()) < 2 ** 24
    # |y| <= 256 and, the bias being a half-integer, the stronger: the stored bf16 y IS y
    assert float(ys.abs().max()) <= 256 and bool(X.bf16_exact(ys).all())
    # sum y^2 (and so every partial sum of y or y^2, quarter-integers) exact in f32
    for pv in (None, X.pivot_of(case)):
        st = X.stats_ref(ys, B, pv)
        d = ys if pv is None else ys - pv.view(1, -1, 1, 1)
        assert float(st[..., 1].max()) < 2 ** 22
        assert float(d.abs().reshape(N // B, B, case[5], -1).sum((1, 3)).max()) < 2 ** 22


@pytest.mark.parametrize("case", X.having("d", X.ALL), ids=X.cid)
def test_dgrad_conditions(case):
    _, scale = X.dgrad_ref(case, "map")
    assert float(scale.max()) < 2 ** 24


@pytest.mark.parametrize("case", X.having("w", X.ALL), ids=X.cid)
def test_wgrad_conditions(case):
    _, scale = X.wgrad_ref(case, "map")
    assert float(scale.max()) < 2 ** 24                       # sum |x||dy| per weight


@pytest.mark.parametrize("case", X.ALL, ids=X.cid)
def test_reference_equals_torch_float32(case):
    """forward, input gradient and weight gradient of torch.nn.functional.conv2d in float32 on
    the CPU (exact on these integers) == the float64 tap loops, bit for bit; and the tap loops ==
    oracle.numpy_oracle on the forward."""
    pad = case[7]
    for kind in ("map", "stats"):
        x, w, b = X.fwd_data(case, kind)
        dy = X.bwd_data(case, "map")
        x32 = x.float().requires_grad_(True)
        w32 = w.float().requires_grad_(True)
        y32 = torch.nn.functional.conv2d(x32, w32, b.float(), padding=pad)
        y32.backward(dy.float())
        assert torch.equal(y32.detach(), X.conv_fwd64(x, w, b, pad).float())
        assert torch.equal(x32.grad, X.conv_dgrad64(dy, w, case[3], case[4], pad).float())
        assert torch.equal(w32.grad, X.conv_wgrad64(x, dy, case[6], pad).float())
    x, w, b = X.fwd_data(case, "map")
    yo, win = O.conv2d_fwd(x.numpy(), w.numpy(), b.numpy(), pad)
    assert np.array_equal(yo, X.fwd_ref(case, "map")[0].numpy())
    dy = X.bwd_data(case, "map")
    dxo, dwo, _ = O.conv2d_bwd(dy.numpy(), win, w.numpy(), x.shape, pad)
    assert np.array_equal(dxo, X.dgrad_ref(case, "map")[0].numpy()) if "d" in case[8] else True
    assert np.array_equal(dwo, X.conv_wgrad64(x, dy, case[6], pad).numpy())


def test_bf16_helpers():
    t = torch.tensor([256.0, 257.0, 258.0, 259.0, 260.0, 128.5, 3.25, 513.0, 514.0], dtype=F64)
    assert X.bf16_ties(t).tolist() == [False, True, False, True, False, True, False, False, True]
    assert t.float().bfloat16().double().tolist()[:5] == [256.0, 256.0, 258.0, 260.0, 260.0]
    assert X.bf16_exact(t).tolist() == [True, False, True, False, True, False, True, False, False]


# ------------------------------------------------------------------ BN -> ReLU -> pool block
@pytest.mark.parametrize("HW", X.POOL_HW, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("C", X.POOL_C)
def test_pool_reference_equals_oracle_on_planted_ties(C, HW):
    """The test-owned first-max pooling / routing == oracle.numpy_oracle.maxpool2_fwd / bwd on
    the block's data: exact ties in pairs and in all four pixels, windows whose maximum is 0."""
    H, W = HW
    y, scale, shift, _coef, _m, _i, gout = X.block_data(C, H, W)
    N, B = X.POOL_N, X.POOL_B
    z = torch.relu(y * X.per_sample(scale, N, B) + X.per_sample(shift, N, B))
    pooled, arg = X.pool_ref(z)
    po, cache = O.maxpool2_fwd(z.numpy())
    assert np.array_equal(po, pooled.numpy()) and np.array_equal(cache[0], arg.numpy())
    assert np.array_equal(O.maxpool2_bwd(gout.numpy(), cache), X.route_ref(gout, arg, H, W).numpy())
    win = torch.stack([z[:, :, i:2 * (H // 2):2, j:2 * (W // 2):2] for i, j in ((0, 0), (0, 1), (1, 0), (1, 1))], -1)
    top = win == pooled.unsqueeze(-1)
    assert bool(((top.sum(-1) == 2) & (pooled > 0)).any()) and bool(((top.sum(-1) == 4) & (pooled > 0)).any())
    assert bool((pooled == 0).any()) and all(bool(((arg == k) & (pooled > 0)).any()) for k in range(4))
    assert bool((scale < 0).any()) and bool((scale > 0).any())


@pytest.mark.parametrize("HW", X.POOL_HW, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("C", X.POOL_C)
def test_block_data_is_exact(C, HW):
    """Every intermediate of the block is exactly representable whatever algebraic form a kernel
    uses: z and the pooled map in bf16, dy in f32 (and its bf16 rounding does round, ties
    included), the backward sums below 2^23 in their unit."""
    H, W = HW
    N, B = X.POOL_N, X.POOL_B
    y, scale, shift, coef, mean, invstd, gout = X.block_data(C, H, W)
    pooled, nib, dz, dy, sums, a2 = X.block_ref(y, scale, shift, coef, mean, invstd, gout, B)
    assert bool(X.bf16_exact(y).all()) and bool(X.bf16_exact(gout).all()) and bool(X.bf16_exact(pooled).all())
    assert torch.equal(dy.float().double(), dy)
    assert not bool(X.bf16_exact(dy).all()) and bool(X.bf16_ties(dy).any())
    # every term dz (y - mean) invstd is a multiple of 1/4: the sums are exact in f32 below 2^22
    assert float(dz.abs().reshape(N // B, B, C, -1).sum((1, 3)).max()) < 2 ** 22
    assert float(a2.max()) < 2 ** 22
    assert torch.equal((dz * 4).round(), dz * 4)


@pytest.mark.parametrize("case", X.LAYER_BWD + X.APPLY_WGRAD, ids=X.cid)
def test_fused_backward_data_is_exact(case):
    """dy (bf16) is a multiple of `unit` everywhere, and the conv gradients of it stay below
    2^24 units per output element: exact in f32 in any order."""
    r = X.fused_ref(case)
    assert bool(X.bf16_exact(r["dy"]).all())
    assert torch.equal((r["dy"] / r["unit"]).round(), r["dy"] / r["unit"])
    assert float(r["dx_abs"].max()) / r["unit"] < 2 ** 24
    assert float(r["dw_abs"].max()) / r["unit"] < 2 ** 24
    assert not bool(X.bf16_exact(r["dx"]).all()), "dx needs no rounding: the store is not exercised"
