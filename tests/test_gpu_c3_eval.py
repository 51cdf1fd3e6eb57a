"""The fused eval-mode 3x3 layer (avd_c3_conv_eval: conv + BatchNorm affine + ReLU + 2x2
max-pool [+ global average] in one launch, no conv output in memory) against the two launches it
replaces (avd_cl_conv_fwd without statistics, then avd_cl_bn_relu_pool) on the same inputs:
bit-identical (torch.equal), so no tolerance is involved.  Shapes: rows tiled inside a sample with
a last partial tile, whole-map packing with a ragged sample count, odd maps (floor pooling),
one to four input chunks and output groups, N = 1; with the grid capped every block walks many
items (the persistent, double-buffered path).  One float64 sanity case bounds the pooled map by
the band tests/test_gpu_cl.py applies to avd_cl_conv_fwd (rel-L2 5e-3, one bf16 rounding).
The route test compares ConvBranch.forward_eval with EVAL_FUSED on and off on both SimCLR
encoder stacks: it is also what admits a first layer to the recompute route."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BF = torch.bfloat16
TOL_BF16 = 5e-3      # tests/test_gpu_cl.py TOL["bf16"]: stored bf16 maps vs float64

CASES = {  # name: (N, H, C, O, mode)
    "a": (3, 56, 32, 64, 0),
    "b": (3, 28, 64, 128, 0),
    "c": (5, 14, 128, 256, 1),
    "d": (5, 14, 32, 64, 0),
    "e": (11, 7, 64, 128, 1),
    "f": (1, 56, 32, 64, 0),
}


@pytest.fixture(scope="module")
def ops():
    from avdino import ops as _ops
    return _ops


def _inputs(name):
    N, H, C, O, mode = CASES[name]
    g = torch.Generator().manual_seed(100 + ord(name))
    x = (torch.rand(N, H, H, C, generator=g) * 2 - 1).to(BF)
    w = ((torch.rand(O, C, 3, 3, generator=g) * 2 - 1) / (3 * C ** 0.5))
    b = torch.rand(O, generator=g) * 0.2 - 0.1
    scale = torch.rand(O, generator=g) + 0.5
    scale[1::2] *= -1                 # both signs
    scale[3] = 0.0                    # one exact zero channel
    shift = torch.rand(O, generator=g) * 0.6 - 0.3
    shift[5::8] = -50.0               # all-negative channels: pooled output all zero
    return x.cuda(), w.cuda(), b.cuda(), scale.cuda(), shift.cuda()


def _layout(ops, w):
    O, C = w.shape[:2]
    wk = torch.empty(ops.cl_weight_elems(O, C, 3, 0), device="cuda", dtype=BF)
    ops.cl_weight_layout(w, wk, 0)
    return wk


def _out(N, H, O, mode):
    if mode == 0:
        return torch.full((N, H // 2, H // 2, O), float("nan"), device="cuda", dtype=BF)
    return torch.full((N, O), float("nan"), device="cuda")


def _two_launches(ops, name, x, wk, b, scale, shift):
    N, H, C, O, mode = CASES[name]
    y = torch.empty(N, H, H, O, device="cuda", dtype=BF)
    ops.cl_conv_fwd(x, wk, b, y, None, N, N, C, H, H, O, 3, 1)
    out = _out(N, H, O, mode)
    ops.cl_bn_relu_pool(y, scale, shift, out, mode, N, N, O, H, H)
    return y, out


_REF = {}


def _reference(ops, name):
    """Inputs and the two-launch result of a case, computed once (default options)."""
    if name not in _REF:
        x, w, b, scale, shift = _inputs(name)
        wk = _layout(ops, w)
        y, out = _two_launches(ops, name, x, wk, b, scale, shift)
        torch.cuda.synchronize()
        _REF[name] = (x, w, wk, b, scale, shift, y, out)
    return _REF[name]


def _check_case(ops, name):
    N, H, C, O, mode = CASES[name]
    x, _w, wk, b, scale, shift, _y, ref = _reference(ops, name)
    out = _out(N, H, O, mode)
    launched = ops.c3_conv_eval(x, wk, b, scale, shift, out, mode, N, H, H, C, O)
    assert launched == ops.c3_eval_serves(N, H, H, C, O, mode)
    if not launched:
        # declined (nothing launched, no error): the engine keeps the two launches
        assert torch.isnan(out.float()).all()
        _assert_branch_falls_back(ops, N, H, C, O)
        return
    torch.cuda.synchronize()
    assert not torch.isnan(out.float()).any()
    assert torch.equal(out, ref), (out.float() - ref.float()).abs().max().item()
    # the all-negative channels pool to exactly zero, the zero-scale channel to relu(shift)
    assert (ref[..., 5::8] == 0).all()


def _assert_branch_falls_back(ops, N, H, C, O):
    """A layer the launcher declines runs on the two launches inside ConvBranch.forward_eval."""
    feats = _branch_features([(1, C, 3, 1), (C, O, 3, 1)], 2 * H, N, (True,))
    assert torch.isfinite(feats[0]).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_c3_conv_eval_bit_identical(ops, name):
    _check_case(ops, name)


@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_c3_conv_eval_capped_grid(ops, avd_opts, name):
    _reference(ops, name)            # the oracle runs with the default options
    avd_opts(grid_cap=3)
    _check_case(ops, name)


def test_c3_conv_eval_declines_without_error(ops):
    """Shapes outside the table: 0 from both entry points, nothing written, no exception."""
    for (N, H, C, O, mode) in [(2, 64, 32, 64, 0), (2, 28, 8, 64, 0), (2, 28, 32, 48, 0), (2, 56, 32, 64, 1)]:
        assert not ops.c3_eval_serves(N, H, H, C, O, mode)
    N, H, C, O = 2, 56, 32, 64       # a 56 x 56 map does not fit a tile whole: no fused average
    x = torch.zeros(N, H, H, C, device="cuda", dtype=BF)
    wk = torch.zeros(ops.cl_weight_elems(O, C, 3, 0), device="cuda", dtype=BF)
    coef = torch.ones(2, O, device="cuda")
    out = _out(N, H, O, 1)
    assert ops.c3_conv_eval(x, wk, None, coef[0], coef[1], out, 1, N, H, H, C, O) is False
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_c3_conv_eval_float64_sanity(ops):
    """Case (b) against float64: conv of the bf16 operands in float64, rounded through bf16 at y
    as the kernel does, affine + ReLU + pool in float64; the band of the stored bf16 maps."""
    N, H, C, O, mode = CASES["b"]
    x, w, wk, b, scale, shift, _y, _ref = _reference(ops, "b")
    out = _out(N, H, O, mode)
    assert ops.c3_conv_eval(x, wk, b, scale, shift, out, mode, N, H, H, C, O)
    xd = x.double().permute(0, 3, 1, 2).cpu()
    wd = w.to(BF).double().cpu()
    y = torch.nn.functional.conv2d(xd, wd, b.double().cpu(), padding=1)
    y = y.float().to(BF).double()
    z = torch.relu(y * scale.double().cpu()[None, :, None, None] + shift.double().cpu()[None, :, None, None])
    ref = torch.nn.functional.max_pool2d(z, 2).permute(0, 2, 3, 1)
    got = out.double().cpu()
    err = (got - ref).norm().item() / max(ref.norm().item(), 1e-30)
    print(f"c3_conv_eval vs float64: rel-L2 {err:.3e}")
    assert err < TOL_BF16, err


# ------------------------------------------------------------------ the engine route
def _branch_features(convs, hw, N, flags, seed=11, central=False):
    """ConvBranch.forward_eval features of a random cnn3 (or CentralNet) stack, once per
    EVAL_FUSED flag."""
    from collections import OrderedDict

    from avdino.engine import ConvBranch, Workspace
    from avdino.params import ParamStore
    from avdino.spec import _central_lenet, _cnn3, central_stack, cnn3_stack
    sd = OrderedDict()
    if central:
        _central_lenet(sd, "t.encoder", convs, 64)
    else:
        _cnn3(sd, "t.encoder", convs, 16)
    store = ParamStore(sd, "cuda", seed=seed, has_teacher=False)
    g = torch.Generator().manual_seed(seed)
    for k, (shape, kind) in store.spec.items():      # non-trivial BatchNorm state
        if kind in ("rm", "bn_b"):
            store[k].copy_(torch.rand(shape, generator=g) * 0.4 - 0.2)
        elif kind == "rv":
            store[k].copy_(torch.rand(shape, generator=g) + 0.5)
        elif kind == "bn_w":
            store[k].copy_((torch.rand(shape, generator=g) + 0.5) * (torch.rand(shape, generator=g) > 0.2))
    x = (torch.rand(N, hw, hw, 1, generator=g) * 2 - 1).to(BF).cuda()
    stack = (central_stack if central else cnn3_stack)("t.encoder", convs, hw)
    outs = []
    old = ConvBranch.EVAL_FUSED
    try:
        for flag in flags:
            ConvBranch.EVAL_FUSED = flag
            br = ConvBranch(stack, BF)
            outs.append(br.forward_eval(Workspace(store.device), store, "ev", x, N).float().clone())
    finally:
        ConvBranch.EVAL_FUSED = old
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("N", [5, 16])
@pytest.mark.parametrize("kind", ["image_simple", "spectrogram_simple"])
def test_forward_eval_fused_route_bit_identical(ops, kind, N):
    from avdino.spec import CNN3_AUDIO_CONVS, CNN3_IMAGE_CONVS
    convs, hw = (CNN3_IMAGE_CONVS, 28) if kind == "image_simple" else (CNN3_AUDIO_CONVS, 112)
    # the fused route is really taken: every layer after the first is served
    H = hw
    for i, (ci, co, _k, _p) in enumerate(convs):
        if i > 0:
            assert ops.c3_eval_serves(N, H, H, ci, co, 1 if i == len(convs) - 1 else 0)
        H //= 2
    fused, plain = _branch_features(convs, hw, N, (True, False))
    assert torch.isfinite(plain).all() and plain.abs().max() > 0
    assert torch.equal(fused, plain), (fused - plain).abs().max().item()


@pytest.mark.parametrize("N", [5, 16])
@pytest.mark.parametrize("kind", ["central_image", "central_audio"])
def test_forward_eval_central_first_layer_route_bit_identical(ops, kind, N):
    """The CentralNet stacks: their 5x5 mid layers keep the two launches, and their first layer
    takes the recompute apply pass only because this comparison is bit-identical."""
    from avdino.spec import CENTRAL_AUDIO_CONVS, CENTRAL_IMAGE_CONVS
    convs, hw = (CENTRAL_IMAGE_CONVS, 28) if kind == "central_image" else (CENTRAL_AUDIO_CONVS, 112)
    fused, plain = _branch_features(convs, hw, N, (True, False), central=True)
    assert torch.isfinite(plain).all() and plain.abs().max() > 0
    assert torch.equal(fused, plain), (fused - plain).abs().max().item()
