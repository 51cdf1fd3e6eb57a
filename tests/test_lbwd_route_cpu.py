"""ConvBranch's routing of the fused layer backward, on CPU (no launch; the library's slab and
MX queries are replaced by stubs): which class switch governs which layer, the single predicate
_layer_bwd_slabs, the alternating dX buffers of consecutive fused layers, and the fp8 predicate
_fused_bwd, which moves only the 56^2 layer off its MX kernels and agrees with _layer_bwd_slabs
about the pooled-gradient layout and the BN group count."""
import pytest

torch = pytest.importorskip("torch")

from avdino import spec  # noqa: E402

SERVED = {(8, 56, 16), (16, 28, 32)}          # (Cin, H, Cout) of the fused launch, 5x5 pad 2


@pytest.fixture
def branch(monkeypatch):
    from avdino import engine as EN
    from avdino import ops

    def slabs(dtype, N, Cin, H, W, Cout, K, pad):
        ok = dtype == torch.bfloat16 and H == W and (Cin, H, Cout) in SERVED and (K, pad) == (5, 2)
        return 512 if ok else 0
    monkeypatch.setattr(ops, "cl_layer_bwd_slabs", slabs)
    monkeypatch.setattr(ops, "mx_wgrad_chunks", lambda *a: 256)
    monkeypatch.setattr(ops, "mx_conv_serves", lambda *a: True)
    for name in ("LAYER_BWD", "LAYER_BWD_28", "FP8_FUSED_BWD"):
        monkeypatch.setattr(EN.ConvBranch, name, True)

    def make(fp8=False, dtype=torch.bfloat16):
        st = spec.central_stack("student.audio_encoder.0", spec.CENTRAL_AUDIO_CONVS, 112)
        return EN.ConvBranch(st, dtype, fp8=fp8)
    return EN, make


BF16_WT = (object(), object(), None, None)    # (forward rows, dgrad rows, no MX layouts)


def test_each_fused_layer_has_its_own_switch(branch):
    EN, make = branch
    br = make()
    assert [d[0] for d in br.dims] == [112, 56, 28, 14]
    N, B = 7168, 1024
    fused = lambda: [bool(br._layer_bwd_slabs(i, N, B, 0, BF16_WT)) for i in range(4)]  # noqa: E731
    assert fused() == [False, True, True, False]
    EN.ConvBranch.LAYER_BWD = False
    assert fused() == [False, False, True, False]
    EN.ConvBranch.LAYER_BWD, EN.ConvBranch.LAYER_BWD_28 = True, False
    assert fused() == [False, True, False, False]


def test_the_predicate_declines_what_the_launch_cannot_take(branch):
    _EN, make = branch
    br = make()
    N = 7168
    assert br._layer_bwd_slabs(2, N, 1024, 0, BF16_WT) == 512
    assert br._layer_bwd_slabs(2, N, N // 9, 0, BF16_WT) == 0            # 9 groups > APPLY_GMAX
    assert br._layer_bwd_slabs(2, N, 1024, 2, BF16_WT) == 0              # f32 (c, h, w) gradient
    assert br._layer_bwd_slabs(2, N, 1024, 0, (object(), None, None, None)) == 0   # no dgrad rows
    assert br._layer_bwd_slabs(2, N, 1024, 0, (object(), object(), None, (1, 2))) == 0   # MX dgrad
    assert make(dtype=torch.float32)._layer_bwd_slabs(2, N, 1024, 0, BF16_WT) == 0


def test_consecutive_fused_layers_alternate_dx_buffers(branch):
    EN, _make = branch
    names = [EN.ConvBranch._lb_dx_name(n) for n in range(4)]
    assert names[0] == "bwd_dx_lb"                  # one fused layer: the buffer it always had
    assert all(a != b for a, b in zip(names, names[1:]))
    assert "bwd_dx" not in names                    # the separate dgrad's buffer is some layer's gout


def test_fp8_moves_only_the_56_layer_off_its_mx_kernels(branch):
    EN, make = branch
    br = make(fp8=True)
    N, B = 4096 * 7, 4096
    assert [br._fused_bwd(i, N, B) for i in range(4)] == [False, True, False, False]
    assert br._mx_ok(2, N, B, dgrad=True) and br._mx_wgrad(2, N, B)       # 28^2 stays MX
    assert not br._mx_ok(1, N, B, dgrad=True) and not br._mx_wgrad(1, N, B)
    assert br._mx_ok(1, N, B)                                             # its forward stays MX
    # the 28^2 layer's MX layouts keep it off the fused launch; the 56^2 layer takes it
    assert br._layer_bwd_slabs(2, N, B, 0, (None, None, (1, 2), (3, 4))) == 0
    assert br._layer_bwd_slabs(1, N, B, 0, (None, object(), (1, 2), None)) == 512
    # more groups than the fused apply holds: the layout choice follows the launch choice
    assert not br._fused_bwd(1, N, N // 9) and br._mx_ok(1, N, N // 9, dgrad=True)
    assert br._layer_bwd_slabs(1, N, N // 9, 0, (None, object(), (1, 2), None)) == 0
    EN.ConvBranch.LAYER_BWD = False
    assert not br._fused_bwd(1, N, B) and br._mx_wgrad(1, N, B)
