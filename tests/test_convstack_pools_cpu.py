"""ConvStackSpec's per-layer pool flags and spec.lstm_image_stack (LSTMImageEncoder.cnn,
models/dino.py:75-115: the third block has no MaxPool2d).  No device needed."""
import pytest

from avdino import spec


def _existing_stacks():
    stacks = {}
    for name, (istack, _il, astack, _al, _sd) in spec.MULTI_ENCODERS.items():
        stacks[name + ".image"] = istack("student")
        stacks[name + ".audio"] = astack("student")
    for name, (_m, stack, _lins, _sd) in spec.UNI_ENCODERS.items():
        stacks[name] = stack("student")
    return stacks


def _pooled_dims(stack):
    """layer_dims() as it was before the flags: every layer pooled."""
    out, h = [], stack.hw
    for (_ci, _co, k, pad) in stack.convs:
        ho = h + 2 * pad - k + 1
        out.append((h, ho, ho // 2))
        h = ho // 2
    return out


def test_default_flags_leave_every_existing_stack_unchanged():
    stacks = _existing_stacks()
    assert len(stacks) >= 12
    for name, st in stacks.items():
        assert st.pools == (True,) * len(st.convs), name
        assert st.nhwc_tail is False, name
        assert st.layer_dims() == _pooled_dims(st), name
    # literal values of three of them, so that this test does not only mirror the code
    assert stacks["multi_central.image"].layer_dims() == [(28, 28, 14), (14, 10, 5)]
    assert stacks["multi_simple.audio"].layer_dims() == [(112, 112, 56), (56, 56, 28), (28, 28, 14), (14, 14, 7)]
    assert stacks["spectrogram_lstm"].layer_dims() == [(112, 112, 56), (56, 56, 28), (28, 28, 14)]
    assert stacks["multi_central.image"].flat == 64 * 5 * 5
    assert stacks["multi_simple.image"].flat == 128


def test_lstm_image_stack_is_28_14_7_7_with_49_tokens_of_128():
    st = spec.lstm_image_stack("student.image_encoder.cnn")
    assert st.convs == spec.CNN3_IMAGE_CONVS and st.hw == 28 and not st.gap
    assert st.pools == (True, True, False) and st.nhwc_tail
    assert st.layer_dims() == [(28, 28, 14), (14, 14, 7), (7, 7, 7)]
    assert st.conv_keys == [f"student.image_encoder.cnn.{i}" for i in (0, 4, 8)]
    assert st.bn_keys == [f"student.image_encoder.cnn.{i}" for i in (1, 5, 9)]
    tokens, channels = st.layer_dims()[-1][2] ** 2, st.convs[-1][1]
    assert (tokens, channels) == (49, 128) and st.flat == 49 * 128


def test_conv_branch_refuses_an_unpooled_stack_and_takes_every_existing_one():
    """The library has no kernels for conv -> BN -> ReLU without a pool yet: ConvBranch must say
    so when it is built, not run a pooled pass over the layer."""
    torch = pytest.importorskip("torch")
    from avdino.engine import ConvBranch
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(NotImplementedError, match="without a max-pool"):
            ConvBranch(spec.lstm_image_stack("student.image_encoder.cnn"), dtype)
        for name, st in _existing_stacks().items():
            assert ConvBranch(st, dtype).dims == st.layer_dims(), name


def _stack(pools, gap=False, nhwc_tail=True):
    return spec.ConvStackSpec(spec.CNN3_IMAGE_CONVS, 28, gap, ["c0", "c1", "c2"], ["b0", "b1", "b2"],
                              pools=pools, nhwc_tail=nhwc_tail)


@pytest.mark.parametrize("pools", [(False, True, True), (True, False, True), (True, False, False)])
def test_an_unpooled_layer_that_is_not_the_last_raises(pools):
    with pytest.raises(ValueError, match="only the last"):
        _stack(pools)


def test_an_unpooled_last_layer_needs_an_nhwc_tail_and_no_gap():
    with pytest.raises(ValueError, match="nhwc_tail"):
        _stack((True, True, False), nhwc_tail=False)
    with pytest.raises(ValueError, match="nhwc_tail"):
        _stack((True, True, False), gap=True)
    with pytest.raises(ValueError, match="flags"):
        _stack((True, False))
    assert _stack((True, True, False)).layer_dims()[-1] == (7, 7, 7)
    assert _stack((True, True, True)).layer_dims()[-1] == (7, 7, 3)
