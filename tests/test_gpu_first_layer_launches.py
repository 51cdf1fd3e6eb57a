"""ConvBranch launches for its first conv layer what the route table says (first_layer_route of
tests/test_first_layer_route.py, which reads the engine's predicates as forward does): a lone
branch per shipped first-layer stack (bf16, N = 4 in two BN groups), one training forward +
backward and one forward without a backward, under every route switch the tests flip, with
recorders over the first-layer entry points of avdino.ops.  The recorded set is compared with a
literal map from the route's fields (the vocabulary of tests/test_first_layer_route.py) to entry
points.  Numerical parity of the routes is tests/test_gpu_conv1_routes.py's and
tests/test_gpu_c1r3_codes.py's; here the first layer's gradients only have to be finite."""
from collections import OrderedDict

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, B = 4, 2
SWITCHES = {"default": {}, "CODES=False": {"CODES": False}, "CODES3=False": {"CODES3": False},
            "GRAM=False": {"GRAM": False}}
STACKS = ("central_image", "central_audio", "cnn3_image", "cnn3_audio")

# route field -> recorded entry points ("name[pass]" for cl_c1_recompute, "[codes]" / "[None]" for
# a pooling pass with / without a code buffer)
STATS = {"gram": {"c1_gram", "c1_gram_finalize"}, "pixel_major": {"c1r5_stats"},
         "pass0": {"cl_c1_recompute[0]"}}
POOL = {("audio", "codes"): {"c1_apply_codes[codes]"}, ("image", "codes"): {"c1r5_apply_codes[codes]"},
        ("c3", "codes"): {"c1r3_apply_codes[codes]"}, ("image", "pixel_major"): {"c1r5_apply_codes[None]"},
        **{(f, "pass1"): {"cl_c1_recompute[1]"} for f in ("audio", "image", "c3")}}
BWD = {("audio", "codes_gram"): {"c1_moments_codes_ng", "c1_codes_combine_gram"},
       ("audio", "codes"): {"c1_moments_codes", "c1_codes_combine"},
       ("image", "codes"): {"c1r5_moments_codes", "c1r5_codes_combine"},
       ("c3", "codes"): {"c1r3_moments_codes", "c1r3_codes_combine"},
       **{(f, "moments"): {"cl_c1_recompute[4]", "cl_c1_recompute_combine"} for f in ("audio", "image", "c3")},
       **{(f, None): set() for f in ("audio", "image", "c3")}}
# positional index of the ``codes`` argument of the pooling passes that take one
APPLY_CODES = {"c1_apply_codes": 6, "c1r5_apply_codes": 6, "c1r3_apply_codes": 6}
ENTRY = sorted({n.split("[")[0] for m in (STATS, POOL, BWD) for s in m.values() for n in s})


def _record(mp, ops):
    seen = []

    def wrap(name):
        orig = getattr(ops, name)

        def rec(*a, **kw):
            if name == "cl_c1_recompute":
                seen.append(f"{name}[{a[0]}]")
            elif name in APPLY_CODES:
                seen.append(f"{name}[{'None' if a[APPLY_CODES[name]] is None else 'codes'}]")
            else:
                seen.append(name)
            return orig(*a, **kw)
        return rec

    for name in ENTRY:
        mp.setattr(ops, name, wrap(name))
    return seen


def _branch(name):
    from avdino import spec as S
    from avdino.engine import ConvBranch
    from avdino.params import ParamStore
    convs, hw, central = {"central_image": (S.CENTRAL_IMAGE_CONVS, 28, True),
                          "central_audio": (S.CENTRAL_AUDIO_CONVS, 112, True),
                          "cnn3_image": (S.CNN3_IMAGE_CONVS, 28, False),
                          "cnn3_audio": (S.CNN3_AUDIO_CONVS, 112, False)}[name]
    sd = OrderedDict()
    if central:
        S._central_lenet(sd, "s.encoder", convs, 64)
    else:
        S._cnn3(sd, "s.encoder", convs, 16)
    store = ParamStore(sd, "cuda", seed=3, has_teacher=False)
    stack = (S.central_stack if central else S.cnn3_stack)("s.encoder", convs, hw)
    return ConvBranch(stack, torch.bfloat16), store, hw


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name", STACKS)
def test_first_layer_launches_are_the_route(monkeypatch, name, switch):
    from avdino import ops
    from avdino.engine import ConvBranch, Workspace
    from tests.test_first_layer_route import first_layer_route
    for k in ("CODES", "CODES3", "GRAM"):
        monkeypatch.setattr(ConvBranch, k, SWITCHES[switch].get(k, True))
    cb, store, hw = _branch(name)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(N, hw, hw, 1, generator=g).to(torch.bfloat16).cuda()
    ws = Workspace(store.device)
    first = [k for k in store.live_keys
             if k.startswith((cb.stack.conv_keys[0] + ".", cb.stack.bn_keys[0] + "."))]
    assert len(first) == 4, first
    for need_dgrad in (True, False):
        route = first_layer_route(cb, N, B, need_dgrad)
        assert route is not None, "every shipped first layer is on a recompute route at (4, 2)"
        family, stats, pool, bwd = route
        assert (bwd is None) == (not need_dgrad)
        with monkeypatch.context() as mp:
            seen = _record(mp, ops)
            feat, ctx = cb.forward(ws, store, "t", x, N, N // B, need_dgrad=need_dgrad)
            assert set(seen) == STATS[stats] | POOL[family, pool], (route, seen)
            assert len(seen) == len(set(seen)), seen
            if need_dgrad:
                del seen[:]
                for k in first:
                    store.grad_of(k).fill_(float("nan"))
                dfeat = torch.randn(feat.shape, generator=g).to(feat.dtype).cuda()
                cb.backward(ws, store, ctx, dfeat)
                torch.cuda.synchronize()
                assert set(seen) == BWD[family, bwd], (route, seen)
                assert len(seen) == len(set(seen)), seen
                for k in first:
                    assert torch.isfinite(store.grad_of(k)).all(), k
            # library passes 2 and 3 (reduce, wgrad) are no part of any route
            assert not {"cl_c1_recompute[2]", "cl_c1_recompute[3]"} & set(seen)
    torch.cuda.synchronize()
