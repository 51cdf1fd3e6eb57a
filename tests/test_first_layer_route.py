"""Which kernels run the first conv layer of every shipped stack, per (N, B, need_dgrad) and per
route switch the tests flip (ConvBranch.CODES, CODES3, GRAM), as one table of literals:
(family, statistics pass, pooling pass, backward) or None for the stored-y generic path.  No GPU
needed: ConvBranch decides from the library's host-side row functions, and only whether they
serve (> 0) matters.

The decision is spread over four predicates in the forward (_recompute_ok / _gram_ok /
_pixel_major / _codes_ok) and inferred again by the backward from its ctx; ``first_layer_route``
below reads them the way forward and backward do.  The table is what a single route function
replacing them has to reproduce (tests/test_gpu_first_layer_launches.py ties its fields to the
launches).  The "single5_*" rows are one-layer stacks: no route, yet their stored-y first layer
is the one place where forward's recompute apply (RC_APPLY) runs in training."""
import itertools

import pytest
import torch

from avdino import spec as S
from avdino import ops
from avdino.engine import ConvBranch

STACKS = {
    "central_image": S.central_stack("s", S.CENTRAL_IMAGE_CONVS, 28),     # (1, 32, 5, 2) @ 28
    "central_audio": S.central_stack("s", S.CENTRAL_AUDIO_CONVS, 112),    # (1, 8, 5, 2) @ 112
    "cnn3_image": S.cnn3_stack("s", S.CNN3_IMAGE_CONVS, 28),              # (1, 32, 3, 1) @ 28
    "cnn3_audio": S.cnn3_stack("s", S.CNN3_AUDIO_CONVS, 112),             # (1, 32, 3, 1) @ 112
    # not shipped: the other recompute shapes ("rc"), and shapes / stacks without a route
    "rc16": S.cnn3_stack("s", [(1, 16, 3, 1), (16, 32, 3, 1)], 28),
    "rc64": S.cnn3_stack("s", [(1, 64, 3, 1), (64, 128, 3, 1)], 28),
    "single": S.cnn3_stack("s", [(1, 32, 3, 1)], 28),
    "w30": S.cnn3_stack("s", [(1, 32, 3, 1), (32, 64, 3, 1)], 30),        # W % 4 == 2
    # one layer, flatten tail: the first layer is also the last and stores y
    "single5_audio": S.central_stack("s", [(1, 8, 5, 2)], 112),
    "single5_image": S.central_stack("s", [(1, 32, 5, 2)], 28),
}
SHIPPED = ("central_image", "central_audio", "cnn3_image", "cnn3_audio")
SWITCHES = {"default": {}, "CODES=False": {"CODES": False}, "CODES3=False": {"CODES3": False},
            "GRAM=False": {"GRAM": False}}
ALL = tuple(SWITCHES)
G6, G2, G33 = (384, 64), (128, 64), (132, 4)      # (N, B): 6, 2 and 33 BN groups
LE32, ANY = (G6, G2), (G6, G2, G33)

# (stack, (N, B)s, need_dgrad, switch settings, (family, stats, pool, bwd)) -- bf16
ROWS = [
    ("central_audio", LE32, True, ("default", "CODES3=False"), ("audio", "gram", "codes", "codes_gram")),
    ("central_audio", LE32, True, ("CODES=False",), ("audio", "gram", "pass1", "moments")),
    ("central_audio", LE32, True, ("GRAM=False",), ("audio", "pass0", "codes", "codes")),
    ("central_audio", LE32, False, ("default", "CODES=False", "CODES3=False"), ("audio", "gram", "pass1", None)),
    ("central_audio", LE32, False, ("GRAM=False",), ("audio", "pass0", "pass1", None)),
    ("central_audio", (G33,), True, ALL, ("audio", "pass0", "pass1", "moments")),
    ("central_audio", (G33,), False, ALL, ("audio", "pass0", "pass1", None)),
    ("central_image", LE32, True, ("default", "CODES3=False", "GRAM=False"),
     ("image", "pixel_major", "codes", "codes")),
    ("central_image", LE32, True, ("CODES=False",), ("image", "pixel_major", "pixel_major", "moments")),
    ("central_image", (G33,), True, ALL, ("image", "pixel_major", "pixel_major", "moments")),
    ("central_image", ANY, False, ALL, ("image", "pixel_major", "pixel_major", None)),
    ("cnn3_image", LE32, True, ("default", "GRAM=False"), ("c3", "pass0", "codes", "codes")),
    ("cnn3_image", LE32, True, ("CODES=False", "CODES3=False"), ("c3", "pass0", "pass1", "moments")),
    ("cnn3_image", (G33,), True, ALL, ("c3", "pass0", "pass1", "moments")),
    ("cnn3_image", ANY, False, ALL, ("c3", "pass0", "pass1", None)),
    ("cnn3_audio", LE32, True, ("default", "GRAM=False"), ("c3", "pass0", "codes", "codes")),
    ("cnn3_audio", LE32, True, ("CODES=False", "CODES3=False"), ("c3", "pass0", "pass1", "moments")),
    ("cnn3_audio", (G33,), True, ALL, ("c3", "pass0", "pass1", "moments")),
    ("cnn3_audio", ANY, False, ALL, ("c3", "pass0", "pass1", None)),
    ("rc16", ANY, True, ALL, ("rc", "pass0", "pass1", "moments")),
    ("rc16", ANY, False, ALL, ("rc", "pass0", "pass1", None)),
    ("rc64", ANY, True, ALL, None),
    ("rc64", ANY, False, ALL, None),
    ("single", ANY, True, ALL, None),
    ("single", ANY, False, ALL, None),
    ("w30", ANY, True, ALL, None),
    ("w30", ANY, False, ALL, None),
    ("single5_audio", ANY, True, ALL, None),
    ("single5_audio", ANY, False, ALL, None),
    ("single5_image", ANY, True, ALL, None),
    ("single5_image", ANY, False, ALL, None),
]
CASES = [(stack, nb, nd, sw, exp) for stack, nbs, nd, sws, exp in ROWS for nb in nbs for sw in sws]


FAMILY = {(1, 8, 5, 2): "audio", (1, 32, 5, 2): "image", (1, 32, 3, 1): "c3"}


def first_layer_route(cb, N, B, need_dgrad):
    """ConvBranch.forward's choice for layer 0 (_first_layer_recompute_fwd's statistics and
    pooling passes) and _first_layer_recompute_bwd's branch for the ctx that forward leaves."""
    ci, co, k, pad = cb.stack.convs[0]
    H = cb.dims[0][0]
    if not (len(cb.stack.convs) > 1 and cb._recompute_ok(N, B, ci, H, co, k, pad, need_dgrad)):
        return None
    family = FAMILY.get((ci, co, k, pad), "rc")
    gram, pm, codes = cb._gram_ok(N, B), cb._pixel_major(N, B), cb._codes_ok(N, B, need_dgrad)
    assert codes in (None, family)
    # the backward without codes: pass 4 where it has rows, else the reduce + wgrad passes
    R4 = ops.cl_c1_recompute_rows(ops.C1_REDUCE_MOMENTS, cb.act, N, B, ci, H, H, co, k, pad)
    bwd = (None if not need_dgrad else ("codes_gram" if codes == "audio" and gram else "codes") if codes
           else "moments" if cb.RC_MOMENTS and R4 > 0 else "reduce_wgrad")
    return (family, "gram" if gram else "pixel_major" if pm else "pass0",
            "codes" if codes else "pixel_major" if pm else "pass1", bwd)


def _route(monkeypatch, stack, dtype, nb, need_dgrad, switch):
    for k in ("CODES", "CODES3", "GRAM"):
        monkeypatch.setattr(ConvBranch, k, SWITCHES[switch].get(k, True))
    return first_layer_route(ConvBranch(STACKS[stack], dtype), nb[0], nb[1], need_dgrad)


def test_rows_cover_every_case():
    seen = [c[:4] for c in CASES]
    assert len(seen) == len(set(seen))
    assert set(seen) == set(itertools.product(STACKS, ANY, (True, False), ALL))


@pytest.mark.parametrize("stack,nb,need_dgrad,switch,expected", CASES,
                         ids=[f"{c[0]}-{c[1][0]}x{c[1][1]}-{'train' if c[2] else 'teacher'}-{c[3]}"
                              for c in CASES])
def test_route_bf16(monkeypatch, stack, nb, need_dgrad, switch, expected):
    assert _route(monkeypatch, stack, torch.bfloat16, nb, need_dgrad, switch) == expected


@pytest.mark.parametrize("stack", list(STACKS))
def test_route_f32_is_the_stored_y_path(monkeypatch, stack):
    for nb, nd, sw in itertools.product(ANY, (True, False), ALL):
        assert _route(monkeypatch, stack, torch.float32, nb, nd, sw) is None


def test_recompute_passes_serve_a_shape_together():
    """avd_cl_c1_recompute_rows serves every pass of a shape or none (c1w3.hip: "every pass, or
    none"; the audio kernels' pass 4 rows are max(1, ...)): a first layer on the recompute route
    always has its one-pass backward (pass 4), so no row above ends in "reduce_wgrad"."""
    assert all(c[4] is None or c[4][3] != "reduce_wgrad" for c in CASES)
    served = 0
    for dt, co, (k, pad), H, (N, B) in itertools.product(
            (torch.bfloat16, torch.float32), (8, 16, 32, 64, 128), ((3, 1), (5, 2), (5, 0)),
            range(4, 132, 2), ANY + ((7168, 1024),)):
        rows = [ops.cl_c1_recompute_rows(p, dt, N, B, 1, H, H, co, k, pad) > 0 for p in range(5)]
        assert all(rows) or not any(rows), (dt, co, k, pad, H, N, B, rows)
        served += rows[0]
    assert served > 0


def test_recompute_passes_refuse_other_kernel_sizes():
    """The library serves 3x3 and 5x5 first layers only: no recompute pass has rows for any other
    kernel size, so "the statistics pass has rows" already implies k is 3 or 5."""
    for dt, ci, co, (k, pad), H, (N, B) in itertools.product(
            (torch.bfloat16, torch.float32), (1, 2), (8, 16, 32, 64, 128),
            ((1, 0), (2, 1), (4, 2), (7, 3), (9, 4)), range(4, 132, 2), ANY + ((7168, 1024),)):
        rows = [ops.cl_c1_recompute_rows(p, dt, N, B, ci, H, H, co, k, pad) for p in range(5)]
        assert not any(rows), (dt, ci, co, k, pad, H, N, B, rows)


@pytest.mark.parametrize("stack", ["single5_audio", "single5_image"])
def test_single_layer_stored_y_takes_the_recompute_apply(stack):
    """A one-layer stack has no route (its first layer is also its last and stores y), but in
    bf16 in front of a flatten tail (hwc: tail mode 0) ConvBranch.forward still pools it through
    cl_c1_recompute(C1_APPLY) rather than cl_bn_relu_pool: the stored-y branch's condition
    (first layer, mode 0, RC_APPLY, bf16, pass 1 has rows) holds.  It fails in f32 and in front
    of the f32 (c, h, w) flatten (mode 2)."""
    ci, co, k, pad = STACKS[stack].convs[0]
    H = STACKS[stack].hw

    def takes_apply(cb, N, B):
        return (cb._tail_mode() == 0 and cb.RC_APPLY and cb.act == torch.bfloat16 and
                ops.cl_c1_recompute_rows(ops.C1_APPLY, cb.act, N, B, ci, H, H, co, k, pad) > 0)

    for N, B in ANY:
        assert takes_apply(ConvBranch(STACKS[stack], torch.bfloat16, hwc=True), N, B)
        assert not takes_apply(ConvBranch(STACKS[stack], torch.float32, hwc=True), N, B)
        assert not takes_apply(ConvBranch(STACKS[stack], torch.bfloat16), N, B)


def test_shipped_first_layers_are_the_table():
    """Every first-layer shape of the shipped multimodal / unimodal / SimCLR stacks is a row above."""
    shipped = {(tuple(st.convs[0]), st.hw) for st in
               [b("s") for e in S.MULTI_ENCODERS.values() for b in (e[0], e[2])] +
               [e[1]("s") for e in S.UNI_ENCODERS.values()]}
    assert shipped == {(tuple(STACKS[n].convs[0]), STACKS[n].hw) for n in SHIPPED}
