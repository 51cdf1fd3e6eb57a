"""Argument validation of the loss, optimiser, eval and staging entry points (csrc/loss.hip,
optim.hip, eval.hip, stage.hip, xent.hip): the documented status codes, on calls that must
return before any launch (a dummy pointer, no device)."""
import ctypes

import pytest

OK, SHAPE, DTYPE, ARG = 0, -1, -2, -4
d = ctypes.c_void_p(4096)            # 16-byte aligned, never dereferenced
odd = ctypes.c_void_p(4100)          # not 16-byte aligned


@pytest.fixture
def lib():
    """The library, loaded when a test runs: a missing build fails the tests, not the collection."""
    from avdino._lib import lib as _lib
    return _lib


def test_status_codes_are_the_documented_ones():
    from avdino import _lib
    assert _lib.STATUS[SHAPE] == "AVD_ERR_SHAPE" and _lib.STATUS[DTYPE] == "AVD_ERR_DTYPE"
    assert _lib.STATUS[ARG] == "AVD_ERR_ARG" and _lib.F32 == 0 and _lib.BF16 == 1


def test_loss_heads_width_and_null(lib):
    def dino(s=d, work=d, P=128):
        return lib.avd_dino_loss(s, d, d, 3, 2, 5, P, 0.1, 0.04, 0.9, 0, d, d, d, work, None)

    assert dino(P=0) == SHAPE and dino(P=513) == SHAPE
    assert dino(s=None) == ARG and dino(work=None) == ARG
    assert lib.avd_mse_loss(d, d, 5, 0, d, d, d, None) == SHAPE
    assert lib.avd_mse_loss(d, d, 5, 513, d, d, d, None) == SHAPE
    assert lib.avd_mse_loss(d, None, 5, 128, d, d, d, None) == ARG
    assert lib.avd_l2norm_fwd(d, d, d, 5, 0, None) == SHAPE
    assert lib.avd_l2norm_fwd(d, d, d, 5, 513, None) == SHAPE
    assert lib.avd_l2norm_fwd(d, None, d, 5, 128, None) == ARG
    assert lib.avd_l2norm_bwd(d, d, d, d, 5, 0, None) == SHAPE
    assert lib.avd_l2norm_bwd(d, d, d, d, 5, 513, None) == SHAPE
    assert lib.avd_l2norm_bwd(d, d, d, None, 5, 128, None) == ARG


def test_softmax_xent_modes_targets_and_leading_dimensions(lib):
    def xent(R=5, C=8, ld=8, targets=d, mode=0, tgt_off=0, col_major=0, dl=d, ldd=8):
        return lib.avd_softmax_xent(d, ld, R, C, targets, mode, tgt_off, col_major, -1, 1.0, d, dl,
                                    ldd, 0, None)

    assert xent(mode=3) == ARG and xent(mode=-1) == ARG
    assert xent(mode=0, targets=None) == ARG
    assert xent(mode=1, tgt_off=4) == SHAPE            # R - 1 + tgt_off = 8 = C
    assert xent(mode=1, tgt_off=-1) == SHAPE
    # a leading dimension shorter than a row: row-major rows hold C elements, column-major R
    assert xent(ld=7) == SHAPE
    assert xent(ldd=7) == SHAPE
    assert xent(R=9, C=8, col_major=1, ld=8) == SHAPE
    assert xent(R=9, C=8, col_major=1, ld=9, ldd=8) == SHAPE
    assert xent(R=5, C=8, col_major=1, ld=4, ldd=5) == SHAPE
    # NT-Xent targets (r + R/2) % R are columns: R <= C
    assert xent(R=10, C=8, mode=2) == SHAPE
    assert xent(R=0) == SHAPE and xent(C=0, ld=0, ldd=0) == SHAPE


def test_argmax_leading_dimension(lib):
    assert lib.avd_argmax_rows(d, 9, 5, 10, d, None) == SHAPE
    assert lib.avd_argmax_correct(d, 9, 5, 10, d, d, None) == SHAPE
    assert lib.avd_argmax_rows(d, 10, 5, 10, None, None) == ARG
    assert lib.avd_argmax_correct(d, 10, 5, 10, None, d, None) == ARG


def test_cosine_consistency_views_and_outputs(lib):
    assert lib.avd_cosine_consistency(d, 1, 3, 16, 1.0, d, d, None) == SHAPE
    assert lib.avd_cosine_consistency(d, 33, 3, 16, 1.0, d, d, None) == SHAPE
    assert lib.avd_cosine_consistency(d, 4, 3, 16, 1.0, None, None, None) == ARG
    assert lib.avd_cosine_consistency(None, 4, 3, 16, 1.0, d, d, None) == ARG


def test_flat_updates_alignment_and_length(lib):
    hp = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.1, 0.001)
    for adam in (lib.avd_adam, lib.avd_adamw):
        assert adam(odd, d, d, d, 8, *hp, None) == SHAPE
        assert adam(d, d, d, odd, 8, *hp, None) == SHAPE
        assert adam(d, d, d, d, -1, *hp, None) == SHAPE
        assert adam(d, d, d, d, 0, *hp, None) == OK
        assert adam(d, None, d, d, 8, *hp, None) == ARG
    for adam_dev in (lib.avd_adam_dev, lib.avd_adamw_dev):
        assert adam_dev(d, odd, d, d, 8, d, 0.9, 0.999, 1e-8, 1e-2, None) == SHAPE
        assert adam_dev(d, d, d, d, -1, d, 0.9, 0.999, 1e-8, 1e-2, None) == SHAPE
        assert adam_dev(d, d, d, d, 0, d, 0.9, 0.999, 1e-8, 1e-2, None) == OK
        assert adam_dev(d, d, d, d, 8, None, 0.9, 0.999, 1e-8, 1e-2, None) == ARG
    assert lib.avd_ema(odd, d, 8, 0.99, None) == SHAPE and lib.avd_ema(d, odd, 8, 0.99, None) == SHAPE
    assert lib.avd_ema(d, d, -1, 0.99, None) == SHAPE and lib.avd_ema(d, d, 0, 0.99, None) == OK
    assert lib.avd_axpy(odd, d, 8, 1.0, None) == SHAPE and lib.avd_axpy(d, odd, 8, 1.0, None) == SHAPE
    assert lib.avd_axpy(d, d, -1, 1.0, None) == SHAPE and lib.avd_axpy(d, d, 0, 1.0, None) == OK
    assert lib.avd_step_begin(None, d, d, 0.9, 0.999, 1, None) == ARG
    assert lib.avd_step_begin(d, None, None, 0.9, 0.999, 1, None) == ARG


def test_counters_add_length(lib):
    assert lib.avd_counters_add(d, d, d, 0, None) == OK
    assert lib.avd_counters_add(d, d, d, -1, None) == SHAPE
    assert lib.avd_counters_add(d, None, d, 4, None) == ARG


def test_knn_select_limits(lib):
    def knn(M=4, N=20, K=5, C=10, ldS=20, Q=None, X=None, D=0):
        return lib.avd_knn_select(d, ldS, d, M, N, K, Q, X, D, d, C, d, d, None)

    assert knn(K=17) == SHAPE and knn(N=4, ldS=4, K=5) == SHAPE and knn(C=65) == SHAPE
    assert knn(ldS=19) == SHAPE and knn(K=0) == SHAPE and knn(C=0) == SHAPE
    assert knn(Q=d, X=None, D=8) == ARG
    assert knn(Q=d, X=d, D=0) == SHAPE


def test_stage_views_shape_and_dtype(lib):
    assert lib.avd_stage_views(d, 2, d, 4, d, 3, 786, d, 0, None) == SHAPE      # HW % 4
    assert lib.avd_stage_views(d, 2, d, 4, d, 3, 784, d, 2, None) == DTYPE
    assert lib.avd_stage_views(d, 2, None, 4, d, 3, 784, d, 0, None) == ARG     # L > 0 without l
    assert lib.avd_stage_views(d, 0, None, 0, d, 3, 784, d, 0, None) == SHAPE


def test_small_reductions_and_fused_xent_workspace(lib):
    assert lib.avd_sum(d, 0, 1.0, d, None) == SHAPE and lib.avd_sum(None, 4, 1.0, d, None) == ARG
    assert lib.avd_row_sqnorm(d, 0, 8, d, None) == SHAPE and lib.avd_row_sqnorm(d, 4, 0, d, None) == SHAPE
    assert lib.avd_bn_eval_coef(d, d, d, d, 1e-5, 0, d, d, None) == SHAPE
    assert lib.avd_bn_eval_coef(d, d, d, None, 1e-5, 4, d, d, None) == ARG
    assert lib.avd_xent_fused_ws(256, 256, 64) == SHAPE
    assert lib.avd_xent_fused_ws(256, 256, 128) > 0


def test_xent_fused_arguments(lib):
    """avd_xent_fused's own checks, in their order: null pointers (ARG), shapes and target
    ranges (SHAPE), then the workspace size (ARG) as the last gate before the launches.  No
    call here passes that gate: every one that passes the shape checks is given a workspace one
    element short, so ARG from such a call means 'accepted up to the workspace check'."""
    R, C, P, Bh = 10, 24, 128, 5
    need = lib.avd_xent_fused_ws(R, C, P)
    assert need > 0

    def xent(q=d, k=d, R=R, C=C, P=P, Bh=Bh, tgt=(5, 0), msk=(0, 5), loss=d, dq=d, dk=d, ws=d, short=1):
        n = lib.avd_xent_fused_ws(R, C, P)
        return lib.avd_xent_fused(q, k, R, C, P, Bh, tgt[0], tgt[1], msk[0], msk[1], 14.0, 0.1, loss,
                                  dq, dk, ws, max(n, 0) - short, None)

    for name in ("q", "k", "loss", "dq", "dk", "ws"):
        assert xent(**{name: None}) == ARG, name
    assert xent(P=64) == SHAPE
    assert xent(R=0) == SHAPE and xent(C=0) == SHAPE
    assert xent(Bh=0) == SHAPE and xent(Bh=11) == SHAPE         # Bh > R
    assert xent(Bh=4) == SHAPE                                  # R > 2 Bh
    assert xent(tgt=(-1, 0)) == SHAPE and xent(tgt=(20, 0)) == SHAPE        # tgt0 + Bh = 25 > C
    assert xent(tgt=(5, -1)) == SHAPE and xent(tgt=(5, 20)) == SHAPE        # tgt1 + (R - Bh) > C
    assert xent(R=9, tgt=(5, 21)) == SHAPE                      # ragged second half: 21 + 4 > C
    # the largest targets that fit, a ragged second half, no masks: accepted
    assert xent(tgt=(19, 19)) == ARG and xent(R=9, tgt=(19, 20)) == ARG and xent(msk=(-1, -1)) == ARG
    # one half (R = Bh): tgt1 is not read, tgt0 still is
    assert xent(Bh=10, tgt=(5, -1)) == ARG and xent(Bh=10, tgt=(5, 1000)) == ARG
    assert xent(Bh=10, tgt=(15, 0)) == SHAPE and xent(Bh=10, tgt=(14, 0)) == ARG
    # the workspace: one short is refused, and only that (the shape checks come first)
    assert xent(short=1) == ARG and xent(tgt=(-1, 0), short=1) == SHAPE and xent(ws=None, P=64) == ARG
