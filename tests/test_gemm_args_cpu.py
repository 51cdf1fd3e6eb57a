"""Argument validation and split-K plans of the dense GEMM family (csrc/gemm.hip), on calls that
return before any launch (dummy pointers, no device).

The status codes are read from the code.  The planner table is the literal one of
tests/gemm_cases.py that test_gpu_gemm_edges.py runs: each case there exists for one tile and one
split count, and a planner change has to revisit the table rather than move a case off its path.
"""
import ctypes

import pytest

from tests import gemm_cases as GC

OK, SHAPE, ARG = 0, -1, -4
d = ctypes.c_void_p(4096)            # 16-byte aligned, never dereferenced
odd = ctypes.c_void_p(4104)          # 8 bytes off


@pytest.fixture
def lib():
    """The library, loaded when a test runs: a missing build fails the tests, not the collection."""
    from avdino._lib import lib as _lib
    return _lib


def test_gemm_status_codes(lib):
    def gemm(M=8, N=8, K=8, A=d, B=d, C=d, mode=1):
        return lib.avd_gemm(M, N, K, A, K, 1, B, N, 1, C, N, None, 1.0, 0.0, mode, None, 0, None)

    assert gemm(A=None) == ARG and gemm(B=None) == ARG and gemm(C=None) == ARG
    assert gemm(M=0) == SHAPE and gemm(N=0) == SHAPE and gemm(K=0) == SHAPE and gemm(M=-1) == SHAPE
    assert gemm(mode=3) == ARG and gemm(mode=-1) == ARG
    assert gemm(A=None, M=0) == ARG                     # the pointers are looked at first


def test_linear_bwd_status_codes(lib):
    def bwd(rows=8, O=8, In=8, dout=d, dout_ld=8, x=d, x_ld=8, W=d, dW=d, dX=d, dx_ld=8, db=None,
            mode=1, which=3, ws=None, ws_elems=0):
        return lib.avd_linear_bwd(rows, O, In, dout, dout_ld, x, x_ld, W, dW, dX, dx_ld, db, mode,
                                  which, ws, ws_elems, None)

    assert bwd(which=0) == ARG and bwd(which=4) == ARG
    assert bwd(mode=0) == ARG and bwd(mode=3) == ARG
    assert bwd(dout_ld=7) == SHAPE and bwd(x_ld=7) == SHAPE and bwd(dx_ld=7) == SHAPE
    assert bwd(rows=0) == SHAPE and bwd(O=0, dout_ld=0) == SHAPE and bwd(In=0, x_ld=0, dx_ld=0) == SHAPE
    # the bias gradient's chunk partials live in the workspace
    need = lib.avd_linear_bwd_ws_elems(8, 8, 8, 1)
    assert need == 64
    assert bwd(db=d) == ARG and bwd(db=d, ws=d, ws_elems=need - 1) == ARG
    # each part needs its own operands, and only those
    assert bwd(dout=None) == ARG
    assert bwd(x=None) == ARG and bwd(dW=None) == ARG and bwd(W=None) == ARG and bwd(dX=None) == ARG
    assert bwd(which=1, x=None, W=None, dX=None) == ARG
    assert bwd(which=2, W=None, x=None, dW=None) == ARG
    # which = 2 without x / dW and which = 1 without W / dX pass the argument checks: what
    # still refuses them here is a later check, so they got past the NULL test
    assert bwd(which=2, x=None, dW=None, mode=0) == ARG
    assert bwd(which=2, x=None, dW=None, dx_ld=7) == SHAPE
    assert bwd(which=1, W=None, dX=None, x_ld=7) == SHAPE


def test_hwc_status_codes(lib):
    def fwd(rows=8, O=8, C=8, HW=1, feat=d, Wp=d, out=d, out_ld=8):
        return lib.avd_linear_fwd_hwc(rows, O, C, HW, feat, Wp, None, out, out_ld, None, 0, None)

    assert fwd(C=4) == SHAPE and fwd(C=12, HW=3) == SHAPE         # In % 8
    assert fwd(out_ld=7) == SHAPE and fwd(rows=0) == SHAPE and fwd(HW=0) == SHAPE
    assert fwd(feat=odd) == ARG and fwd(Wp=odd) == ARG
    assert fwd(feat=None) == ARG and fwd(Wp=None) == ARG and fwd(out=None) == ARG

    need = lib.avd_linear_hwc_ws_elems(8, 8, 8)
    assert need == 64

    def bwd(rows=8, O=8, C=8, HW=1, dout=d, dout_ld=8, feat=d, Wp=d, dW=d, db=None, dX=d, which=3,
            ws=d, ws_elems=need):
        return lib.avd_linear_bwd_hwc(rows, O, C, HW, dout, dout_ld, feat, Wp, dW, db, dX, which, ws,
                                      ws_elems, None)

    assert bwd(C=4) == SHAPE and bwd(O=6, dout_ld=8) == SHAPE and bwd(dout_ld=10) == SHAPE
    assert bwd(dout_ld=4) == SHAPE and bwd(rows=0) == SHAPE
    assert bwd(dout=odd) == ARG and bwd(feat=odd) == ARG and bwd(Wp=odd) == ARG
    assert bwd(ws=None) == ARG and bwd(ws_elems=need - 1) == ARG
    assert bwd(which=0) == ARG and bwd(which=4) == ARG
    assert bwd(dout=None) == ARG and bwd(feat=None) == ARG and bwd(dX=None) == ARG
    assert bwd(which=2, feat=None, dW=None, ws=None) == ARG     # past the NULL test, no workspace

    P, I = ctypes.c_void_p, ctypes.c_int
    ptrs, ints = (P * 5)(*([4096] * 5)), (I * 5)(*([8] * 5))

    def weights(n, W=ptrs, Wp=ptrs, O=ints, C=ints, HW=ints):
        return lib.avd_linear_weight_hwc(n, W, Wp, O, C, HW, None)

    assert weights(0) == ARG and weights(5) == ARG and weights(-1) == ARG
    assert weights(1, W=None) == ARG and weights(1, HW=None) == ARG
    assert weights(2, W=(P * 2)(4096, None)) == ARG
    assert weights(2, O=(I * 2)(8, 0)) == SHAPE


def test_workspace_sizes_of_degenerate_problems(lib):
    for mode in (1, 2):
        for M, N, K in [(0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8), (8, 8, -5)]:
            assert lib.avd_gemm_ws_elems(M, N, K, mode) == 0
            assert lib.avd_linear_hwc_ws_elems(M, N, K) == 0
        assert lib.avd_linear_bwd_ws_elems(0, 8, 8, mode) == 0
        assert lib.avd_linear_bwd_ws_elems(8, 0, 8, mode) == 0
    # modes without split-K need none
    for mode in (0, 3, -1):
        assert lib.avd_gemm_ws_elems(5, 7, 32771, mode) == 0


@pytest.mark.parametrize("case", GC.GEMM_CASES, ids=GC.gemm_id)
def test_gemm_plan_table(lib, case):
    M, N, K, tile, S, last, _ = case
    need = GC.gemm_need(case)
    assert (need == 0) == (S == 1)
    for mode in (1, 2):
        assert lib.avd_gemm_ws_elems(M, N, K, mode) == need
    assert lib.avd_gemm_ws_elems(M, N, K, 0) == 0
    # the chunk is whole 64-wide k-tiles and the last one is what is left of K
    if S > 1:
        chunk = (K - last) // (S - 1)
        assert chunk % 64 == 0 and chunk * (S - 1) + last == K and 0 < last <= chunk


@pytest.mark.parametrize("case", GC.LINEAR_BWD_CASES, ids=GC.linear_bwd_id)
def test_linear_bwd_plan_table(lib, case):
    rows, O, In, _, _, s1, s2, need = case
    w1 = s1 * O * In if s1 > 1 else 0
    w2 = s2 * rows * In if s2 > 1 else 0
    assert need == w1 + w2 + GC.db_elems(rows, O)
    for mode in (1, 2):
        assert lib.avd_linear_bwd_ws_elems(rows, O, In, mode) == need
        assert lib.avd_gemm_ws_elems(O, In, rows, mode) == w1
        assert lib.avd_gemm_ws_elems(rows, In, O, mode) == w2


@pytest.mark.parametrize("rows,O", GC.DB_CASES)
def test_bias_gradient_partials(lib, rows, O):
    both = lib.avd_gemm_ws_elems(O, 8, rows, 1) + lib.avd_gemm_ws_elems(rows, 8, O, 1)
    assert lib.avd_linear_bwd_ws_elems(rows, O, 8, 1) == both + GC.db_elems(rows, O)


def test_bias_gradient_chunks_are_literal():
    assert [GC.db_elems(r, 1) for r in (1, 33, 127, 128, 129, 1028, 4100)] == [1, 33, 127, 128, 65, 115, 125]


@pytest.mark.parametrize("case", GC.HWC_CASES, ids=GC.hwc_id)
def test_hwc_plan_table(lib, case):
    rows, O, C, HW, sf, s1, s2, need = case
    In = C * HW
    wf = sf * rows * O if sf > 1 else 0
    w1 = s1 * O * In if s1 > 1 else 0
    w2 = s2 * rows * In if s2 > 1 else 0
    assert need == max(wf, w1 + w2 + GC.db_elems(rows, O))
    assert lib.avd_linear_hwc_ws_elems(rows, O, In) == need
    assert lib.avd_gemm_ws_elems(rows, O, In, 2) == wf
    assert lib.avd_gemm_ws_elems(O, In, rows, 2) == w1
    assert lib.avd_gemm_ws_elems(rows, In, O, 2) == w2
