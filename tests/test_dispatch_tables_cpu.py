"""The sizes the LSTM, cross-attention and ViT dispatchers accept (csrc/lstm.hip, xattn.hip, vit.hip:
one template instantiation per value) against the sets the Python layer publishes and against the
case tables of the float64 parity tests.  The sizing queries are host functions that give the
shape verdict without a launch, so this runs without a GPU.

A size added to a dispatcher fails here until ops / spec publish it and a parity case launches it.
"""
import ctypes

from avdino import ops, spec
from avdino._lib import lib
from tests import test_gpu_lstm as TL
from tests import test_gpu_vit_ops as TV
from tests import test_gpu_xattn as TX


def lstm_accepts(H, N=3, T=5):
    a, b = ctypes.c_longlong(0), ctypes.c_longlong(0)
    rc = lib.avd_lstm_ws(N, T, H, ctypes.byref(a), ctypes.byref(b))
    assert rc in (0, -1), (H, rc)
    return rc == 0


def test_lstm_hidden_sizes():
    accepted = {H for H in range(1, 161) if lstm_accepts(H)}
    assert accepted == set(ops.LSTM_HIDDEN) == set(spec.LSTM_HIDDEN)
    assert spec.LSTM_DIMS == tuple(2 * h for h in spec.LSTM_HIDDEN)
    assert accepted == set(TL.HS) == {c[1] for c in TL.CASES}


def test_xattn_dims():
    accepted = {E for E in range(1, 1041) if lib.avd_xattn_bwd_ws(1, 3, 17, E) > 0}
    assert accepted == set(ops.XATTN_DIMS)
    assert accepted == set(TX.DIMS)
    assert set(TX.TWO_DIR_DIMS) <= accepted


def test_mhsa_head_dims_and_token_limit():
    ts = (1, 255, 256, 257)
    ok = {(dh, T) for dh in range(1, 161) for T in ts if lib.avd_mhsa_bwd_ws(2, 3, T, dh) > 0}
    dhs = {dh for dh, _ in ok}
    assert dhs == set(ops.MHSA_HEAD_DIMS)
    assert ok == {(dh, T) for dh in dhs for T in ts if T <= ops.MHSA_TMAX}      # the same T for every dh
    assert ops.MHSA_TMAX == 256 and lib.avd_mhsa_bwd_ws(2, 3, ops.MHSA_TMAX + 1, 32) < 0
    assert dhs == set(TV.MHSA_DHS)
    assert ops.MHSA_TMAX in TV.MHSA_TS and ops.MHSA_TMAX - 1 in TV.MHSA_TS and max(TV.MHSA_TS) == ops.MHSA_TMAX
    # the dropout cases stay inside the accepted set
    assert all(dh in dhs and T <= ops.MHSA_TMAX for _n, _h, T, dh, _p in TV.MHSA_DROPOUT_CASES)


def test_layer_norm_widths():
    accepted = {E for E in range(1, 545) if lib.avd_ln_bwd_ws(7, E) > 0}
    assert accepted == set(range(32, ops.LN_EMAX + 1, 32))
    table = set(TV.LN_ES) | {TV.LN_CAP_E}
    assert table <= accepted
    assert min(accepted) in table and ops.LN_EMAX in table
    assert any(E % 64 == 32 for E in table)                   # a lane's chunk half valid
    assert any(E & (E - 1) for E in table)                    # not a power of two
