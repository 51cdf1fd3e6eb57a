"""The C-ABI library loads and exports every symbol include/avdino.h declares, the ctypes
prototypes cover them, and host-side validation rejects bad arguments before any launch
(no GPU needed: nothing here launches a kernel)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "avdino.h")


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_functions():
    fns = header_functions()
    assert "avd_cl_conv_fwd" in fns and "avd_adam" in fns and len(fns) >= 25


def test_library_exports_every_declared_symbol():
    from avdino import _lib
    missing = [f for f in header_functions() if not hasattr(_lib.lib, f)]
    assert not missing, missing


def header_declarations():
    """{name: (return type text, [parameter texts])} read from the header by this test's own
    regex, independent of avdino._lib's parser."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t*]*?)\s*\b(avd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        params = " ".join(params.split())
        out[name] = (" ".join(ret.split()), [] if params == "void" else [a.strip() for a in params.split(",")])
    return out


def test_ctypes_prototypes_cover_header():
    """Every function the header declares is bound on lib with as many argtypes as it has
    parameters, a c_void_p exactly where the parameter is a pointer, and the declared restype."""
    from avdino import _lib
    decls = header_declarations()
    assert set(decls) == set(header_functions()) == set(_lib.PROTOS) == set(_lib.RESTYPES)
    rets = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}
    for name, (ret, params) in decls.items():
        fn = getattr(_lib.lib, name)
        assert fn.restype is rets[ret] is _lib.RESTYPES[name], name
        assert list(fn.argtypes) == _lib.PROTOS[name] and len(fn.argtypes) == len(params), name
        assert [t is ctypes.c_void_p for t in fn.argtypes] == ["*" in a for a in params], name


def test_ctypes_prototypes_match_hand_written_signatures():
    """Signatures written out by hand from the header text: together they cover every scalar
    type, pointers of each kind, (void) and both non-int returns."""
    from avdino import _lib
    P, I, L, U, F, D = (ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong,
                        ctypes.c_float, ctypes.c_double)
    want = {
        "avd_version": (I, []),
        "avd_last_error": (ctypes.c_char_p, []),
        "avd_gemm": (I, [I, I, I, P, L, L, P, L, L, P, L, P, F, F, I, P, L, P]),
        "avd_step_begin": (I, [P, P, P, D, D, U, P]),
        "avd_gelu_fwd": (I, [P, P, L, I, F, U, P, P]),
        "avd_lstm_ws": (I, [I, I, I, P, P]),
        "avd_linear_bwd_ws_elems": (L, [I, I, I, I]),
        "avd_mx_weight_bytes": (L, [I, I, I, I]),
        "avd_linear_weight_hwc": (I, [I, P, P, P, P, P, P]),
        "avd_cl_weight_layout": (I, [P, P, I, I, I, I, I, P]),
    }
    for name, (ret, args) in want.items():
        fn = getattr(_lib.lib, name)
        assert _lib.PROTOS[name] == args and list(fn.argtypes) == args, name
        assert _lib.RESTYPES[name] is ret and fn.restype is ret, name


def test_header_parser_rejects_what_it_does_not_know():
    from avdino._lib import parse_header
    protos, rets = parse_header('extern "C" {\ntypedef enum { A = 0 } avd_dtype;\n/* c */ int avd_f(avd_dtype dt,\n'
                                '  const unsigned long long* s, unsigned long long n);\n}\n')
    assert protos == {"avd_f": [ctypes.c_int, ctypes.c_void_p, ctypes.c_ulonglong]}
    assert rets == {"avd_f": ctypes.c_int}
    with pytest.raises(ImportError, match=r"avd_f.*short"):
        parse_header("int avd_f(int a, short b);")
    with pytest.raises(ImportError, match=r"avd_f.*avd_options"):       # a struct by value
        parse_header("typedef struct { int a; } avd_options;\nint avd_f(avd_options o, void* stream);")
    with pytest.raises(ImportError, match=r"avd_f.*float"):
        parse_header("float avd_f(void);")
    with pytest.raises(ImportError, match=r"avd_f.*void\*"):
        parse_header("void* avd_f(int a);")
    with pytest.raises(ImportError, match="unsigned x"):
        parse_header("int avd_f(unsigned x);")
    with pytest.raises(ImportError, match="not a function declaration"):
        parse_header("int avd_f(int (*cb)(int));")
    with pytest.raises(ImportError, match="not a function declaration"):
        parse_header("static const int avd_n = 3;")


def test_missing_header_fails_loudly(tmp_path, monkeypatch):
    """The prototypes come from the header alone: where it cannot be read, the import-time read
    raises ImportError, as a missing library does."""
    from avdino import _lib
    assert os.path.samefile(_lib.HEADER_PATH, HEADER)
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "avdino.h"))
    with pytest.raises(ImportError, match="avdino.h"):
        _lib._read_header()


def test_host_helpers():
    from avdino._lib import lib
    assert lib.avd_version() >= 1
    assert lib.avd_cl_stat_rows(112, 112, 512, 5, 8, 16, 1) == 57344
    assert lib.avd_cl_stat_rows(14, 14, 512, 3, 32, 64, 1) == 1024
    assert lib.avd_cl_wgrad_chunks(7168, 16, 8, 5) == 512
    assert lib.avd_cl_wgrad_chunks(7168, 64, 32, 5) == 256
    assert lib.avd_cl_wgrad_chunks(12, 16, 8, 5) == 12
    assert lib.avd_colstats_parts(6144) == 384       # 16-row partials


def test_argument_validation_without_launch():
    from avdino._lib import lib
    # null pointers -> AVD_ERR_ARG; bad shapes -> AVD_ERR_SHAPE; bad dtype -> AVD_ERR_DTYPE
    assert lib.avd_cl_conv_fwd(None, None, None, None, None, 1, 1, 1, 8, 28, 28, 16, 5, 2, None) == -4
    dummy = ctypes.c_void_p(16)
    assert lib.avd_cl_conv_fwd(dummy, dummy, None, dummy, None, 1, 1, 1, 8, 28, 28, 16, 7, 2, None) == -1
    assert lib.avd_cl_conv_fwd(dummy, dummy, None, dummy, None, 7, 1, 1, 8, 28, 28, 16, 5, 2, None) == -4
    assert lib.avd_bn_finalize(dummy, 0, 1, 1, 2, dummy, dummy, 1e-5, 0.1, dummy, dummy, dummy,
                               dummy, None, None, None, 0, None) == -1
    assert lib.avd_stage_views(dummy, 2, None, 1, None, 4, 784, dummy, 0, None) == -4
    assert lib.avd_stage_views(dummy, 2, None, 0, None, 4, 783, dummy, 0, None) == -1
    assert lib.avd_act_fwd(dummy, dummy, 0, None, None, 4, 1, 8, 1.0, 0, None) == -1


def test_product_fails_loudly_without_library(tmp_path, monkeypatch):
    """No silent fallback: pointing the loader at a missing library raises on import."""
    import importlib
    import sys
    monkeypatch.setenv("AVDINO_LIB", str(tmp_path / "nope.so"))
    sys.modules.pop("avdino._lib", None)
    with pytest.raises(ImportError):
        importlib.import_module("avdino._lib")
    monkeypatch.delenv("AVDINO_LIB")
    sys.modules.pop("avdino._lib", None)
    importlib.import_module("avdino._lib")
