"""ctypes binding of libavdino.so (include/avdino.h).

There is no fallback: if the shared library is missing or was built for another
architecture, importing this module raises, so nothing can silently run a CPU path.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AVDINO_LIB", os.path.join(_HERE, "libavdino.so"))
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "avdino.h"))

F32, BF16 = 0, 1

# the header's scalar types (a pointer of any kind is c_void_p)
_SCALARS = {
    "int": ctypes.c_int,
    "avd_dtype": ctypes.c_int,
    "long long": ctypes.c_longlong,
    "unsigned long long": ctypes.c_ulonglong,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
}
_RETURNS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char*": ctypes.c_char_p}


def _param_type(fn, text):
    if "*" in text:
        return ctypes.c_void_p
    words = [w for w in text.split() if w != "const"]
    for t in (" ".join(words), " ".join(words[:-1])):     # without / with a parameter name
        if t in _SCALARS:
            return _SCALARS[t]
    raise ImportError(f"avdino.h: {fn}: unrecognised parameter type {text!r}")


def parse_header(text):
    """(PROTOS, RESTYPES) of a header in include/avdino.h's C subset: once comments, preprocessor
    lines and the typedef / enum / extern "C" scaffolding are gone, every statement is
    ``RET avd_name(PARAMS);`` over the types above.  Anything else raises ImportError."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r"\b(typedef\s+)?(enum|struct)\b[^{};()]*\{[^{}]*\}[^{};()]*;", " ", text)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    protos, restypes = {}, {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.replace("}", " ").split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.+?)\b(avd_\w+) ?\(([^()]*)\)", stmt)
        if m is None:
            raise ImportError(f"avdino.h: not a function declaration: {stmt!r}")
        ret, fn, params = m.group(1).replace(" *", "*").strip(), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise ImportError(f"avdino.h: {fn}: unrecognised return type {ret!r}")
        restypes[fn] = _RETURNS[ret]
        protos[fn] = [] if params == "void" else [_param_type(fn, a.strip()) for a in params.split(",")]
    return protos, restypes


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise ImportError(f"include/avdino.h not readable at {HEADER_PATH} ({e}): the ctypes "
                          f"prototypes are taken from it") from None


# name -> argtypes and name -> restype of every function the header declares
PROTOS, RESTYPES = parse_header(_read_header())


class AvdError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libavdino.so not found at {LIB_PATH}: build it with "
            f"`make -C multimodal-ssl-avmnist_amd/csrc` (or __graft_entry__.build()). "
            f"There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, args in PROTOS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = RESTYPES[name]
    return lib


lib = _load()

STATUS = {-1: "AVD_ERR_SHAPE", -2: "AVD_ERR_DTYPE", -3: "AVD_ERR_HIP", -4: "AVD_ERR_ARG"}


def check(rc, name="avd"):
    if rc != 0:
        msg = STATUS.get(rc, str(rc))
        if rc == -3:
            msg += f" ({lib.avd_last_error().decode()})"
        raise AvdError(f"{name} failed: {msg}")
    return rc


def call(name, *args):
    return check(getattr(lib, name)(*args), name)
