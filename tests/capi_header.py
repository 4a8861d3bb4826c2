"""The prototypes of include/voltrix_capi.h as ctypes types, for the tests that hold the binding (voltrix/capi.py::SIGNATURES) to the header."""
import ctypes
import os
import re

from conftest import REPO

HEADER = os.path.join(REPO, "include", "voltrix_capi.h")

_INT_P = ctypes.POINTER(ctypes.c_int)
# every type spelling the header uses; one outside it is an error here, not something to skip
PARAMETER_TYPES = {"void*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
                   "double": ctypes.c_double, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int*": _INT_P,
                   "const int*": _INT_P}
RETURN_TYPES = {"void": None, "int": ctypes.c_int, "int64_t": ctypes.c_int64}


def _spelling(text: str) -> str:
    return re.sub(r"\s*\*\s*", "*", " ".join(text.split()))


def prototypes():
    """``{name: (return type, [(parameter type, parameter name), ...])}`` of every ``voltrix_*`` function, in the header's order."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    found = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\n\*]*?)\b(voltrix_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        assert name not in found, f"{name} is declared twice"
        args = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            ctype, arg = re.fullmatch(r"(.*?)(\w+)", param.strip(), flags=re.S).groups()
            assert _spelling(ctype) in PARAMETER_TYPES, f"{name}: parameter type {_spelling(ctype)!r} is not in the binding's vocabulary"
            args.append((PARAMETER_TYPES[_spelling(ctype)], arg))
        assert _spelling(ret) in RETURN_TYPES, f"{name}: return type {_spelling(ret)!r} is not in the binding's vocabulary"
        found[name] = (RETURN_TYPES[_spelling(ret)], args)
    # nothing that looks like a call or a declaration of a voltrix_ function escaped the prototype pattern
    assert sorted(found) == sorted(set(re.findall(r"\b(voltrix_[a-z0-9_]+)\s*\(", text)))
    return found
