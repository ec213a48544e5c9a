"""The ctypes table of projectedlmc._hip against include/plmc.h, for every symbol the header declares (no GPU, no library).

The compiler holds every C wrapper against the header; this holds the Python side against the same header: each declaration
`ret plmc_name(args);` is mapped to ctypes argument types (any pointer -> c_void_p, int -> c_int, int64_t -> c_int64, double ->
c_double, (void) -> none) and compared with _hip._TYPED[base] for base_f32 / base_f64 and with _hip._PLAIN[name][0] for the rest.
"""
import ctypes
import os
import re

from projectedlmc import _hip

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plmc.h")
SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}


def _declarations():
    """{name: [ctypes type of each parameter]} of every function the header declares."""
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))
    out = {}
    for m in re.finditer(r"\b(plmc_\w+)\s*\(([^()]*)\)\s*;", text):
        name, params = m.group(1), " ".join(m.group(2).split())
        assert name not in out, "%s is declared twice" % name
        out[name] = [] if params == "void" else [_ctype(p) for p in params.split(",")]
    return out


def _ctype(param):
    if "*" in param:
        return ctypes.c_void_p
    words = [w for w in param.split() if w != "const"]
    assert len(words) == 2 and words[0] in SCALARS, "parameter %r: no ctypes mapping" % param
    return SCALARS[words[0]]


def test_parser_reads_the_forms_the_header_uses():
    assert _ctype("const float *X") is ctypes.c_void_p and _ctype("void *stream") is ctypes.c_void_p
    assert _ctype("int64_t lda") is ctypes.c_int64 and _ctype("int q") is ctypes.c_int and _ctype("double eps") is ctypes.c_double
    decl = _declarations()
    assert decl["plmc_version"] == [] and decl["plmc_pad"] == [ctypes.c_int64]
    assert len(decl) > 250              # every family form of every operation, both element types


def test_declared_names_are_the_exported_symbols():
    exported = _hip.exported_symbols()
    assert len(exported) == len(set(exported))
    assert set(_declarations()) == set(exported)


def test_every_argtypes_row_matches_its_declaration():
    decl = _declarations()
    wrong = []
    for name, args in sorted(decl.items()):
        base = name[:-4] if name.endswith(("_f32", "_f64")) else None
        have = _hip._TYPED[base] if base in _hip._TYPED else _hip._PLAIN[name][0]
        if list(have) != args:
            wrong.append(name)
    assert not wrong, "argtypes differ from include/plmc.h: %s" % ", ".join(wrong)
