"""ctypes binding of the C ABI in include/pcs.h (libpcs.so, built in-tree for gfx950).

The header is the table: its structs, prototypes, enumerators and PCS_ABI_VERSION are parsed once
at import into the ``ct.Structure`` classes, ``SIGNATURES`` and the constants below, so a new entry
point is declared in the header only (tests/golden/abi_tables.json records the result).  A header
of EXT_HEADERS adds entry points of the same library beside pcs.h's (EXT_SIGNATURES), and so does one
of DENSE_HEADERS, into a table of its own (DENSE_SIGNATURES; tests/golden/abi_tables_dense.json), and
one of FOLD_HEADERS likewise (FOLD_SIGNATURES; tests/golden/abi_tables_fold.json).

There is no fallback: if the library is missing or fails to load, every GPU entry point
raises.  ``torch`` is imported first so that the HIP runtime torch ships (same SONAME
``libamdhip64.so.7``) is the one the library binds to -- one runtime per process.
"""
from __future__ import annotations

import ctypes as ct
import os
import re

import torch  # noqa: F401  (loads torch's HIP runtime before libpcs.so)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libpcs.so")
HEADER_PATH = os.path.join(_HERE, "..", "include", "pcs.h")   # csrc/Makefile's ../../include/pcs.h
# Headers beside pcs.h that add entry points of the same library and nothing else (no struct, no
# constant, no change to pcs.h's tables or to PCS_ABI_VERSION): read after pcs.h into EXT_SIGNATURES
EXT_HEADERS = ("pcs_segmax.h",)
# The same for the dense voxel U-Net's kernels, kept in a table of their own (DENSE_SIGNATURES) so that
# EXT_SIGNATURES stays the segmented max's
DENSE_HEADERS = ("pcs_dense.h",)
# The same for the folded inference convolutions (pcs_*_affine), in FOLD_SIGNATURES
FOLD_HEADERS = ("pcs_fold.h",)

_SCALARS = {"int": ct.c_int, "int32_t": ct.c_int32, "int64_t": ct.c_int64, "uint64_t": ct.c_uint64,
            "float": ct.c_float}
_POINTEES = {*_SCALARS, "void", "uint8_t", "char"}
_DECL = re.compile(r"(const\s+)?(\w+)\s*(\*?)\s*(\w+)$")      # [const] TYPE [*]NAME
_ITEMS = [(kind, re.compile(r"\s*" + rx)) for kind, rx in (
    ("opaque", r"typedef\s+struct\s+\w+\s*\*\s*(\w+)\s*;"),
    ("struct", r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;"),
    ("enum", r"enum\s*\{([^{}]*)\}\s*;"),
    ("function", r"((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*\(([^(){};]*)\)\s*;"))]


def _fail(what, text):
    raise ImportError(f"include/pcs.h: {what}: {' '.join(text.split())[:100]!r}")


def _declarators(stmt, types):
    """(name, type, is_pointer, is_const) of each declarator of `[const] TYPE [*]a, [*]b`."""
    first, *more = (s.strip() for s in stmt.split(","))
    m = _DECL.match(first)
    if not m or m.group(2) not in types:
        _fail("unknown declaration", stmt)
    out = [(m.group(4), m.group(2), bool(m.group(3)), bool(m.group(1)))]
    for s in more:
        n = re.match(r"(\*?)\s*(\w+)$", s)
        if not n:
            _fail("unknown declaration", stmt)
        out.append((n.group(2), m.group(2), bool(n.group(1)), out[0][3]))
    return out


def _value_type(base, pointer, opaque, text):
    if pointer or base in opaque:
        return ct.c_void_p
    if base not in _SCALARS:
        _fail("unknown type of a value", text)
    return _SCALARS[base]


def parse_header(text):
    """(constants {X: int} of every PCS_X enumerator and integer define, structs {C name: [(field,
    ctype)]}, functions [(name, restype text, [(parameter, type, is_pointer, is_const)])]) of the
    header text.  Anything it does not understand raises ImportError naming the text."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)
    consts, structs, functions, opaque = {}, {}, [], set()

    def directive(m):
        d = m.group(0).strip()
        v = re.fullmatch(r"#define\s+PCS_(\w+)\s+(-?\d+)", d)
        if v:
            consts[v.group(1)] = int(v.group(2))
        elif not re.fullmatch(r"#(ifndef\s+\w+|define\s+\w+|endif|include\s+<\w+\.h>)", d):
            _fail("unknown directive", d)
        return " "
    text = re.sub(r"^[ \t]*#.*$", directive, text, flags=re.M)
    pos, end = 0, len(text.rstrip())
    while pos < end:
        for kind, rx in _ITEMS:
            m = rx.match(text, pos)
            if m:
                break
        else:
            _fail("unknown declaration", text[pos:])
        types = _POINTEES | opaque | set(structs)
        if kind == "opaque":
            opaque.add(m.group(1))
        elif kind == "struct":
            stmts = [s for s in m.group(1).split(";") if s.strip()]
            structs[m.group(2)] = [(name, _value_type(base, ptr, opaque, s))
                                   for s in stmts for name, base, ptr, _ in _declarators(s, types)]
        elif kind == "enum":
            items = [s.strip() for s in m.group(1).split(",")]
            for s in items[:-1] + [s for s in items[-1:] if s]:   # C allows one trailing comma
                v = re.fullmatch(r"PCS_(\w+)\s*=\s*(-?\d+)", s)
                if not v:
                    _fail("enumerator without an integer value", s)
                consts[v.group(1)] = int(v.group(2))
        else:
            params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
            params = [_declarators(p, types)[0] for p in params]
            for p, (_, base, ptr, _) in zip(m.group(3).split(","), params):
                _value_type(base, ptr, opaque, p)
            functions.append((m.group(2), " ".join(m.group(1).split()), params))
        pos = m.end()
    return consts, structs, functions


def _class_name(c_name):   # pcs_pool_bwd_args -> PoolBwdArgs
    return "".join(p.capitalize() for p in c_name.split("_")[1:])


def _bind(structs, functions):
    """The module's tables from a parsed header: struct classes, SIGNATURES, and per function the
    (parameter name, C type text, tensor dtypes accepted or None, struct class or None) of call()."""
    classes = {c: type(_class_name(c), (ct.Structure,), {"_fields_": fields, "__module__": __name__})
               for c, fields in structs.items()}
    restypes = {"int": ct.c_int, "int64_t": ct.c_int64, "const char *": ct.c_char_p}
    every = [d for d in vars(torch).values() if isinstance(d, torch.dtype)]
    byte = frozenset(d for d in every if d.itemsize == 1)   # keep bits are uint8, fp8 operands a float8 dtype
    int8b = frozenset(d for d in every if d.itemsize == 8 and not d.is_floating_point and not d.is_complex)
    tensors = {"float": frozenset([torch.float32]), "int32_t": frozenset([torch.int32]), "int64_t": int8b,
               "uint64_t": int8b, "uint8_t": byte, "void": frozenset()}   # empty: any dtype
    signatures, params = [], {}
    for name, res, ps in functions:
        if res not in restypes:
            _fail("unknown return type", f"{res} {name}")
        on_stream = any(base == "pcs_stream_t" for _, base, _, _ in ps)
        argtypes, info = [], []
        for pname, base, ptr, const in ps:
            ctext = f"{'const ' if const else ''}{base}{' *' if ptr else ''}"
            dtypes = struct = None
            if not ptr:
                at = _SCALARS.get(base, ct.c_void_p)   # (parse_header let only scalars and pcs_stream_t through)
            elif base in classes:
                at = ct.POINTER(struct := classes[base])
            elif base == "char":
                at = ct.c_char_p
            elif base == "int32_t" and not const and not on_stream:   # a host out-parameter
                at, ctext = ct.POINTER(ct.c_int32), ctext + " on the host"
            else:
                at, dtypes = ct.c_void_p, tensors.get(base)
            argtypes.append(at)
            info.append((pname, ctext, dtypes, struct))
        signatures.append((name, restypes[res], argtypes))
        params[name] = tuple(info)
    return classes, signatures, params


if not os.path.exists(HEADER_PATH):
    raise ImportError(f"pcs_amd reads its C ABI from {HEADER_PATH}, which is missing")
with open(HEADER_PATH) as _f:
    _consts, _structs, _functions = parse_header(_f.read())
if "ABI_VERSION" not in _consts:
    _fail("missing define", "PCS_ABI_VERSION")


def parse_extension(main_text, ext_text, main=None):
    """The functions an extension header adds to main_text's (pcs.h's): it is parsed behind pcs.h, which
    it includes for the types, and may declare functions only.  main: parse_header(main_text), if at
    hand."""
    ext_text = re.sub(r'^[ \t]*#include\s+"pcs\.h"[ \t]*$', "", ext_text, flags=re.M)
    consts, structs, functions = main or parse_header(main_text)
    c2, s2, f2 = parse_header(main_text + "\n" + ext_text)
    if c2 != consts or s2 != structs or f2[:len(functions)] != functions:
        _fail("an extension header may only add functions", ext_text)
    return f2[len(functions):]


_ext_functions, _dense_functions, _fold_functions = [], [], []
for _hs, _into in ((EXT_HEADERS, _ext_functions), (DENSE_HEADERS, _dense_functions), (FOLD_HEADERS, _fold_functions)):
    for _h in _hs:
        with open(HEADER_PATH) as _f, open(os.path.join(os.path.dirname(HEADER_PATH), _h)) as _g:
            _into += parse_extension(_f.read(), _g.read(), (_consts, _structs, _functions))
# F32, BF16, FP8, PRO_*, EPI_*, FLAG_*, HEAD_*, EINVAL, ... and ABI_VERSION (the struct layouts' version)
globals().update(_consts)
# GemmArgs, WgradArgs, Seg12Args, Conv3dGeom, PoolBwdArgs, HeadArgs; (name, restype, argtypes) of
# every function the header declares
_classes, _signatures, _PARAMS = _bind(_structs, _functions + _ext_functions + _dense_functions + _fold_functions)
_n, _m = len(_functions), len(_functions) + len(_ext_functions)
_d = _m + len(_dense_functions)
SIGNATURES, EXT_SIGNATURES, DENSE_SIGNATURES = _signatures[:_n], _signatures[_n:_m], _signatures[_m:_d]
FOLD_SIGNATURES = _signatures[_d:]
globals().update({c.__name__: c for c in _classes.values()})

_lib = None


class PcsError(RuntimeError):
    pass


def load():
    """Load libpcs.so (raises ImportError with build instructions when absent)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("PCS_LIB", LIB_PATH)   # an alternative build, for A/B timing
    if not os.path.exists(path):
        raise ImportError(
            f"pcs_amd HIP library not built: {path} is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C point-cloud-cnn-segmentation_amd/csrc`.")
    lib = ct.CDLL(path)
    for name, res, args in SIGNATURES + EXT_SIGNATURES + DENSE_SIGNATURES + FOLD_SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    got = lib.pcs_abi_version()
    if got != ABI_VERSION:   # the struct classes mirror one layout of include/pcs.h
        raise ImportError(f"{path} has C ABI version {got}, this binding expects {ABI_VERSION}: rebuild it "
                          "(`make -C point-cloud-cnn-segmentation_amd/csrc`)")
    _lib = lib
    return lib


_PLAIN = frozenset([int, float, type(None)])


def _refuse(name, i, a):
    pname, ctext, dtypes, struct = _PARAMS[name][i]
    if isinstance(a, ct.Structure):
        got = f"a {type(a).__name__}"
    elif dtypes is None:
        got = "a tensor"
    elif dtypes and a.dtype not in dtypes:
        got = f"a {a.dtype} tensor"
    else:
        got = f"a tensor on {a.device}, not on a HIP device"
    raise TypeError(f"{name}: {pname} is {ctext}, got {got}")


def _convert(name, args):
    """args as the library takes them: a tensor becomes its data_ptr() once its dtype fits the
    header's pointee type and it lives on a HIP device, a struct is passed by reference; None,
    numbers and ctypes objects pass through."""
    params = _PARAMS[name]
    if len(args) != len(params):
        raise TypeError(f"{name} takes {len(params)} arguments ({', '.join(p[0] for p in params)}), got {len(args)}")
    out = list(args)
    for i, a in enumerate(args):
        if type(a) in _PLAIN:   # (first: isinstance on torch.Tensor is the slow test, and call is on the launch path)
            continue
        if isinstance(a, torch.Tensor):
            dtypes = params[i][2]
            if dtypes is None or (dtypes and a.dtype not in dtypes) or not a.is_cuda:
                _refuse(name, i, a)
            out[i] = a.data_ptr()
        elif isinstance(a, ct.Structure):
            if type(a) is not params[i][3]:
                _refuse(name, i, a)
            out[i] = ct.byref(a)
    return out


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*_convert(name, args))
    if rc < 0:
        raise PcsError(f"{name} failed ({rc}): {lib.pcs_last_error().decode()}")
    return rc


def forward_call(name, args, epi, stream):
    """A forward convolution or its folded twin: name(*args, stream), or with epi = (scale, shift, R, relu)
    name_affine(*args, *epi, stream).  A one-liner for all seven pairs of include/pcs_fold.h because each
    twin takes its twin's arguments, then the epilogue, then the stream, which
    tests/test_fold_abi.py::test_each_twin_takes_its_twins_arguments_plus_the_epilogue pins."""
    return call(name, *args, stream) if epi is None else call(name + "_affine", *args, *epi, stream)


def workspace(name, *args) -> int:
    """The value of a size query (a *_workspace, *_capacity or *_geometry function); a negative
    return raises PcsError with the library's message."""
    lib = load()
    n = int(getattr(lib, name)(*_convert(name, args)))
    if n < 0:
        raise PcsError(lib.pcs_last_error().decode())
    return n


def dtype_code(dtype, what=None):
    """BF16 / F32 of a storage dtype; ``what`` names the argument in the error."""
    if dtype == torch.bfloat16:
        return BF16
    if dtype == torch.float32:
        return F32
    raise ValueError(f"{what} must be bf16 or fp32, got {dtype}" if what else f"bf16 or fp32 expected, got {dtype}")


def ptr(t):
    """Raw device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def stream_ptr(device=None):
    return torch.cuda.current_stream(device).cuda_stream
