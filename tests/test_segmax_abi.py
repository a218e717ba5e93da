"""Host-side argument validation of the segmented-max entry points (csrc/segmax.hip and the max lift
of csrc/pointhead.hip): bad arguments are rejected with -1000 and a message naming the entry point
before any launch, and empty problems return without one, so no GPU is needed."""
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "point-cloud-cnn-segmentation_amd", "csrc", "libpcs.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built (run __graft_entry__.build())")

P = 4096   # a non-NULL, 16-byte aligned pointer value; never dereferenced on the host
BIG = 1 << 40


def _lib():
    import pcs_amd._lib as L
    return L, L.load()


SNAPSHOT = os.path.join(REPO, "tests", "golden", "abi_tables_segmax.json")
NAMES = ("pcs_rows_segmax", "pcs_rows_argselect", "pcs_point_lift_max", "pcs_point_lift_max_bwd",
         "pcs_point_lift_max_bwd_workspace")


def test_symbols_are_bound_and_abi_version_stays():
    """The entry points are declared in include/pcs_segmax.h, an extension beside pcs.h: the binding
    keeps them in EXT_SIGNATURES, pcs.h's own tables and PCS_ABI_VERSION are as they were."""
    L, lib = _lib()
    assert {n for n, _, _ in L.EXT_SIGNATURES} == set(NAMES)
    assert not {n for n, _, _ in L.SIGNATURES} & set(NAMES)
    for n in NAMES:
        fn = getattr(lib, n)
        assert fn.argtypes is not None and len(fn.argtypes) == len(L._PARAMS[n]), n
    assert lib.pcs_abi_version() == 3 == L.ABI_VERSION


def _type_name(t):
    import ctypes as ct
    if isinstance(t, type) and issubclass(t, ct._Pointer):
        return f"POINTER({t._type_.__name__})"
    return t.__name__


def _tables(L):
    return {n: [_type_name(res), [_type_name(a) for a in args]] for n, res, args in L.EXT_SIGNATURES}


def test_extension_tables_equal_the_recorded_snapshot():
    """What the binding derives from include/pcs_segmax.h against tests/golden/abi_tables_segmax.json, in
    the form of tests/golden/abi_tables.json's functions: a change is a reviewable data diff
    (regenerate with `python tests/test_segmax_abi.py`)."""
    import json
    import pcs_amd._lib as L
    assert _tables(L) == json.load(open(SNAPSHOT))


def test_extension_header_is_c99_and_adds_functions_only(tmp_path):
    import shutil
    import subprocess
    import pcs_amd._lib as L
    inc = os.path.join(REPO, "include")
    main, ext = open(os.path.join(inc, "pcs.h")).read(), open(os.path.join(inc, "pcs_segmax.h")).read()
    assert [f[0] for f in L.parse_extension(main, ext)] == [n for n, _, _ in L.EXT_SIGNATURES]
    with pytest.raises(ImportError, match="only add functions"):
        L.parse_extension(main, ext + "\n#define PCS_EXTRA 1\n")
    cc = shutil.which("cc")
    if cc is not None:   # (tests/test_lib_abi.py compiles pcs.h the same way)
        src = tmp_path / "ext.c"
        src.write_text('#include "pcs_segmax.h"\nint main(void) { return pcs_rows_segmax == 0; }\n')
        subprocess.run([cc, "-std=c99", "-fsyntax-only", "-I", inc, str(src)], check=True)


def test_python_names_are_exported():
    import pcs_amd
    for n in ("segment_max", "voxel_max", "sparse_max_pool", "SparseMaxPool3d", "point_lift_max"):
        assert callable(getattr(pcs_amd, n)), n


def test_segmax_rejects_bad_arguments():
    L, lib = _lib()

    def segmax(X=P, xdt=None, src=P, seg_off=P, M=10, C=64, Y=P, ydt=None, arg=P):
        return lib.pcs_rows_segmax(X, L.BF16 if xdt is None else xdt, src, seg_off, M, C, Y, L.BF16 if ydt is None else ydt,
                                   arg, None)

    for null in ("X", "seg_off", "Y"):
        assert segmax(**{null: None}) == -1000, null
    assert b"pcs_rows_segmax" in lib.pcs_last_error() and b"NULL" in lib.pcs_last_error()
    assert segmax(M=-1) == -1000 and b"M >= 0" in lib.pcs_last_error()
    for C in (0, -8, 4, 12, 60):
        assert segmax(C=C) == -1000 and segmax(C=C, xdt=L.F32) == -1000 and segmax(C=C, ydt=L.F32) == -1000
    assert b"C %" in lib.pcs_last_error()
    for C in (0, 2, 6, 10):                                          # fp32 on both sides: a multiple of 4
        assert segmax(C=C, xdt=L.F32, ydt=L.F32) == -1000
    assert segmax(xdt=L.FP8) == -1000 and segmax(ydt=7) == -1000
    assert b"dtype" in lib.pcs_last_error()
    assert segmax(X=None, src=None, seg_off=None, Y=None, arg=None, M=0) == 0   # no launch


def test_argselect_rejects_bad_arguments():
    L, lib = _lib()

    def select(dY=P, ddt=None, arg=P, seg_of=P, R=10, C=64, dX=P, xdt=None):
        return lib.pcs_rows_argselect(dY, L.BF16 if ddt is None else ddt, arg, seg_of, R, C, dX,
                                      L.BF16 if xdt is None else xdt, None)

    for null in ("dY", "arg", "seg_of", "dX"):
        assert select(**{null: None}) == -1000, null
    assert b"pcs_rows_argselect" in lib.pcs_last_error() and b"NULL" in lib.pcs_last_error()
    assert select(R=-1) == -1000 and select(R=1 << 31) == -1000
    assert b"R" in lib.pcs_last_error()
    for C in (0, -8, 4, 12, 60):
        assert select(C=C) == -1000 and select(C=C, ddt=L.F32) == -1000
    assert b"C %" in lib.pcs_last_error()
    assert select(C=6, ddt=L.F32, xdt=L.F32) == -1000
    assert select(ddt=L.FP8) == -1000 and select(xdt=-1) == -1000
    assert b"dtype" in lib.pcs_last_error()
    assert select(dY=None, arg=None, seg_of=None, dX=None, R=0) == 0


def test_lift_max_rejects_bad_arguments():
    L, lib = _lib()

    def lift(Pt=P, ldp=4, Cin=4, W=P, bias=P, order=P, seg_off=P, V=10, C=64, Y=P, ydt=None):
        return lib.pcs_point_lift_max(Pt, ldp, Cin, W, bias, order, seg_off, V, C, Y, L.BF16 if ydt is None else ydt, None)

    for null in ("Pt", "W", "order", "seg_off", "Y"):
        assert lift(**{null: None}) == -1000, null
    assert b"pcs_point_lift_max" in lib.pcs_last_error() and b"NULL" in lib.pcs_last_error()
    for Cin in (0, 9, -1):
        assert lift(Cin=Cin, ldp=16) == -1000
    assert b"Cin" in lib.pcs_last_error()
    assert lift(ldp=3) == -1000 and b"ldp" in lib.pcs_last_error()
    for C in (0, -8, 4, 12, 60, 1032, 2048):
        assert lift(C=C) == -1000 and lift(C=C, ydt=L.F32) == -1000
    assert b"C %" in lib.pcs_last_error()
    assert lift(ydt=L.FP8) == -1000 and lift(ydt=7) == -1000
    assert b"dtype" in lib.pcs_last_error()
    assert lift(V=-1) == -1000
    assert lift(Pt=None, W=None, bias=None, order=None, seg_off=None, Y=None, V=0) == 0


def test_lift_max_bwd_rejects_bad_arguments():
    L, lib = _lib()

    def bwd(dV=P, dt=None, Pt=P, ldp=4, Cin=4, W=P, bias=P, order=P, seg_off=P, V=10, C=64, ws=P, nbytes=BIG, dW=P, db=P):
        return lib.pcs_point_lift_max_bwd(dV, L.BF16 if dt is None else dt, Pt, ldp, Cin, W, bias, order, seg_off, V, C, ws,
                                          nbytes, dW, db, None)

    for null in ("dV", "Pt", "W", "order", "seg_off", "dW", "ws"):
        assert bwd(**{null: None}) == -1000, null
    assert b"pcs_point_lift_max_bwd" in lib.pcs_last_error()
    for Cin in (0, 9):
        assert bwd(Cin=Cin, ldp=16) == -1000
    assert bwd(ldp=2) == -1000
    for C in (0, 4, 60, 1032):
        assert bwd(C=C) == -1000
    assert bwd(dt=L.FP8) == -1000 and bwd(dt=-1) == -1000
    assert bwd(V=-1) == -1000
    for V, C, Cin in ((10, 64, 4), (3000, 96, 8), (1 << 21, 64, 4)):
        need = lib.pcs_point_lift_max_bwd_workspace(V, C, Cin)
        blocks = need // (4 * (C * Cin + C))
        assert need > 0 and need % (4 * (C * Cin + C)) == 0 and 1 <= blocks <= 2048
        assert bwd(V=V, C=C, Cin=Cin, ldp=8, nbytes=need - 1) == -1000
        assert b"workspace" in lib.pcs_last_error()
    assert bwd(ws=P + 4) == -1000                                      # not 16-byte aligned
    assert lib.pcs_point_lift_max_bwd_workspace(0, 64, 4) == 0
    for bad in ((-1, 64, 4), (10, 60, 4), (10, 64, 0), (10, 64, 9), (10, 2048, 4)):
        assert lib.pcs_point_lift_max_bwd_workspace(*bad) == -1000, bad
    assert b"pcs_point_lift_max_bwd_workspace" in lib.pcs_last_error()
    assert bwd(dV=None, Pt=None, W=None, order=None, seg_off=None, dW=None, db=None, ws=None, nbytes=0, V=0) == 0


if __name__ == "__main__":   # regenerate the snapshot from include/pcs_segmax.h as _lib.py reads it
    import json
    import sys
    sys.path.insert(0, REPO)
    import pcs_amd._lib as L
    with open(SNAPSHOT, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(_tables(L).items())) + "\n}\n")
