"""CPU-side checks of the C ABI: the library loads and exports every declared symbol."""
import ctypes as ct
import json
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pcs.h")
LIB = os.path.join(REPO, "point-cloud-cnn-segmentation_amd", "csrc", "libpcs.so")
SNAPSHOT = os.path.join(REPO, "tests", "golden", "abi_tables.json")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pcs_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_abi():
    names = declared_functions()
    for n in ["pcs_gemm", "pcs_wgrad", "pcs_head", "pcs_adam", "pcs_bn_fwd_finalize",
              "pcs_bn_bwd_finalize", "pcs_pool_finalize", "pcs_pool_bwd", "pcs_dropout_bits"]:
        assert n in names


@pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built (run __graft_entry__.build())")
def test_library_exports_every_declared_symbol():
    import torch  # noqa: F401  (same HIP runtime as the product path)
    lib = ct.CDLL(LIB)
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing
    lib.pcs_abi_version.restype = ct.c_int
    hdr = open(os.path.join(REPO, "include", "pcs.h")).read()
    want = int(re.search(r"#define PCS_ABI_VERSION (\d+)", hdr).group(1))
    assert lib.pcs_abi_version() == want == 3
    import pcs_amd._lib as L
    assert L.ABI_VERSION == want


def _type_name(t):
    if isinstance(t, type) and issubclass(t, ct._Pointer):
        return f"POINTER({t._type_.__name__})"
    return t.__name__


def abi_tables(L):
    """What a binding module says about the ABI, as plain data: per function the ctypes names of the
    result and of every argument, per struct class its (field, ctypes name) list in order."""
    structs = [c for c in vars(L).values()
               if isinstance(c, type) and issubclass(c, ct.Structure) and c is not ct.Structure]
    return {"abi_version": L.ABI_VERSION,
            "functions": {n: [_type_name(res), [_type_name(a) for a in args]] for n, res, args in L.SIGNATURES},
            "structs": {c.__name__: [[f, _type_name(t)] for f, t in c._fields_] for c in structs}}


def test_derived_tables_equal_the_recorded_snapshot():
    """The tables _lib.py derives from include/pcs.h against tests/golden/abi_tables.json, recorded
    from the hand-written tables they replaced: an ABI change is a reviewable data diff."""
    import pcs_amd._lib as L
    got, want = abi_tables(L), json.load(open(SNAPSHOT))
    assert len(L.SIGNATURES) == len(got["functions"]) and set(got["functions"]) == set(declared_functions())
    diff = [f"{kind}.{k}" for kind in ("functions", "structs")
            for k in sorted(set(got[kind]) | set(want[kind])) if got[kind].get(k) != want[kind].get(k)]
    assert not diff and got == want, (
        f"include/pcs.h no longer gives the recorded ABI tables: {diff or 'abi_version'}.  After adding an entry "
        "point, regenerate the snapshot (`python tests/test_lib_abi.py`) and review its diff; if a struct or an "
        "existing signature changed, bump PCS_ABI_VERSION in include/pcs.h as well.")


def test_struct_layouts_agree_with_a_c_compiler(tmp_path):
    """sizeof and every offsetof of the six argument structs, from a C99 program that includes pcs.h."""
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler (cc) on PATH")
    import pcs_amd._lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    c_names = re.findall(r"typedef\s+struct\s*\{[^{}]*\}\s*(\w+)\s*;", hdr)
    classes = {c: getattr(L, "".join(p.capitalize() for p in c.split("_")[1:])) for c in c_names}
    assert len(classes) == 6
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pcs.h"', 'int main(void) {']
    for c, cls in classes.items():
        lines.append(f'  printf("{c} %zu\\n", sizeof({c}));')
        lines += [f'  printf("{c}.{f} %zu\\n", offsetof({c}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(ln.split() for ln in out.splitlines())
    want = {}
    for c, cls in classes.items():
        want[c] = str(ct.sizeof(cls))
        want.update({f"{c}.{f}": str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert got == want
    assert [want[c] for c in c_names] == ["288", "184", "208", "184", "128", "56"]


@pytest.mark.parametrize("text,names", [
    ("typedef struct ihipStream_t *pcs_stream_t;\nint pcs_f(const double *x, pcs_stream_t stream);", "const double *x"),
    ("int pcs_f(int32_t n);\ntypedef struct { int32_t a; float b;\nint pcs_g(void);", "typedef struct { int32_t a;"),
    ("enum { PCS_A = 1, PCS_B };", "PCS_B"),
    ("int pcs_f(unsigned n);", "unsigned n"),
    ("typedef struct { int32_t a; uint8_t b; } pcs_t;", "uint8_t b"),
    ("#pragma pack(1)\nint pcs_f(void);", "#pragma pack(1)"),
])
def test_parser_refuses_what_it_does_not_know(text, names):
    """An unknown parameter type, an unterminated struct, an enumerator without a value (and an
    unknown scalar, a by-value field of a pointee-only type, an unknown directive): each raises and
    names the offending text; nothing is guessed."""
    import pcs_amd._lib as L
    with pytest.raises(ImportError, match=re.escape(names)):
        L.parse_header(text)


def test_parser_reads_multi_declarator_lines():
    import pcs_amd._lib as L
    consts, structs, functions = L.parse_header(
        "#define PCS_ABI_VERSION 7\nenum { PCS_X = -3, };\n"
        "typedef struct { const void *A, *A2; const uint8_t *m; float k; int64_t n, ld; } pcs_t;\n"
        "int64_t pcs_q(pcs_t *args);")
    assert consts == {"ABI_VERSION": 7, "X": -3}
    assert structs == {"pcs_t": [("A", ct.c_void_p), ("A2", ct.c_void_p), ("m", ct.c_void_p), ("k", ct.c_float),
                                 ("n", ct.c_int64), ("ld", ct.c_int64)]}
    assert functions == [("pcs_q", "int64_t", [("args", "pcs_t", True, False)])]


@pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built")
def test_argument_validation_without_gpu():
    """Invalid arguments are rejected on the host, before any launch (no GPU needed)."""
    import pcs_amd._lib as L
    lib = L.load()
    a = L.GemmArgs(num_scenes=1, scene_rows=128, K=60, Ncols=64, dtype=L.BF16)
    assert lib.pcs_gemm(ct.byref(a), None) == -1000
    assert b"multiple" in lib.pcs_last_error()
    h = L.HeadArgs(num_scenes=1, scene_rows=64, Cin=128, num_classes=40)
    assert lib.pcs_head(ct.byref(h), None) == -1000
    assert lib.pcs_dropout_bits(1, 0, 16, 12, 0.3, None, None) == -1000


@pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built")
def test_geometry_is_scene_aligned():
    import pcs_amd._lib as L
    lib = L.load()
    for N, B in [(4096, 4), (3000, 3), (2097152, 4), (1, 1), (129, 2)]:
        a = L.GemmArgs(num_scenes=B, scene_rows=N, K=64, Ncols=1024, dtype=L.BF16)
        rpc = lib.pcs_gemm_geometry(ct.byref(a))
        assert rpc % 128 == 0 and rpc > 0
        cps = a.chunks_per_scene
        assert (cps - 1) * rpc < N <= cps * rpc      # no empty chunk, full coverage


@pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built")
def test_fused_dgrad_wgrad_validates_shapes_without_gpu():
    import pcs_amd._lib as L
    lib = L.load()
    a = L.WgradArgs(num_scenes=1, scene_rows=128, Cout=256, Cin=64, dtype=L.BF16, dy_mode=L.PRO_RAW,
                    x_mode=L.PRO_BNRELU)
    assert lib.pcs_dgrad_wgrad_folded_workspace(ct.byref(a)) < 0
    a.Cout = 512
    # include/pcs.h: a slab R [512, 64] | G [64, 64] | S [64] per slice, the summed R | G, then
    # S_b [B, 64] and cvec [B, 64], all fp32
    B, slab, rg = 1, 512 * 64 + 64 * 64 + 64, 512 * 64 + 64 * 64
    nbytes = lib.pcs_dgrad_wgrad_folded_workspace(ct.byref(a))
    assert a.splits_per_scene >= 1
    assert nbytes == (B * a.splits_per_scene * slab + rg + 2 * B * 64) * 4


@pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built")
@pytest.mark.parametrize("n,dtype", [(1024, "BF16"), (64, "F32")])
def test_gemm_rejects_removed_prologue_without_gpu(n, dtype):
    """Prologue 3 (a hole in the enum since ABI 3) is refused before any operand is looked at:
    every pointer is NULL, and the error names the prologue, not a missing operand."""
    import pcs_amd._lib as L
    lib = L.load()
    for epi in (L.EPI_RAW, L.EPI_DGRAD):
        a = L.GemmArgs(num_scenes=1, scene_rows=256, K=n, Ncols=n, dtype=getattr(L, dtype), prologue=3,
                       epilogue=epi)
        assert lib.pcs_gemm(ct.byref(a), None) == -1000
        assert b"prologue" in lib.pcs_last_error()


@pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built")
def test_wgrad_rejects_removed_dy_mode_without_gpu():
    import pcs_amd._lib as L
    lib = L.load()
    a = L.WgradArgs(num_scenes=1, scene_rows=128, Cout=64, Cin=64, dtype=L.BF16, dy_mode=3,
                    x_mode=L.PRO_BNRELU)
    assert lib.pcs_wgrad(ct.byref(a), None) == -1000
    assert b"dy_mode" in lib.pcs_last_error()


@pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built")
@pytest.mark.parametrize("field", ["reserved0", "reserved1", "reserved2"])
def test_wgrad_rejects_reserved_fields_without_gpu(field):
    """The three pointer fields removed in ABI 3 keep their place in pcs_wgrad_args; a caller that
    still fills one gets PCS_EINVAL, not a silent no-op."""
    import pcs_amd._lib as L
    lib = L.load()
    a = L.WgradArgs(num_scenes=1, scene_rows=128, Cout=64, Cin=64, dtype=L.BF16, dy_mode=L.PRO_BWD,
                    x_mode=L.PRO_BNRELU)
    assert lib.pcs_wgrad_workspace(ct.byref(a)) > 0
    setattr(a, field, 1)
    a.splits_per_scene = 0
    assert lib.pcs_wgrad_workspace(ct.byref(a)) == -1000
    assert lib.pcs_wgrad(ct.byref(a), None) == -1000


@pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built")
def test_unfolded_dgrad_wgrad_is_not_exported():
    import torch  # noqa: F401  (same HIP runtime as the product path)
    lib = ct.CDLL(LIB)
    assert hasattr(lib, "pcs_dgrad_wgrad_folded") and hasattr(lib, "pcs_dgrad_wgrad_folded_workspace")
    assert not hasattr(lib, "pcs_dgrad_wgrad")
    assert not hasattr(lib, "pcs_dgrad_wgrad_workspace")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built")
def test_conv3d_argument_validation_without_gpu():
    """pcs_conv3d* reject bad geometries on the host, before any launch (no GPU needed)."""
    import pcs_amd._lib as L
    lib = L.load()

    def geom(**kw):
        d = dict(B=1, Di=8, Hi=8, Wi=8, Do=8, Ho=8, Wo=8, Cin=64, Cout=64, k=3, s=1, p=1, transposed=0)
        d.update(kw)
        return L.Conv3dGeom(**d)

    ok = geom()
    assert lib.pcs_conv3d_wgrad_workspace(ct.byref(ok)) > 0
    for bad in (geom(Cin=48), geom(Cout=40), geom(Do=7), geom(k=4), geom(s=3), geom(p=3),
                geom(transposed=1, Do=9)):
        assert lib.pcs_conv3d(ct.byref(bad), 1, 1, None, 1, L.BF16, None) == -1000
    assert lib.pcs_conv3d(ct.byref(ok), 1, 1, None, 1, L.F32 + 7, None) == -1000
    assert lib.pcs_conv3d_wgrad_workspace(ct.byref(geom(Cin=40))) == -1000
    assert lib.pcs_conv3d_wgrad_workspace(ct.byref(geom(Cin=32, Cout=96))) > 0   # 32-channel tiles
    up = geom(Di=4, Hi=4, Wi=4, k=2, s=2, p=0, transposed=1)     # 4^3 -> 8^3
    assert lib.pcs_conv3d_wgrad_workspace(ct.byref(up)) > 0


def test_seg_backward_geometry_without_gpu():
    """seg_conv2 / seg_conv3 backward (pcs_dgrad_wgrad_bn): the four-wave kernel's slices
    (fused_seg4.hip: 16-row steps, one 256-column workgroup per CU)."""
    import pcs_amd._lib as L
    lib = L.load()
    for cout, cin in ((256, 512), (128, 256)):
        for flags, nblk in ((0, cin // 256),):
            a = L.GemmArgs(num_scenes=4, scene_rows=128 ** 3, K=cout, Ncols=cin, dtype=L.BF16,
                           prologue=L.PRO_BWD, epilogue=L.EPI_DGRAD, flags=flags)
            nbytes = lib.pcs_dgrad_wgrad_bn_workspace(ct.byref(a))
            cps = a.chunks_per_scene
            assert nbytes == 4 * cps * cout * cin * 4
            assert cps * 4 * nblk >= 256 and cps * 4 * nblk < 2 * 256   # about one workgroup per CU


@pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built")
def test_sparse_pairs_argument_validation_without_gpu():
    """The pair-list entry points reject bad tap offsets and channel counts on the host, before
    any launch, and size their workspaces from the host tap offsets (no GPU needed)."""
    import pcs_amd._lib as L
    lib = L.load()
    assert lib.pcs_sparse_pairs_workspace(1000, 27) == ((1000 + 255) // 256 * 27 + 1) * 4
    assert lib.pcs_sparse_pairs_workspace(-1, 27) == -1000
    assert lib.pcs_sparse_pairs_workspace(10, 28) == -1000
    good = (ct.c_int64 * 28)(*([0] * 13 + [100] * 15))       # only the centre tap: 100 rows
    ta = ct.addressof(good)
    assert lib.pcs_sparse_conv_wgrad_pairs_workspace(ta, 27, 100, 64, 64) > 0
    assert lib.pcs_sparse_conv_wgrad_pairs_workspace(ta, 27, 100, 32, 64) == -1000   # Cin % 64
    # slices are divided over the 64 x 64 channel tiles: 27 taps x 2^20 pairs keep the workspace
    # near 2048 tiles' partials at every width (a fixed 2048 slices took 544 MB at 256 -> 256)
    V = 1 << 20
    full = (ct.c_int64 * 28)(*[t * V for t in range(28)])
    for ch, lim in ((64, 40 << 20), (128, 48 << 20), (256, 48 << 20)):
        nb = lib.pcs_sparse_conv_wgrad_pairs_workspace(ct.addressof(full), 27, V, ch, ch)
        assert 0 < nb <= lim, (ch, nb)
    bad = (ct.c_int64 * 28)(*([0] * 13 + [100] * 14 + [50]))   # decreasing
    assert lib.pcs_sparse_conv_wgrad_pairs_workspace(ct.addressof(bad), 27, 100, 64, 64) == -1000
    start = (ct.c_int64 * 28)(*([5] + [100] * 27))             # not starting at 0
    assert lib.pcs_sparse_conv_pairs(1, 1, ct.addressof(start), 27, 100, 1, 64, 1, 64, None, 1, 1, L.BF16, 0,
                                     None) == -1000
    assert lib.pcs_sparse_conv_pairs(1, 1, ta, 27, 100, 1, 64, 1, 48, None, 1, 1, L.BF16, 0, None) == -1000   # Cout
    assert lib.pcs_sparse_conv_pairs(1, 1, ta, 27, 100, 1, 64, 1, 64, None, None, 1, L.BF16, 0, None) == -1000   # no Z


def write_snapshot(tables):
    """One line per function and per struct, sorted: a new entry point is one added line."""
    def rows(d):
        return ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(d.items()))
    with open(SNAPSHOT, "w") as f:
        f.write(f'{{\n "abi_version": {tables["abi_version"]},\n "functions": {{\n{rows(tables["functions"])}\n }},\n'
                f' "structs": {{\n{rows(tables["structs"])}\n }}\n}}\n')


if __name__ == "__main__":   # regenerate the snapshot from include/pcs.h as _lib.py reads it
    import sys
    sys.path.insert(0, REPO)
    import pcs_amd._lib as L
    write_snapshot(abi_tables(L))
