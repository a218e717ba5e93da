"""Host-side argument validation of the sparse BatchNorm entry points (pcs_sparse_bn_geometry,
pcs_sparse_bn_stats, pcs_sparse_bn_apply, pcs_sparse_bn_bwd_reduce, pcs_sparse_bn_bwd_apply): bad
arguments are rejected before any launch and empty problems return without one, so no GPU is
needed."""
import ctypes as ct
import os

import pytest

import pcs_amd.sparse_norm  # noqa: F401  (the layer these entry points serve: no layer, no test)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "point-cloud-cnn-segmentation_amd", "csrc", "libpcs.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built (run __graft_entry__.build())")

BAD_C = (0, -8, 12, 60, 1032)          # with bf16 on either side
BAD_C_F32 = (0, -8, 2, 6, 63, 1028)    # fp32 on both sides: C % 4, C <= 1024
EINVAL = -1000


def _lib():
    import pcs_amd._lib as L
    return L, L.load()


def _geometry(lib, V, C=64):
    nb = ct.c_int32(-7)
    rpb = lib.pcs_sparse_bn_geometry(V, C, ct.byref(nb))
    return rpb, nb.value


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 3000, 131072, 131073, 1373184])
def test_geometry_contract(V):
    _, lib = _lib()
    rpb, nb = _geometry(lib, V)
    assert rpb == max(64, 64 * -(-V // (64 * 2048)))
    assert nb == -(-V // rpb) and 1 <= nb <= 2048
    assert (nb - 1) * rpb < V <= nb * rpb          # every row in a block, no block empty


def test_geometry_rejects_bad_arguments():
    _, lib = _lib()
    assert lib.pcs_sparse_bn_geometry(10, 64, None) == EINVAL
    assert b"pcs_sparse_bn_geometry" in lib.pcs_last_error()
    assert _geometry(lib, -1)[0] == EINVAL
    for C in (0, -8, 6, 1032):                     # it takes no dtype: the fp32 rule
        assert _geometry(lib, 10, C)[0] == EINVAL, C
    assert b"pcs_sparse_bn_geometry" in lib.pcs_last_error()
    assert _geometry(lib, 0) == (64, 0)            # an empty level: no block


def _check_entry(L, lib, name, fn, pointers, two_sided=True):
    """The rules every launching entry point shares.  fn(**overrides) calls it with valid defaults, so
    every call here overrides one of them with something invalid (a valid call would launch)."""
    here = name.encode()
    assert fn(V=0, **{p: None for p in pointers}) == 0                       # no row: no launch
    for p in pointers:
        assert fn(**{p: None}) == EINVAL, p
        assert here in lib.pcs_last_error() and b"NULL" in lib.pcs_last_error()
    assert fn(V=-1) == EINVAL
    assert here in lib.pcs_last_error()
    for C in BAD_C:
        for kw in ({}, {"xdt": L.F32}, {"ydt": L.F32}) if two_sided else ({},):
            assert fn(C=C, **kw) == EINVAL, (C, kw)
        assert b"C %" in lib.pcs_last_error() and here in lib.pcs_last_error()
    for C in BAD_C_F32:
        assert fn(C=C, xdt=L.F32, ydt=L.F32) == EINVAL, C
    for bad in (L.FP8, 7, -1):
        assert fn(xdt=bad) == EINVAL
        if two_sided:
            assert fn(ydt=bad) == EINVAL
        assert b"dtype" in lib.pcs_last_error() and here in lib.pcs_last_error()


def _check_blocks(lib, name, fn):
    """A geometry with an empty block, or one that misses rows, is refused."""
    for V, nb, rpb in ((100, 3, 64), (128, 3, 64), (100, 1, 64), (100, 0, 64), (100, 2, 0), (100, -1, 64),
                       (65, 1, 64), (3000, 48, 64), (3000, 46, 64)):
        assert fn(V=V, nb=nb, rpb=rpb) == EINVAL, (V, nb, rpb)
        assert name.encode() in lib.pcs_last_error()


def test_stats_rejects_bad_arguments():
    L, lib = _lib()

    def stats(X=1, xdt=None, ydt=None, V=100, C=64, nb=2, rpb=64, stats=1):
        return lib.pcs_sparse_bn_stats(X, L.BF16 if xdt is None else xdt, V, C, nb, rpb, stats, None)

    _check_entry(L, lib, "pcs_sparse_bn_stats", stats, ("X", "stats"), two_sided=False)   # one dtype: ydt is unused
    _check_blocks(lib, "pcs_sparse_bn_stats", stats)


def test_apply_rejects_bad_arguments():
    L, lib = _lib()

    def apply(X=1, xdt=None, R=1, scale=1, shift=1, relu=1, V=100, C=64, Y=1, ydt=None):
        return lib.pcs_sparse_bn_apply(X, L.BF16 if xdt is None else xdt, R, scale, shift, relu, V, C, Y,
                                       L.BF16 if ydt is None else ydt, None)

    _check_entry(L, lib, "pcs_sparse_bn_apply", apply, ("X", "scale", "shift", "Y"))
    assert apply(X=None, R=None, scale=None, shift=None, Y=None, V=0, C=4, xdt=L.F32, ydt=L.F32) == 0


def test_bwd_reduce_rejects_bad_arguments():
    L, lib = _lib()

    def reduce(dY=1, Y=1, ydt=None, X=1, xdt=None, mean=1, rstd=1, relu=1, V=100, C=64, nb=2, rpb=64, DZ=1, stats=1):
        return lib.pcs_sparse_bn_bwd_reduce(dY, Y, L.BF16 if ydt is None else ydt, X, L.BF16 if xdt is None else xdt,
                                            mean, rstd, relu, V, C, nb, rpb, DZ, stats, None)

    # with relu the stored output (the gate) and DZ are required too
    _check_entry(L, lib, "pcs_sparse_bn_bwd_reduce", reduce, ("dY", "Y", "X", "mean", "rstd", "DZ", "stats"))
    for p in ("dY", "X", "mean", "rstd", "stats"):
        assert reduce(relu=0, Y=None, DZ=None, **{p: None}) == EINVAL, p
    _check_blocks(lib, "pcs_sparse_bn_bwd_reduce", reduce)
    _check_blocks(lib, "pcs_sparse_bn_bwd_reduce", lambda **kw: reduce(relu=0, Y=None, DZ=None, **kw))


def test_bwd_apply_rejects_bad_arguments():
    L, lib = _lib()

    def apply(DZ=1, ydt=None, X=1, xdt=None, alpha=1, beta_c=1, gamma_c=1, V=100, C=64, dX=1):
        return lib.pcs_sparse_bn_bwd_apply(DZ, L.BF16 if ydt is None else ydt, X, L.BF16 if xdt is None else xdt, alpha,
                                           beta_c, gamma_c, V, C, dX, None)

    _check_entry(L, lib, "pcs_sparse_bn_bwd_apply", apply, ("DZ", "X", "alpha", "beta_c", "gamma_c", "dX"))
