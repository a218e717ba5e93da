"""Host-side argument validation of the two-source sparse convolution's entry points
(pcs_sparse_conv_cat, _cat_dgrad, _cat_wgrad and their pair-list forms): bad arguments return
PCS_EINVAL, with the entry's name in pcs_last_error(), before any launch, and M == 0 returns 0
without one, so no GPU is needed."""
import ctypes as ct
import os

import pytest

from pcs_amd.sparse import SubMConv3dCat, submanifold_conv3d_cat  # noqa: F401  (the layer these entry points serve)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "point-cloud-cnn-segmentation_amd", "csrc", "libpcs.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libpcs.so not built (run __graft_entry__.build())")

EINVAL = -1000
BAD_CH = (0, -64, 32, 96, 100, 1 << 21)
TAPS = 27


def _lib():
    import pcs_amd._lib as L
    return L, L.load()


def _tap_off(taps=TAPS, per_tap=3):
    return (ct.c_int64 * (taps + 1))(*[per_tap * t for t in range(taps + 1)])


def _entries(L, lib):
    """name -> (fn(**overrides) with valid defaults, its pointer arguments, has a dtype, has flip, has a
    workspace).  Pointers default to 1 (non-NULL, never dereferenced: every call here is refused or
    has M == 0); tap_off is a real host array, the library reads it."""
    def ws_gather(k):
        return lib.pcs_sparse_conv_wgrad_workspace(k["M"], k["taps"], k["CA"] + k["CB"], k["Cout"])

    def ws_pairs(k):
        return lib.pcs_sparse_conv_wgrad_pairs_workspace(k["tap_off"], k["taps"], k["M"], k["CA"] + k["CB"], k["Cout"])

    base = dict(M=100, taps=TAPS, CA=64, CB=128, Cout=64, dt=L.BF16, flip=0, nbr=1, XA=1, XB=1, W=1, bias=None, Y=1, dY=1,
                Wt=1, dXA=1, dXB=1, ws=1, nbytes=None, dW=1, db=None, pin=1, ppos=1, pout=1, Z=1, tap_off=None)

    def make(call, ws_fn=None):
        def fn(**over):
            k = dict(base, **over)
            if k["tap_off"] is None and "tap_off" not in over:
                k["tap_off"] = _tap_off(k["taps"] if 1 <= k["taps"] <= 27 else TAPS)
            if ws_fn is not None and k["nbytes"] is None:
                need = ws_fn(k)
                k["nbytes"] = need if need >= 0 else 1 << 40   # (a bad shape is refused whatever the size)
            return call(k)
        return fn

    return {
        "pcs_sparse_conv_cat": (make(lambda k: lib.pcs_sparse_conv_cat(
            k["nbr"], k["M"], k["taps"], k["XA"], k["CA"], k["XB"], k["CB"], k["W"], k["Cout"], k["bias"], k["Y"], k["dt"],
            k["flip"], None)), ("nbr", "XA", "XB", "W", "Y"), True, True, False),
        "pcs_sparse_conv_cat_dgrad": (make(lambda k: lib.pcs_sparse_conv_cat_dgrad(
            k["nbr"], k["M"], k["taps"], k["dY"], k["Cout"], k["Wt"], k["dXA"], k["CA"], k["dXB"], k["CB"], k["dt"],
            k["flip"], None)), ("nbr", "dY", "Wt", "dXA", "dXB"), True, True, False),
        "pcs_sparse_conv_cat_wgrad": (make(lambda k: lib.pcs_sparse_conv_cat_wgrad(
            k["nbr"], k["M"], k["taps"], k["XA"], k["CA"], k["XB"], k["CB"], k["dY"], k["Cout"], k["ws"], k["nbytes"],
            k["dW"], k["db"], None), ws_gather), ("nbr", "XA", "XB", "dY", "ws", "dW"), False, False, True),
        "pcs_sparse_conv_cat_pairs": (make(lambda k: lib.pcs_sparse_conv_cat_pairs(
            k["pin"], k["ppos"], k["tap_off"], k["taps"], k["M"], k["XA"], k["CA"], k["XB"], k["CB"], k["W"], k["Cout"],
            k["bias"], k["Z"], k["Y"], k["dt"], k["flip"], None)),
            ("pin", "ppos", "tap_off", "XA", "XB", "W", "Z", "Y"), True, True, False),
        "pcs_sparse_conv_cat_dgrad_pairs": (make(lambda k: lib.pcs_sparse_conv_cat_dgrad_pairs(
            k["pin"], k["ppos"], k["tap_off"], k["taps"], k["M"], k["dY"], k["Cout"], k["Wt"], k["Z"], k["dXA"], k["CA"],
            k["dXB"], k["CB"], k["dt"], k["flip"], None)),
            ("pin", "ppos", "tap_off", "dY", "Wt", "Z", "dXA", "dXB"), True, True, False),
        "pcs_sparse_conv_cat_wgrad_pairs": (make(lambda k: lib.pcs_sparse_conv_cat_wgrad_pairs(
            k["pin"], k["pout"], k["tap_off"], k["taps"], k["M"], k["XA"], k["CA"], k["XB"], k["CB"], k["dY"], k["Cout"],
            k["ws"], k["nbytes"], k["dW"], k["db"], None), ws_pairs),
            ("pin", "pout", "tap_off", "XA", "XB", "dY", "ws", "dW"), False, False, True),
    }


NAMES = ["pcs_sparse_conv_cat", "pcs_sparse_conv_cat_dgrad", "pcs_sparse_conv_cat_wgrad", "pcs_sparse_conv_cat_pairs",
         "pcs_sparse_conv_cat_dgrad_pairs", "pcs_sparse_conv_cat_wgrad_pairs"]


@pytest.mark.parametrize("name", NAMES)
def test_entry_rejects_bad_arguments(name):
    L, lib = _lib()
    fn, pointers, has_dtype, has_flip, has_ws = _entries(L, lib)[name]
    here = name.encode()

    def refused(**over):
        lib.pcs_sparse_bn_geometry(10, 64, None)            # another entry's name into the error text first
        assert fn(**over) == EINVAL, over
        assert lib.pcs_last_error().startswith(here + b":"), lib.pcs_last_error()

    for p in pointers:
        refused(**{p: None})
    refused(M=-1)
    for bad in BAD_CH:
        refused(CA=bad)
        refused(CB=bad)
        refused(Cout=bad)
    for taps in (0, -1, 28):
        refused(taps=taps)
    if has_dtype:
        for bad in (L.FP8, 7, -1):
            refused(dt=bad)
    if has_flip:
        refused(flip=1, taps=8)                             # the flipped tap order needs the centred 27-tap map
        refused(flip=2)
        refused(flip=-1)
    if has_ws:
        need = None
        for M in (100, 1):
            k = dict(M=M)
            full = (lib.pcs_sparse_conv_wgrad_pairs_workspace(_tap_off(), TAPS, M, 192, 64) if "pairs" in name
                    else lib.pcs_sparse_conv_wgrad_workspace(M, TAPS, 192, 64))
            assert full > 0
            for short in (full - 1, 0, -5):
                refused(nbytes=short, **k)
            need = full
        assert need is not None
    if "pairs" in name:
        dec = _tap_off()
        dec[5] = dec[4] - 1
        refused(tap_off=dec)                                # a pair count below zero
        start = _tap_off()
        start[0] = 1
        refused(tap_off=start)


@pytest.mark.parametrize("name", NAMES)
def test_empty_problem_returns_without_a_launch(name):
    L, lib = _lib()
    fn = _entries(L, lib)[name][0]
    empty = _tap_off(per_tap=0)
    assert fn(M=0, tap_off=empty) == 0
    assert fn(M=0, tap_off=empty, bias=1, db=1) == 0
    if "pairs" in name:                                     # without pairs the pair arrays may be NULL
        assert fn(M=0, tap_off=empty, pin=None, pout=None, Z=None) == 0


def test_abi_version_unchanged():
    L, lib = _lib()
    assert lib.pcs_abi_version() == L.ABI_VERSION == 3
