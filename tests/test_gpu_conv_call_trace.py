"""The folded layer is the unfused layer plus an epilogue, call for call (MI355X): fold.conv_bn and the
layer's own forward run the same function, so the library calls of conv_bn(conv, bn, *inputs, residual=r)
are those of conv(*inputs) with the forward entry point renamed + "_affine" and handed (scale, shift, R,
relu) before the stream, plus one pcs_bn_eval_coefs; operand preparation, the torch.cat fall-back, the
pair-list / tile-gather route, the geometry and the Z scratch cannot differ.

pcs_amd._lib.call is replaced by a recorder that keeps, per call, the name, every int / float / None
argument, (dtype, shape) of every tensor and the fields of a Conv3dGeom, and forwards to the real call.
The padding copies are torch ops and are not in the trace.  Geometry and parameters are
tests/test_gpu_fold_layers.py's: sparse grid 16, 2 scenes, occupancy 0.3, on both routes; dense
2 x 6 x 6 x 10 (stencil) and 2 x 8 x 8 x 8 (k = 2, s = 2).  Widths: padded and native single-source
layers, the two-source layers below (fall-back) and at their alignment.  Each case also compares the two
outputs bit for bit (the unfused fp32 output through bn.eval())."""
import ctypes as ct

import pytest
import torch

from test_gpu_fold_layers import DEV, _bits, _bn, _case, _levels, route  # noqa: F401  (route: a fixture)

pytestmark = pytest.mark.gpu
FORWARD = {"pcs_sparse_conv", "pcs_sparse_conv_pairs", "pcs_sparse_conv_rows", "pcs_sparse_conv_cat",
           "pcs_sparse_conv_cat_pairs", "pcs_conv3d", "pcs_conv3d_cat"}


def _describe(a):
    if isinstance(a, torch.Tensor):
        return (a.dtype, tuple(a.shape))
    if isinstance(a, ct.Structure):
        return (type(a).__name__,) + tuple(getattr(a, f) for f, _ in a._fields_)
    assert type(a) in (int, float, type(None)), type(a)
    return a


@pytest.fixture
def trace(monkeypatch):
    """The list the recorder appends (name, described arguments) to; clear it between runs."""
    import pcs_amd._lib as L
    real, calls = L.call, []

    def recorder(name, *args):
        calls.append((name, tuple(_describe(a) for a in args)))
        return real(name, *args)
    monkeypatch.setattr(L, "call", recorder)
    return calls


def _check(trace, kind, cin, cout, entry, align):
    from pcs_amd.fold import conv_bn
    conv, xs, tail, bn_cls, ref = _case(kind, cin, cout, seed=cin * 1000 + cout)
    if tail:                                                       # the pair lists are built on first use: not a layer's call
        sv, link = _levels()
        sv.pairs(), link.down_pairs(), link.up_pairs()
    g = torch.Generator().manual_seed(5)
    bn = _bn(bn_cls, cout, True, g)
    r = torch.randn(ref.shape, generator=g).to(DEV)
    trace.clear()
    with torch.no_grad():
        y32 = conv(*xs, *tail, out_dtype=torch.float32)
    unfused = list(trace)
    trace.clear()
    y = conv_bn(conv, bn, *xs, *tail, residual=r, out_dtype=torch.float32)
    folded = list(trace)
    trace.clear()

    assert [n for n, _ in unfused if n in FORWARD] == [entry], [n for n, _ in unfused]
    assert [n for n, _ in folded].count("pcs_bn_eval_coefs") == 1
    ck = -(-cout // align) * align                                 # the channels the kernel runs, zero-padded
    coef = (torch.float32, (ck,))
    want = [(n + "_affine", a[:-1] + (coef, coef, (torch.float32, tuple(ref.shape[:-1]) + (ck,)), 1) + a[-1:])
            if n in FORWARD else (n, a) for n, a in unfused]
    assert [c for c in folded if c[0] != "pcs_bn_eval_coefs"] == want
    assert not any(n in FORWARD for n, _ in folded)

    bn.eval()
    with torch.no_grad():
        assert torch.equal(_bits(y), _bits(bn(y32, residual=r)))


@pytest.mark.parametrize("route", ["gather", "pairs"], indirect=True)
@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("kind", ["subm", "down"])
def test_sparse_layers(trace, kind, c, route):
    _check(trace, kind, c, c, "pcs_sparse_conv_pairs" if route == "pairs" else "pcs_sparse_conv", 64)


def test_sparse_up_layer(trace):
    _check(trace, "up", 64, 64, "pcs_sparse_conv_rows", 64)


@pytest.mark.parametrize("route", ["gather", "pairs"], indirect=True)
@pytest.mark.parametrize("c", [32, 64])
def test_sparse_two_source_layer(trace, c, route):
    entry = "pcs_sparse_conv" if c == 32 else "pcs_sparse_conv_cat"   # 32: torch.cat and the padded single-source layer
    _check(trace, "subm_cat", c, c, entry + ("_pairs" if route == "pairs" else ""), 64)


@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 128)])
@pytest.mark.parametrize("kind", ["conv3d_stencil", "conv3d_down", "conv_transpose3d"])
def test_dense_layers(trace, kind, cin, cout):
    _check(trace, kind, cin, cout, "pcs_conv3d", 32)


@pytest.mark.parametrize("c", [16, 32])
def test_dense_two_source_layer(trace, c):
    _check(trace, "conv3d_cat", c, c, "pcs_conv3d" if c == 16 else "pcs_conv3d_cat", 32)
