"""The two-source submanifold convolution (sparse.submanifold_conv3d_cat, SubMConv3dCat; the
pcs_sparse_conv_cat* entry points) on MI355X.  The layer reads [xa | xb] in the concatenated
layer's k-step order, so the layer test is tolerance-free: every output and gradient is torch.equal
to submanifold_conv3d on torch.cat([xa, xb], 1).  The entry points themselves are compared with the
fp64 numpy statement tests/sparse_cat_refs.py on hand-made maps (bounds: 1e-5 norm-relative for
fp32 stores and fp32 gradients, 8e-3 for bf16 stores, as tests/test_gpu_sparse_kst32.py)."""
import ctypes as ct

import numpy as np
import pytest
import torch

import sparse_cat_refs as refs
from pcs_amd.sparse import SubMConv3dCat, submanifold_conv3d_cat

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
BF, F32 = torch.bfloat16, torch.float32
SHAPES = [(64, 128, 64), (128, 64, 128)]   # unequal sources; CB = 128: two k-steps; Cout = 128: two column tiles


@pytest.fixture(params=["gather", "pairs", "default"])
def conv_path(request, monkeypatch):
    """tests/test_gpu_sparse.py's fixture: the tile gather, the pair lists (here at every width, so
    the pair-list weight gradient runs on these layers too), and the module's own mix."""
    import pcs_amd.sparse as S
    if request.param != "default":
        monkeypatch.setattr(S, "PAIR_TAPS_MAX", 0.0 if request.param == "gather" else 27.0)
        monkeypatch.setattr(S, "PAIR_WGRAD", request.param == "pairs")
        monkeypatch.setattr(S, "PAIR_WGRAD_MAX_CH2", 1 << 30)
    return request.param


_LEVELS = {}


def _level(grid, occupancy):
    """The occupied voxels of two jittered scenes (the geometry of tests/test_gpu_point_voxel.py's
    _clouds(seed, 2, grid, occupancy)), built once per geometry."""
    if (grid, occupancy) not in _LEVELS:
        from pcs_amd.data import jittered_clouds, ragged_collate
        from pcs_amd.sparse import sparse_voxels
        from pcs_amd.voxel import voxelize
        clouds = jittered_clouds(21 + grid, 2, grid=grid, occupancy=occupancy, per_voxel=3)
        rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])
        _LEVELS[(grid, occupancy)] = sparse_voxels(rb, voxelize(rb, grid, LO, HI), LO, HI)
    return _LEVELS[(grid, occupancy)]


def _operands(V, ca, cb, cout, seed):
    """Seeded bf16-exact operands on the device: xa, xb, weight [Cout, CA + CB, 3, 3, 3] fp32, bias, dy."""
    g = torch.Generator().manual_seed(seed)
    xa = torch.randn(V, ca, generator=g).to(BF)
    xb = torch.randn(V, cb, generator=g).to(BF)
    w = (torch.randn(cout, ca + cb, 3, 3, 3, generator=g) * 0.05).to(BF).float()
    b = (torch.randn(cout, generator=g) * 0.1).to(BF).float()
    dy = torch.randn(V, cout, generator=g).to(BF)
    return [t.to(DEV) for t in (xa, xb, w, b, dy)]


def _run_cat(sv, xa, xb, w, b, dy, out_dtype, need=(True, True, True)):
    """(y, dxa, dxb, dw, db) of the two-source layer; need = which of (xa, xb, weights) take a gradient."""
    xa, xb = xa.clone().requires_grad_(need[0]), xb.clone().requires_grad_(need[1])
    w = w.clone().requires_grad_(need[2])
    b = None if b is None else b.clone().requires_grad_(need[2])
    y = submanifold_conv3d_cat(xa, xb, w, sv, b, out_dtype)
    y.backward(dy.to(out_dtype))
    return y.detach(), xa.grad, xb.grad, w.grad, None if b is None else b.grad


def _run_concatenated(sv, xa, xb, w, b, dy, out_dtype):
    from pcs_amd.sparse import submanifold_conv3d
    ca = xa.shape[1]
    x = torch.cat([xa, xb], 1).requires_grad_()
    w, b = w.clone().requires_grad_(), b.clone().requires_grad_()
    y = submanifold_conv3d(x, w, sv, b, out_dtype)
    y.backward(dy.to(out_dtype))
    return y.detach(), x.grad[:, :ca], x.grad[:, ca:], w.grad, b.grad


@pytest.mark.parametrize("ca,cb,cout", SHAPES)
@pytest.mark.parametrize("grid,occupancy", [(16, 0.3), (32, 0.05)])
def test_bit_identical_to_the_concatenated_layer(grid, occupancy, ca, cb, cout, conv_path):
    sv = _level(grid, occupancy)
    ops = _operands(sv.num_voxels, ca, cb, cout, ca + cout + grid)
    if conv_path != "default":
        assert sv.use_pairs() == (conv_path == "pairs")
    for out_dtype in (BF, F32):
        got = _run_cat(sv, *ops, out_dtype)
        ref = _run_concatenated(sv, *ops, out_dtype)
        assert got[0].dtype == out_dtype and got[0].shape == (sv.num_voxels, cout)
        for name, a, r in zip(("y", "dxa", "dxb", "dW", "db"), got, ref):
            assert a.shape == r.shape and a.dtype == r.dtype, name
            assert torch.equal(a, r), (name, out_dtype, float((a.float() - r.float()).abs().max()))
        assert got[3].abs().max() > 0 and got[1].abs().max() > 0 and got[2].abs().max() > 0


def test_autograd_keeps_the_sources_not_their_concatenation(conv_path):
    sv = _level(16, 0.3)
    xa, xb, w, b, _ = _operands(sv.num_voxels, 64, 128, 64, 3)
    xa.requires_grad_()
    y = submanifold_conv3d_cat(xa, xb, w.requires_grad_(), sv, b)
    saved = y.grad_fn.saved_tensors
    assert any(t.data_ptr() == xa.data_ptr() for t in saved) and any(t.data_ptr() == xb.data_ptr() for t in saved)
    assert all(tuple(t.shape) != (sv.num_voxels, 192) for t in saved)


@pytest.mark.parametrize("need", [(True, False, False), (False, True, False), (False, False, True)],
                         ids=["xa", "xb", "weights"])
def test_needs_input_grad(need, conv_path):
    """Only xa, only xb, only the weights: None elsewhere, values bit-equal to the full run."""
    sv = _level(16, 0.3)
    ops = _operands(sv.num_voxels, 64, 128, 64, 7)
    full = _run_cat(sv, *ops, BF)
    part = _run_cat(sv, *ops, BF, need=need)
    assert torch.equal(part[0], full[0])
    wanted = (need[0], need[1], need[2], need[2])
    for name, a, r, want in zip(("dxa", "dxb", "dW", "db"), part[1:], full[1:], wanted):
        if want:
            assert a is not None and torch.equal(a, r), name
        else:
            assert a is None, name


def test_deterministic(conv_path):
    sv = _level(32, 0.05)
    ops = _operands(sv.num_voxels, 128, 64, 128, 9)
    first, second = _run_cat(sv, *ops, BF), _run_cat(sv, *ops, BF)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def _rel(a, r):
    r = torch.as_tensor(r)
    return float((a.double().cpu() - r).abs().max() / r.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("ca,cb", [(48, 64)])
def test_off_multiple_widths_take_the_documented_fallback(ca, cb, conv_path):
    """(CA, CB) = (48, 64): torch.cat + submanifold_conv3d (zero-padded there), within the fp64 bounds."""
    sv = _level(16, 0.3)
    xa, xb, w, b, dy = _operands(sv.num_voxels, ca, cb, 64, 13)
    y, dxa, dxb, dw, db = _run_cat(sv, xa, xb, w, b, dy, F32)
    nbr = sv.nbr.cpu().numpy()
    wk = w.permute(0, 2, 3, 4, 1).reshape(64, 27, ca + cb).cpu().numpy()
    f = lambda t: t.float().cpu().numpy()   # noqa: E731
    assert _rel(y, refs.conv_cat(nbr, f(xa), f(xb), wk, f(b))) < 1e-5
    ra, rb_ = refs.dgrad_cat(nbr, f(dy), wk, ca)           # the centred map: the gather with W^T, flipped
    assert dxa.shape == (sv.num_voxels, ca) and dxb.shape == (sv.num_voxels, cb)
    assert _rel(dxa, ra) < 8e-3 and _rel(dxb, rb_) < 8e-3  # input gradients are stored in bf16
    rw, rdb = refs.wgrad_cat(nbr, f(xa), f(xb), f(dy))
    assert _rel(dw.permute(0, 2, 3, 4, 1).reshape(64, 27, ca + cb), rw) < 1e-5 and _rel(db, rdb) < 1e-5


def test_empty_level():
    """V = 0: empty outputs and input gradients, zero weight and bias gradients, no launch."""
    from pcs_amd.sparse import SparseVoxels
    sv = SparseVoxels(torch.empty(0, dtype=torch.int64, device=DEV), torch.full((2,), -1, dtype=torch.int64, device=DEV),
                      torch.zeros(2, dtype=torch.int32, device=DEV), torch.empty(0, 27, dtype=torch.int32, device=DEV), 16)
    xa, xb, w, b, dy = _operands(0, 64, 128, 64, 1)
    y, dxa, dxb, dw, db = _run_cat(sv, xa, xb, w, b, dy, BF)
    assert y.shape == (0, 64) and dxa.shape == (0, 64) and dxb.shape == (0, 128)
    assert dw.shape == w.shape and not dw.any() and db.shape == b.shape and not db.any()


def test_state_dict_round_trips_with_the_concatenated_layer():
    from pcs_amd.sparse import SubMConv3d
    torch.manual_seed(0)
    cat, one = SubMConv3dCat(64, 128, 64).to(DEV), SubMConv3d(192, 64).to(DEV)
    assert list(cat.state_dict()) == list(one.state_dict()) == ["weight", "bias"]
    assert [tuple(v.shape) for v in cat.state_dict().values()] == [(64, 192, 3, 3, 3), (64,)]
    one.load_state_dict(cat.state_dict())
    back = SubMConv3dCat(64, 128, 64).to(DEV)
    back.load_state_dict(one.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(cat.state_dict().values(), back.state_dict().values()))
    sv = _level(16, 0.3)
    xa, xb, _, _, _ = _operands(sv.num_voxels, 64, 128, 64, 5)
    with torch.no_grad():
        assert torch.equal(back(xa, xb, sv), one(torch.cat([xa, xb], 1), sv))
    assert SubMConv3dCat(64, 64, 64, bias=False).bias is None


def test_bad_inputs_raise_before_any_launch():
    sv = _level(16, 0.3)
    V = sv.num_voxels
    xa, xb, w, b, _ = _operands(V, 64, 128, 64, 2)
    with pytest.raises(ValueError, match="bf16"):
        submanifold_conv3d_cat(xa.float(), xb, w, sv, b)
    with pytest.raises(ValueError, match="bf16"):
        submanifold_conv3d_cat(xa, xb.float(), w, sv, b)
    with pytest.raises(ValueError, match="one row per voxel"):
        submanifold_conv3d_cat(xa[:-1], xb, w, sv, b)
    with pytest.raises(ValueError, match="one row per voxel"):
        submanifold_conv3d_cat(xa, torch.cat([xb, xb[:1]]), w, sv, b)
    with pytest.raises(ValueError, match="input channels"):
        submanifold_conv3d_cat(xa, xb, w[:, :128].contiguous(), sv, b)
    with pytest.raises(ValueError, match="3x3x3"):
        submanifold_conv3d_cat(xa, xb, w[:, :, :2], sv, b)
    with pytest.raises(ValueError, match="SubMConv3dCat"):
        SubMConv3dCat(64, 128, 64).to(DEV)(xb, xa, sv)          # the sources swapped


# ---- the entry points themselves against the fp64 statement, on hand-made maps
def _pairs(nmap):
    from pcs_amd.sparse import _build_pairs
    return _build_pairs(nmap)


def _maps():
    """name -> (int32 map [M, 27], rows of the source arrays): M = 130 (two full 64-row tiles and a
    ragged one; about 80 % empty entries, row 77 all empty), M = 1, and isolated rows (centre tap only)."""
    rng = np.random.default_rng(11)
    big = rng.integers(0, 130, size=(130, 27)).astype(np.int32)
    big[rng.random((130, 27)) < 0.8] = -1
    big[77] = -1
    one = rng.integers(0, 40, size=(1, 27)).astype(np.int32)
    one[0, rng.random(27) < 0.5] = -1
    one[0, 13] = 7
    iso = np.full((70, 27), -1, dtype=np.int32)
    iso[:, 13] = np.arange(70)
    return {"m130": (big, 130), "m1": (one, 40), "isolated": (iso, 70)}


_ABI = {}


def _abi_case(name, ca, cb, cout):
    """The map, its pair lists, bf16-exact operands (host fp32 and device) and the fp64 references
    of one case, built once."""
    key = (name, ca, cb, cout)
    if key not in _ABI:
        nbr, n_in = _maps()[name]
        g = torch.Generator().manual_seed(ca + 2 * cout + n_in)
        xa = torch.randn(n_in, ca, generator=g).to(BF)
        xb = torch.randn(n_in, cb, generator=g).to(BF)
        w = (torch.randn(cout, 27, ca + cb, generator=g) * 0.05).to(BF)
        b = torch.randn(cout, generator=g) * 0.1
        dy_in = torch.randn(n_in, cout, generator=g).to(BF)      # the input gradient gathers dy rows through the map
        dy_out = torch.randn(nbr.shape[0], cout, generator=g).to(BF)
        f = lambda t: t.float().numpy()   # noqa: E731
        ref = {"fwd": {fl: refs.conv_cat(nbr, f(xa), f(xb), f(w), f(b), fl) for fl in (0, 1)},
               "dgrad": {fl: refs.dgrad_cat(nbr, f(dy_in), f(w), ca, fl) for fl in (0, 1)},
               "wgrad": refs.wgrad_cat(nbr, f(xa), f(xb), f(dy_out))}
        nmap = torch.from_numpy(nbr).to(DEV)
        wt = torch.from_numpy(refs.weight_t(f(w))).to(BF)        # exact: a permutation of bf16 values
        _ABI[key] = dict(nbr=nbr, nmap=nmap, pairs=_pairs(nmap), ref=ref,
                         dev=[t.to(DEV).contiguous() for t in (xa, xb, w, b, dy_in, dy_out, wt)])
    return _ABI[key]


@pytest.mark.parametrize("form", ["gather", "pairs"])
@pytest.mark.parametrize("ca,cb,cout", SHAPES)
@pytest.mark.parametrize("name", ["m130", "m1", "isolated"])
def test_entry_points_match_fp64(name, ca, cb, cout, form):
    from pcs_amd import _lib as L
    c = _abi_case(name, ca, cb, cout)
    xa, xb, w, b, dy_in, dy_out, wt = c["dev"]
    nmap, (pin, pout, ppos, tap_off, P) = c["nmap"], c["pairs"]
    M, st, toff = nmap.shape[0], L.stream_ptr(DEV), ct.addressof(tap_off)
    assert P == int((c["nbr"] >= 0).sum())
    nan = lambda *shape, dtype: torch.full(shape, float("nan"), dtype=dtype, device=DEV)   # noqa: E731

    for dtype, code, tol in ((F32, L.F32, 1e-5), (BF, L.BF16, 8e-3)):
        for flip in (0, 1):
            y = nan(M, cout, dtype=dtype)
            dxa, dxb = nan(M, ca, dtype=dtype), nan(M, cb, dtype=dtype)
            if form == "gather":
                L.call("pcs_sparse_conv_cat", L.ptr(nmap), M, 27, L.ptr(xa), ca, L.ptr(xb), cb, L.ptr(w), cout, L.ptr(b),
                       L.ptr(y), code, flip, st)
                L.call("pcs_sparse_conv_cat_dgrad", L.ptr(nmap), M, 27, L.ptr(dy_in), cout, L.ptr(wt), L.ptr(dxa), ca,
                       L.ptr(dxb), cb, code, flip, st)
            else:
                z = torch.empty(max(P, 1), max(cout, ca + cb), dtype=F32, device=DEV)
                L.call("pcs_sparse_conv_cat_pairs", L.ptr(pin), L.ptr(ppos), toff, 27, M, L.ptr(xa), ca, L.ptr(xb), cb,
                       L.ptr(w), cout, L.ptr(b), L.ptr(z), L.ptr(y), code, flip, st)
                L.call("pcs_sparse_conv_cat_dgrad_pairs", L.ptr(pin), L.ptr(ppos), toff, 27, M, L.ptr(dy_in), cout,
                       L.ptr(wt), L.ptr(z), L.ptr(dxa), ca, L.ptr(dxb), cb, code, flip, st)
            ra, rb_ = c["ref"]["dgrad"][flip]
            errs = _rel(y, c["ref"]["fwd"][flip]), _rel(dxa, ra), _rel(dxb, rb_)
            print(f"{name} {form} {dtype} flip {flip}: y {errs[0]:.2e}, dxa {errs[1]:.2e}, dxb {errs[2]:.2e}")
            assert max(errs) < tol, errs
            if name == "m130":                                  # the all-empty row: the bias alone, zero gradients
                assert torch.equal(y[77], b.to(dtype)) and not dxa[77].any() and not dxb[77].any()

    if form == "gather":
        nbytes = L.workspace("pcs_sparse_conv_wgrad_workspace", M, 27, ca + cb, cout)
        entry, head = "pcs_sparse_conv_cat_wgrad", (L.ptr(nmap), M, 27)
    else:
        nbytes = L.workspace("pcs_sparse_conv_wgrad_pairs_workspace", toff, 27, M, ca + cb, cout)
        entry, head = "pcs_sparse_conv_cat_wgrad_pairs", (L.ptr(pin), L.ptr(pout), toff, 27, M)
    ws = torch.empty(nbytes // 4, dtype=F32, device=DEV)
    dw, db = nan(cout, 27, ca + cb, dtype=F32), nan(cout, dtype=F32)
    L.call(entry, *head, L.ptr(xa), ca, L.ptr(xb), cb, L.ptr(dy_out), cout, L.ptr(ws), nbytes, L.ptr(dw), L.ptr(db), st)
    rw, rdb = c["ref"]["wgrad"]
    errs = _rel(dw, rw), _rel(db, rdb)
    print(f"{name} {form}: dW {errs[0]:.2e}, db {errs[1]:.2e}")
    assert max(errs) < 1e-5, errs
    dw2 = nan(cout, 27, ca + cb, dtype=F32)
    L.call(entry, *head, L.ptr(xa), ca, L.ptr(xb), cb, L.ptr(dy_out), cout, L.ptr(ws), nbytes, L.ptr(dw2), None, st)
    assert torch.equal(dw2, dw)                                 # deterministic, and db is optional
