"""The Cin % 64 == 32 instantiations (32-channel k-steps) of sparse_conv_kernel, pair_gemm_kernel and
pair_rows_kernel on MI355X.  The Python layers pad channels to 64, so only direct calls of
pcs_sparse_conv, pcs_sparse_conv_pairs and pcs_sparse_conv_rows with Cin = 32 reach them.
Reference: fp64 numpy on the same bf16-exact operands,
    y[m] = b + sum_t W[:, tw(t), :] x[nbr[m, t]],  tw(t) = flip ? taps - 1 - t : t."""
import ctypes as ct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CIN, COUT, M = 32, 64, 130   # M: two full 64-row tiles and a ragged one


def _rel(a, r):
    return float((a.double().cpu() - r).abs().max() / r.abs().max().clamp_min(1e-30))


def _operands(taps, n_in, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_in, CIN, generator=g).to(torch.bfloat16)
    w = (torch.randn(COUT, taps, CIN, generator=g) * 0.05).to(torch.bfloat16)
    b = torch.randn(COUT, generator=g) * 0.1
    return x, w, b


def _reference(nbr, x, w, b, flip):
    taps = nbr.shape[1]
    xd, wd = x.double().numpy(), w.double().numpy()
    y = np.tile(b.double().numpy(), (nbr.shape[0], 1))
    for t in range(taps):
        rows = np.nonzero(nbr[:, t] >= 0)[0]
        y[rows] += xd[nbr[rows, t]] @ wd[:, taps - 1 - t if flip else t, :].T
    return torch.from_numpy(y)


def _pairs(nmap):
    """(pair_in, pair_out, pair_pos, tap_off host array) of an int32 [M, taps] device map."""
    from pcs_amd import _lib as L
    (m, taps), st = nmap.shape, L.stream_ptr(DEV)
    nb = int(L.load().pcs_sparse_pairs_workspace(m, taps))
    assert nb > 0
    ws = torch.empty(nb // 4, dtype=torch.int32, device=DEV)
    counts = torch.empty(taps, dtype=torch.int64, device=DEV)
    L.call("pcs_sparse_pairs_count", L.ptr(nmap), m, taps, L.ptr(ws), L.ptr(counts), st)
    tap_off = (ct.c_int64 * (taps + 1))(0, *torch.cumsum(counts, 0).tolist())
    P = int(tap_off[taps])
    pin = torch.empty(max(P, 1), dtype=torch.int32, device=DEV)
    pout = torch.empty(max(P, 1), dtype=torch.int32, device=DEV)
    ppos = torch.empty(m, taps, dtype=torch.int32, device=DEV)
    L.call("pcs_sparse_pairs_build", L.ptr(nmap), m, taps, L.ptr(ws), L.ptr(counts), L.ptr(pin), L.ptr(pout),
           L.ptr(ppos), st)
    return pin, pout, ppos, tap_off


def _gather(nmap, x, w, b, dtype, flip):
    from pcs_amd import _lib as L
    m, taps = nmap.shape
    y = torch.full((m, COUT), float("nan"), dtype=dtype, device=DEV)
    L.call("pcs_sparse_conv", L.ptr(nmap), m, taps, L.ptr(x), CIN, L.ptr(w), COUT, L.ptr(b), L.ptr(y),
           L.BF16 if dtype == torch.bfloat16 else L.F32, flip, L.stream_ptr(DEV))
    return y


_CASE_A = {}


def _case_a():
    """A random 27-tap map (about 80 % empty entries, row 77 all empty), its pair lists, the
    operands on the device and the fp64 references of both tap orders; built once."""
    if not _CASE_A:
        rng = np.random.default_rng(11)
        nbr = rng.integers(0, M, size=(M, 27)).astype(np.int32)
        nbr[rng.random((M, 27)) < 0.8] = -1
        nbr[77] = -1
        x, w, b = _operands(27, M, 5)
        nmap = torch.from_numpy(nbr).to(DEV)
        _CASE_A.update(nbr=nbr, nmap=nmap, pairs=_pairs(nmap), dev=(x.to(DEV), w.to(DEV), b.to(DEV)),
                       ref={f: _reference(nbr, x, w, b, f) for f in (0, 1)})
    return _CASE_A


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 8e-3)], ids=["f32", "bf16"])
@pytest.mark.parametrize("flip", [0, 1])
def test_gather_and_pairs_cin32(flip, dtype, tol):
    from pcs_amd import _lib as L
    c = _case_a()
    x, w, b = c["dev"]
    pin, _, ppos, tap_off = c["pairs"]
    P = int(tap_off[27])
    assert 0 < P == int((c["nbr"] >= 0).sum())

    def pairs():
        y = torch.full((M, COUT), float("nan"), dtype=dtype, device=DEV)
        z = torch.empty(P, COUT, dtype=torch.float32, device=DEV)
        L.call("pcs_sparse_conv_pairs", L.ptr(pin), L.ptr(ppos), ct.addressof(tap_off), 27, M, L.ptr(x), CIN, L.ptr(w),
               COUT, L.ptr(b), L.ptr(z), L.ptr(y), L.BF16 if dtype == torch.bfloat16 else L.F32, flip,
               L.stream_ptr(DEV))
        return y

    yg, yp = _gather(c["nmap"], x, w, b, dtype, flip), pairs()
    assert yg.dtype == dtype and yp.dtype == dtype
    eg, ep, egp = _rel(yg, c["ref"][flip]), _rel(yp, c["ref"][flip]), _rel(yp, yg.double().cpu())
    print(f"flip {flip} {dtype}: gather {eg:.2e}, pairs {ep:.2e}, pairs vs gather {egp:.2e}")
    assert eg < tol and ep < tol
    assert egp < tol
    assert torch.equal(yg[77], b.to(dtype)) and torch.equal(yp[77], b.to(dtype))   # the all-empty row: the bias
    assert torch.equal(_gather(c["nmap"], x, w, b, dtype, flip), yg)
    assert torch.equal(pairs(), yp)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.bfloat16, 8e-3)], ids=["f32", "bf16"])
def test_rows_cin32(dtype, tol):
    """pcs_sparse_conv_rows on a one-hot 8-tap map whose taps have 0, 1, 64 and 65 pairs."""
    from pcs_amd import _lib as L
    counts, n_in = (65, 0, 1, 64, 0, 0, 0, 0), 40
    rng = np.random.default_rng(13)
    tap = rng.permutation(np.repeat(np.arange(8), counts))
    assert len(tap) == M
    nbr = np.full((M, 8), -1, dtype=np.int32)
    nbr[np.arange(M), tap] = rng.integers(0, n_in, size=M)
    x, w, b = _operands(8, n_in, 9)
    ref = _reference(nbr, x, w, b, 0)
    nmap = torch.from_numpy(nbr).to(DEV)
    pin, pout, _, tap_off = _pairs(nmap)
    assert [tap_off[t + 1] - tap_off[t] for t in range(8)] == list(counts)
    x, w, b = x.to(DEV), w.to(DEV), b.to(DEV)

    def rows():
        y = torch.full((M, COUT), float("nan"), dtype=dtype, device=DEV)
        L.call("pcs_sparse_conv_rows", L.ptr(pin), L.ptr(pout), ct.addressof(tap_off), 8, M, L.ptr(x), CIN, L.ptr(w),
               COUT, L.ptr(b), L.ptr(y), L.BF16 if dtype == torch.bfloat16 else L.F32, L.stream_ptr(DEV))
        return y

    yr, yg = rows(), _gather(nmap, x, w, b, dtype, 0)
    er, erg = _rel(yr, ref), _rel(yr, yg.double().cpu())
    print(f"rows {dtype}: {er:.2e}, rows vs gather {erg:.2e}")
    assert yr.dtype == dtype and er < tol
    assert erg < tol
    assert torch.equal(rows(), yr)
