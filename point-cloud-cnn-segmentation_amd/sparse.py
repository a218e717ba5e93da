"""Occupied-voxel (sparse) path: the north star's "hash-indexed gather" (BASELINE configs[2],
SURVEY §8 f4).  Build-defined, like the rest of the voxel vocabulary: the reference has no voxel
grid, so parity is against oracle/sparse_oracle.py and against torch's dense conv3d evaluated on
the occupied sites ("not reference parity").

    vb = voxelize(rb, grid=256)                          # pcs_voxelize (voxel.py)
    sv = sparse_voxels(rb, vb)                           # keys, hash table, 27-neighbour map
    conv = SubMConv3d(64, 64)                            # torch Conv3d parameter layout
    y = conv(x, sv)                                      # x: bf16 [V, 64] per-voxel features

A submanifold 3x3x3 convolution: outputs exist only at occupied voxels and read only occupied
neighbours (nbr[v][t], -1 = empty), so an occupied-only network never densifies.  The neighbour
map is built once per voxelisation (pcs_voxel_hash_build + pcs_sparse_neighbors) and shared by
every layer at that resolution, forward and backward (the input gradient is the same gather with
the transposed, tap-flipped weight).

A U-Net changes resolution with the 2x2x2, stride-2 pair, still on occupied voxels only:

    svc, link = coarsen(sv)                              # grid / 2: the occupied 2x2x2 cells
    c = SparseDownConv3d(64, 128)(e, link)               # nn.Conv3d(k=2, s=2) on the fine voxels
    u = SparseUpConv3d(128, 64)(c, link)                 # nn.ConvTranspose3d(k=2, s=2) back to them

The down forward and the up input gradient are the 8-tap gather through link.child (the kernels
above at taps = 8); the up forward and the down input gradient have one tap per output row and
run pcs_sparse_conv_rows, which writes each row once from its own tap's GEMM tile.

The decoder's skip connection convolves (up, skip) without concatenating them:

    m = SubMConv3dCat(64, 64, 64)(u, e, sv)              # == SubMConv3d(128, 64)(torch.cat([u, e], 1), sv)

The kernels read the two arrays as the column blocks of one X operand (pcs_sparse_conv_cat*), in
the concatenated layer's k-step order, so the result is bit-identical to it; no [V, CA + CB]
tensor is written, kept for the backward or sliced into gradients.  sparse_unet.py assembles the
levels (SparsePyramid) and these layers into the occupied-voxel U-Net.
"""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass, field

import torch

from . import _lib as L
from .data import RaggedBatch
from .voxel import (CH_ALIGN, VoxelBatch, _box, _bf16_2d, _conv_operands, _kernel_weight, _layer, _pad_channels, _unpad,
                    _weight_t, _wgrad)

TAPS = 27
K2_TAPS = 8   # the k = 2, s = 2 layers between a level and its coarse level
# forward / input gradient through the pair lists (gather-GEMM-reduce) when the map has at most
# this many occupied taps per voxel; above it the tile-gather kernel, whose zero rows are then few
# and which keeps no per-pair products in memory.  The weight gradient takes the pair lists at
# every occupancy (PAIR_WGRAD) for layers of at most PAIR_WGRAD_MAX_CH2 = Cin x Cout channel
# pairs (64 -> 64, the shape profiles/bench_sparse_pairs_r05.txt measured); wider layers keep
# the tile-gather weight gradient until the pair form is measured there
PAIR_TAPS_MAX = 3.0
PAIR_WGRAD = True
PAIR_WGRAD_MAX_CH2 = 64 * 64


def _build_pairs(nmap: torch.Tensor):
    """Per-tap pair lists of an int32 [M, taps] map (pcs_sparse_pairs_*; one host read of the tap
    counts): (pair_in, pair_out, pair_pos, tap_off, P) with tap_off a host int64 array of
    taps + 1 entries."""
    (M, taps), dev = nmap.shape, nmap.device
    st = L.stream_ptr(dev)
    nb = L.workspace("pcs_sparse_pairs_workspace", M, taps)
    ws =torch.empty(max(nb // 4, 1), dtype=torch.int32, device=dev)
    counts = torch.empty(taps, dtype=torch.int64, device=dev)
    L.call("pcs_sparse_pairs_count", nmap, M, taps, ws, counts, st)
    tap_off = (ct.c_int64 * (taps + 1))(0, *torch.cumsum(counts, 0).tolist())
    P = int(tap_off[taps])
    pin = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    pout = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    ppos = torch.empty(M, taps, dtype=torch.int32, device=dev)
    L.call("pcs_sparse_pairs_build", nmap, M, taps, ws, counts, pin, pout, ppos, st)
    return pin, pout, ppos, tap_off, P


@dataclass
class SparseVoxels:
    keys: torch.Tensor         # int64 [V] (u64 keys: scene * G^3 + (ix * G + iy) * G + iz), ascending
    table_keys: torch.Tensor   # int64 [cap] (u64, all ones = empty)
    table_vals: torch.Tensor   # int32 [cap]
    nbr: torch.Tensor          # int32 [V, 27]
    grid: int
    _pairs: tuple = field(default=None, repr=False)   # (pair_in, pair_out, pair_pos, tap_off host array, P)

    @property
    def num_voxels(self) -> int:
        return self.keys.numel()

    def pairs(self):
        """Per-tap pair lists of the neighbour map, built once (pcs_sparse_pairs_*; one host read of
        the 27 tap counts): (pair_in, pair_out, pair_pos, tap_off, P) with tap_off a host int64
        array of 28 entries."""
        if self._pairs is None:
            self._pairs = _build_pairs(self.nbr)
        return self._pairs

    def use_pairs(self) -> bool:
        """The forward / input gradient form for this map (the pair lists or the tile gather)."""
        return self.num_voxels > 0 and self.pairs()[4] <= PAIR_TAPS_MAX * self.num_voxels

    def find(self, keys: torch.Tensor) -> torch.Tensor:
        """int32 rows of the voxels with these keys (-1: unoccupied), one device lookup each."""
        q = keys.reshape(-1).to(torch.int64).contiguous()
        out = torch.empty(q.numel(), dtype=torch.int32, device=q.device)
        L.call("pcs_voxel_hash_find", self.table_keys, self.table_vals, self.table_keys.numel(), q, q.numel(), out,
               L.stream_ptr(q.device))
        return out


def sparse_from_keys(keys: torch.Tensor, grid: int) -> SparseVoxels:
    """Hash table and neighbour map of the occupied voxels with these keys (int64 [V] on a HIP
    device; unique)."""
    if not keys.is_cuda:
        raise RuntimeError("pcs_amd sparse voxels run on a HIP device only (no CPU fallback)")
    keys = keys.to(torch.int64).contiguous()
    n, dev = keys.numel(), keys.device
    # the open-addressing table keeps one row per key: duplicates (or negative keys, which as
    # uint64 could equal the EMPTY sentinel) would silently alias rows
    if n and (int(keys.min()) < 0 or torch.unique(keys).numel() != n):
        raise ValueError("sparse_from_keys: keys must be unique and non-negative")
    cap = L.workspace("pcs_voxel_hash_capacity", n)
    tk =torch.empty(cap, dtype=torch.int64, device=dev)
    tv = torch.empty(cap, dtype=torch.int32, device=dev)
    st = L.stream_ptr(dev)
    L.call("pcs_voxel_hash_build", keys, n, tk, tv, cap, st)
    nbr = torch.empty(n, TAPS, dtype=torch.int32, device=dev)
    L.call("pcs_sparse_neighbors", tk, tv, cap, keys, n, int(grid), nbr, st)
    return SparseVoxels(keys, tk, tv, nbr, int(grid))


def sparse_voxels(rb: RaggedBatch, vb: VoxelBatch, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)) -> SparseVoxels:
    """The sparse index of a voxelisation (the same points, box and grid as voxelize())."""
    dev = vb.voxel_of_point.device
    pts = rb.points.to(dev, torch.float32).contiguous()
    off = rb.offsets.to(dev, torch.int64).contiguous()
    V = vb.batch.points.shape[0]
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    L.call("pcs_voxel_keys", pts, off, off.numel() - 1, pts.shape[0], int(vb.grid), *_box(lo, hi), vb.voxel_of_point,
           keys, L.stream_ptr(dev))
    return sparse_from_keys(keys, vb.grid)


def _conv_taps(nmap, pairs, x, cin, w, cout, bias, y, ydt, flip=0, epi=None):
    """y[m] = b + sum_t W[tw(t)] x[nmap[m][t]]: through the map's pair lists (pairs; Z = per-pair
    products, fp32) or, with pairs None, in gathered tiles; epi: L.forward_call's."""
    (rows, taps), st = nmap.shape, L.stream_ptr(x.device)
    if pairs is None:
        L.forward_call("pcs_sparse_conv", (nmap, rows, taps, x, cin, w, cout, bias, y, ydt, flip), epi, st)
        return
    pin, _, ppos, tap_off, P = pairs
    z = torch.empty(max(P, 1), cout, dtype=torch.float32, device=x.device)
    L.forward_call("pcs_sparse_conv_pairs", (pin, ppos, ct.addressof(tap_off), taps, rows, x, cin, w, cout, bias, z, y, ydt,
                                             flip), epi, st)


def _sparse_wgrad(nmap, pairs_fn, xk, dyb, cin, cout, has_bias, use_pairs):
    """(dwk, db) of a convolution through nmap [rows_out, taps], un-padded to cin, cout: over the
    map's pair lists (pairs_fn()) or in gathered tiles."""
    (rows, taps), cin_k, cout_k = nmap.shape, xk.shape[1], dyb.shape[1]
    if use_pairs:
        pin, pout, _, tap_off, _ = pairs_fn()
        nbytes = L.workspace("pcs_sparse_conv_wgrad_pairs_workspace", ct.addressof(tap_off), taps, rows, cin_k, cout_k)
        name, head = "pcs_sparse_conv_wgrad_pairs", (pin, pout, ct.addressof(tap_off), taps, rows)
    else:
        nbytes = L.workspace("pcs_sparse_conv_wgrad_workspace", rows, taps, cin_k, cout_k)
        name, head = "pcs_sparse_conv_wgrad", (nmap, rows, taps)
    head += (xk, cin_k, dyb, cout_k)
    return _wgrad(name, head, nbytes, taps, cin, cout, cin_k, cout_k, has_bias, xk.device)


def _sparse_forward(x, wk, bias, at, out_dtype, up=None, epi=None):
    """The forward of every single-source sparse layer, unfused or with the epilogue epi of fold.conv_bn
    (the _affine twins): x bf16 [rows_in, Cin], wk the kernel-layout weight [Cout, taps * Cin] (fp32
    master), at the SparseVoxels of a submanifold layer (up None) or the CoarseLink of a down (up False)
    or up (up True) layer.  The gather runs through the map's pair lists or in tiles, as at.use_pairs()
    says; the up map has one tap per output row and runs pcs_sparse_conv_rows.  Returns (y, xk, wb,
    whether the pair lists carried it): y without the padded channels, and the operands as the kernel
    read them, which the backward keeps."""
    nmap, rows_in = (at.nbr, at.nbr.shape[0]) if up is None else (at.up, at.coarse) if up else (at.child, at.fine)
    taps = TAPS if up is None else K2_TAPS
    if not x.is_cuda:
        raise RuntimeError("pcs_amd sparse conv runs on a HIP device only (no CPU fallback)")
    if x.dtype != torch.bfloat16 or x.dim() != 2 or x.shape[0] != rows_in or nmap.shape[1] != taps:
        raise ValueError("x must be bf16 [V, C] with a [V, 27] neighbour map" if up is None else
                         f"x must be bf16 [{rows_in}, C]: the {'coarse' if up else 'fine'} voxels of the link")
    rows, cin, cout = nmap.shape[0], x.shape[1], wk.shape[0]
    if wk.shape[1] != taps * cin:
        raise ValueError(f"weight has {wk.shape[1] // taps} input channels, x has {cin}")
    xk, wb, bk, cin_k, cout_k = _conv_operands(x, wk, bias, taps, CH_ALIGN)
    epi = epi and epi(cout, cout_k, (rows, cout), x.device)
    y = torch.empty(rows, cout_k, dtype=out_dtype, device=x.device)
    ydt = L.dtype_code(out_dtype, what="out_dtype")
    pairs = False
    if up:
        _conv_rows(at, xk, cin_k, wb, cout_k, bk, y, ydt, epi)
    else:
        pairs = at.use_pairs()
        _conv_taps(nmap, (at.down_pairs() if up is False else at.pairs()) if pairs else None, xk, cin_k, wb, cout_k, bk, y,
                   ydt, 0, epi)
    return _unpad(y, cout), xk, wb, pairs


class _SubMConvFn(torch.autograd.Function):
    """y = b + sum_t W_t x[nbr[:, t]] with w in kernel layout [Cout, 27 * Cin] (fp32 master);
    channel counts off the 64 multiple run zero-padded (exact, as voxel._Conv3dFn)."""

    @staticmethod
    def forward(ctx, x, wk, bias, sv, out_dtype):
        y, xk, wb, ctx.pairs = _sparse_forward(x, wk, bias, sv, out_dtype)
        ctx.save_for_backward(xk, wb, sv.nbr)
        ctx.sv = sv
        ctx.wpairs = PAIR_WGRAD and xk.shape[0] > 0 and xk.shape[1] * wb.shape[0] <= PAIR_WGRAD_MAX_CH2
        ctx.cfg = (bias is not None, x.shape[1], wk.shape[0])
        return y

    @staticmethod
    def backward(ctx, dy):
        xk, wb, nbr = ctx.saved_tensors
        has_bias, cin, cout = ctx.cfg
        V, cin_k = xk.shape
        cout_k = wb.shape[0]
        dyb = _bf16_2d(_pad_channels(dy, cout_k), V, cout_k)
        dx = dwk = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(V, cin_k, dtype=torch.bfloat16, device=xk.device)
            _conv_taps(nbr, ctx.sv.pairs() if ctx.pairs else None, dyb, cout_k, _weight_t(wb, TAPS), cin_k, None, dx,
                       L.BF16, 1)
            if cin_k != cin:
                dx = dx[:, :cin].contiguous()
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            dwk, db = _sparse_wgrad(nbr, ctx.sv.pairs, xk, dyb, cin, cout, has_bias, ctx.wpairs)
        return dx, dwk, db, None, None


def _submanifold_conv3d(x, weight, sv, bias, out_dtype, epi=None):
    """submanifold_conv3d, or (epi) the same layer under fold.conv_bn's epilogue."""
    if tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError("submanifold_conv3d is the 3x3x3 form")
    return _layer(_SubMConvFn, _sparse_forward, epi, x, _kernel_weight(weight), bias, sv, out_dtype)


def submanifold_conv3d(x, weight, sv: SparseVoxels, bias=None, out_dtype=torch.bfloat16):
    """3x3x3 submanifold convolution of per-voxel features x (bf16 [V, Cin]); weight [Cout, Cin,
    3, 3, 3] (torch Conv3d layout, fp32), bias [Cout] or None."""
    return _submanifold_conv3d(x, weight, sv, bias, out_dtype)


class SubMConv3d(torch.nn.Module):
    """Submanifold 3x3x3 convolution on occupied voxels with nn.Conv3d(cin, cout, 3, padding=1)'s
    parameter layout and init: on a dense grid that is zero off the occupied voxels, its output at
    the occupied voxels equals that Conv3d's."""

    def __init__(self, cin, cout, bias=True):
        super().__init__()
        ref = torch.nn.Conv3d(cin, cout, 3, 1, 1, bias=bias)
        self.weight, self.bias = ref.weight, ref.bias

    def _conv(self, epi, x, sv, out_dtype):   # forward, or with epi the layer under fold.conv_bn
        return _submanifold_conv3d(x, self.weight, sv, self.bias, out_dtype, epi)

    def forward(self, x, sv: SparseVoxels, out_dtype=torch.bfloat16):
        return self._conv(None, x, sv, out_dtype)


# ---- the two-source layer: the submanifold convolution of [xa | xb] without the concatenation
def _conv_taps_cat(nmap, pairs, xa, ca, xb, cb, w, cout, bias, y, ydt, epi=None):
    """_conv_taps on x = [xa | xb] along channels (pcs_sparse_conv_cat, pcs_sparse_conv_cat_pairs)."""
    (rows, taps), st = nmap.shape, L.stream_ptr(xa.device)
    if pairs is None:
        L.forward_call("pcs_sparse_conv_cat", (nmap, rows, taps, xa, ca, xb, cb, w, cout, bias, y, ydt, 0), epi, st)
        return
    pin, _, ppos, tap_off, P = pairs
    z = torch.empty(max(P, 1), cout, dtype=torch.float32, device=xa.device)
    L.forward_call("pcs_sparse_conv_cat_pairs", (pin, ppos, ct.addressof(tap_off), taps, rows, xa, ca, xb, cb, w, cout, bias,
                                                 z, y, ydt, 0), epi, st)


def _dgrad_taps_cat(nmap, pairs, dyb, cout, wt, dxa, ca, dxb, cb):
    """(dxa, dxb) = the two column blocks of the input gradient, one gather pass over dyb
    (pcs_sparse_conv_cat_dgrad, pcs_sparse_conv_cat_dgrad_pairs); wt = _weight_t(wb)."""
    (rows, taps), st = nmap.shape, L.stream_ptr(dyb.device)
    if pairs is None:
        L.call("pcs_sparse_conv_cat_dgrad", nmap, rows, taps, dyb, cout, wt, dxa, ca, dxb, cb, L.BF16, 1, st)
        return
    pin, _, ppos, tap_off, P = pairs
    z = torch.empty(max(P, 1), ca + cb, dtype=torch.float32, device=dyb.device)
    L.call("pcs_sparse_conv_cat_dgrad_pairs", pin, ppos, ct.addressof(tap_off), taps, rows, dyb, cout, wt, z, dxa, ca,
           dxb, cb, L.BF16, 1, st)


def _sparse_wgrad_cat(nmap, pairs_fn, xa, xb, dyb, has_bias, use_pairs):
    """_sparse_wgrad with X's columns taken from xa, then xb; the workspaces are the concatenated
    layer's (the same split geometry, so the same summation order)."""
    (rows, taps), ca, cb, cout = nmap.shape, xa.shape[1], xb.shape[1], dyb.shape[1]
    cin = ca + cb
    if use_pairs:
        pin, pout, _, tap_off, _ = pairs_fn()
        nbytes = L.workspace("pcs_sparse_conv_wgrad_pairs_workspace", ct.addressof(tap_off), taps, rows, cin, cout)
        name, head = "pcs_sparse_conv_cat_wgrad_pairs", (pin, pout, ct.addressof(tap_off), taps, rows)
    else:
        nbytes = L.workspace("pcs_sparse_conv_wgrad_workspace", rows, taps, cin, cout)
        name, head = "pcs_sparse_conv_cat_wgrad", (nmap, rows, taps)
    head += (xa, ca, xb, cb, dyb, cout)
    return _wgrad(name, head, nbytes, taps, cin, cout, cin, cout, has_bias, xa.device)


def _sparse_cat_forward(xa, xb, wk, bias, sv, out_dtype, epi=None):
    """_sparse_forward on [xa | xb] along channels, ca, cb and cout multiples of 64 (pcs_sparse_conv_cat*;
    their _affine twins with the epilogue epi).  An empty level launches nothing.  Returns (y, xa, xb,
    wb, whether the pair lists carried it)."""
    V, ca, cb, cout = xa.shape[0], xa.shape[1], xb.shape[1], wk.shape[0]
    xa, xb = xa.contiguous(), xb.contiguous()
    wb = _bf16_2d(wk, cout, TAPS * (ca + cb))
    bk = None if bias is None else bias.float().contiguous()
    epi = epi and epi(cout, cout, (V, cout), xa.device)
    y = torch.empty(V, cout, dtype=out_dtype, device=xa.device)
    pairs = sv.use_pairs()
    if V > 0:
        _conv_taps_cat(sv.nbr, sv.pairs() if pairs else None, xa, ca, xb, cb, wb, cout, bk, y,
                       L.dtype_code(out_dtype, what="out_dtype"), epi)
    return y, xa, xb, wb, pairs


class _SubMConvCatFn(torch.autograd.Function):
    """_SubMConvFn on x = [xa | xb] (ca, cb and cout multiples of 64), which is never built: the
    kernels read the two arrays, autograd keeps xa and xb themselves, and one gather pass over dy
    writes both input gradients.  The dispatch is _SubMConvFn's at ca + cb input channels."""

    @staticmethod
    def forward(ctx, xa, xb, wk, bias, sv, out_dtype):
        y, xa, xb, wb, ctx.pairs = _sparse_cat_forward(xa, xb, wk, bias, sv, out_dtype)
        ctx.save_for_backward(xa, xb, wb, sv.nbr)
        ctx.sv = sv
        ctx.wpairs = PAIR_WGRAD and xa.shape[0] > 0 and (xa.shape[1] + xb.shape[1]) * wb.shape[0] <= PAIR_WGRAD_MAX_CH2
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        xa, xb, wb, nbr = ctx.saved_tensors
        (V, ca), cb, cout, dev = xa.shape, xb.shape[1], wb.shape[0], xa.device
        need_a, need_b, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        need_w = need_w or (ctx.has_bias and ctx.needs_input_grad[3])
        dxa = torch.empty(V, ca, dtype=torch.bfloat16, device=dev) if need_a else None
        dxb = torch.empty(V, cb, dtype=torch.bfloat16, device=dev) if need_b else None
        dwk = db = None
        if V == 0:   # an empty level: the entry points launch nothing and write nothing
            if need_w:
                dwk = torch.zeros(cout, TAPS * (ca + cb), dtype=torch.float32, device=dev)
                db = torch.zeros(cout, dtype=torch.float32, device=dev) if ctx.has_bias else None
            return dxa, dxb, dwk, db, None, None
        dyb = _bf16_2d(dy, V, cout)
        pairs = ctx.sv.pairs() if ctx.pairs else None
        if need_a or need_b:
            wt = _weight_t(wb, TAPS)   # [ca + cb, 27 * cout]: a row block per source
            if need_a and need_b:
                _dgrad_taps_cat(nbr, pairs, dyb, cout, wt, dxa, ca, dxb, cb)
            elif need_a:
                _conv_taps(nbr, pairs, dyb, cout, wt[:ca], ca, None, dxa, L.BF16, 1)
            else:
                _conv_taps(nbr, pairs, dyb, cout, wt[ca:], cb, None, dxb, L.BF16, 1)
        if need_w:
            dwk, db = _sparse_wgrad_cat(nbr, ctx.sv.pairs, xa, xb, dyb, ctx.has_bias, ctx.wpairs)
        return dxa, dxb, dwk, db, None, None


def _submanifold_conv3d_cat(xa, xb, weight, sv, bias, out_dtype, epi=None):
    """submanifold_conv3d_cat, or (epi) the same layer, with the same torch.cat fall-back, under
    fold.conv_bn's epilogue."""
    if not (xa.is_cuda and xb.is_cuda):
        raise RuntimeError("pcs_amd sparse conv runs on a HIP device only (no CPU fallback)")
    V = sv.nbr.shape[0]
    for name, t in (("xa", xa), ("xb", xb)):
        if t.dtype != torch.bfloat16 or t.dim() != 2 or t.shape[0] != V:
            raise ValueError(f"{name} must be bf16 [{V}, C]: one row per voxel of the [V, 27] neighbour map")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    ca, cb, cout = xa.shape[1], xb.shape[1], weight.shape[0]
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError("submanifold_conv3d_cat is the 3x3x3 form")
    if weight.shape[1] != ca + cb:
        raise ValueError(f"weight has {weight.shape[1]} input channels, xa and xb have {ca} + {cb}")
    if bias is not None and bias.shape != (cout,):
        raise ValueError(f"bias must be [{cout}]")
    if ca % CH_ALIGN or cb % CH_ALIGN or cout % CH_ALIGN or ca == 0 or cb == 0:
        return _submanifold_conv3d(torch.cat([xa, xb], 1), weight, sv, bias, out_dtype, epi)
    return _layer(_SubMConvCatFn, _sparse_cat_forward, epi, xa, xb, _kernel_weight(weight), bias, sv, out_dtype)


def submanifold_conv3d_cat(xa, xb, weight, sv: SparseVoxels, bias=None, out_dtype=torch.bfloat16):
    """submanifold_conv3d(torch.cat([xa, xb], 1), weight, sv, bias, out_dtype) without the
    concatenated tensor, and bit-identical to it (the same k-step and summation order): xa bf16
    [V, CA], xb bf16 [V, CB], weight [Cout, CA + CB, 3, 3, 3] (the concatenated layer's, fp32), bias
    [Cout] or None.  The forward writes and autograd keeps no [V, CA + CB] tensor, and the backward
    writes the two input gradients from one gather pass over dy (None for an input that needs none).
    The two-source kernels take CA, CB and Cout in multiples of 64; any other width runs torch.cat
    and submanifold_conv3d (zero-padded there): those shapes have no two-source path."""
    return _submanifold_conv3d_cat(xa, xb, weight, sv, bias, out_dtype)


class SubMConv3dCat(torch.nn.Module):
    """SubMConv3d(ca + cb, cout) applied to the channel concatenation of two inputs without building
    it (submanifold_conv3d_cat): a U-Net decoder's convolution of (up, skip).  The parameters are
    exactly nn.Conv3d(ca + cb, cout, 3, padding=1)'s, so state dicts load into SubMConv3d(ca + cb,
    cout) and back.  Widths off the multiple of 64 run torch.cat and the single-source layer."""

    def __init__(self, ca, cb, cout, bias=True):
        super().__init__()
        ref = torch.nn.Conv3d(ca + cb, cout, 3, 1, 1, bias=bias)
        self.weight, self.bias = ref.weight, ref.bias
        self.ca, self.cb = ca, cb

    def _conv(self, epi, xa, xb, sv, out_dtype):
        if xa.shape[-1] != self.ca or xb.shape[-1] != self.cb:
            raise ValueError(f"SubMConv3dCat({self.ca}, {self.cb}): got {xa.shape[-1]} and {xb.shape[-1]} channels")
        return _submanifold_conv3d_cat(xa, xb, self.weight, sv, self.bias, out_dtype, epi)

    def forward(self, xa, xb, sv: SparseVoxels, out_dtype=torch.bfloat16):
        return self._conv(None, xa, xb, sv, out_dtype)


# ---- stride-2 down / up convolutions (k = 2, s = 2) between a fine level and its coarse level
@dataclass
class CoarseLink:
    """The maps between the voxels of a level (grid G, even) and of its coarse level (G / 2): a
    coarse voxel is a 2x2x2 cell with at least one occupied fine voxel; tap = ((ix & 1) * 2 +
    (iy & 1)) * 2 + (iz & 1) is a fine voxel's corner of its cell (the tap order of a torch
    Conv3d weight [Cout, Cin, 2, 2, 2])."""
    child: torch.Tensor    # int32 [Vc, 8]: row of the fine voxel at tap t of the cell, or -1
    parent: torch.Tensor   # int32 [Vf]: row of the coarse voxel
    tap: torch.Tensor      # int32 [Vf]
    up: torch.Tensor       # int32 [Vf, 8]: parent[f] at column tap[f], -1 elsewhere
    fine: int
    coarse: int
    _down: tuple = field(default=None, repr=False)
    _up: tuple = field(default=None, repr=False)
    _cells: tuple = field(default=None, repr=False)

    def child_segments(self):
        """(src int32 [8 Vc], seg_off int64 [Vc + 1]): the child map as segments of eight taps, one per
        coarse voxel in tap order (segmax.sparse_max_pool's), built once."""
        if self._cells is None:
            seg_off = torch.arange(self.coarse + 1, dtype=torch.int64, device=self.child.device) * K2_TAPS
            self._cells = (self.child.reshape(-1), seg_off)
        return self._cells

    def down_pairs(self):
        """Pair lists of the child map (in: fine row, out: coarse row), as SparseVoxels.pairs()."""
        if self._down is None:
            self._down = _build_pairs(self.child)
        return self._down

    def up_pairs(self):
        """Pair lists of the up map (in: coarse row, out: fine row; every fine row once)."""
        if self._up is None:
            self._up = _build_pairs(self.up)
        return self._up

    def use_pairs(self) -> bool:
        """The form of the 8-tap gather through the child map (the pair lists or the tile gather):
        SparseVoxels.use_pairs()'s rule; the child map has one entry per fine voxel."""
        return self.coarse > 0 and self.fine <= PAIR_TAPS_MAX * self.coarse


def coarsen(sv: SparseVoxels):
    """(sv_coarse, link): the coarse level of sv (grid / 2; its voxels are the occupied 2x2x2
    cells, rows in ascending key order as sparse_from_keys documents, with their own hash table and
    27-neighbour map) and the CoarseLink between the two.  sv.grid must be even."""
    if sv.grid % 2 != 0:
        raise ValueError(f"coarsen: the grid must be even, got {sv.grid}")
    V, dev = sv.num_voxels, sv.keys.device
    st = L.stream_ptr(dev)
    pkey = torch.empty(V, dtype=torch.int64, device=dev)
    tap = torch.empty(V, dtype=torch.int32, device=dev)
    L.call("pcs_sparse_coarse_keys", sv.keys, V, sv.grid, pkey, tap, st)
    ckeys, crow = torch.unique(pkey, sorted=True, return_inverse=True)
    svc = sparse_from_keys(ckeys, sv.grid // 2)
    Vc = svc.num_voxels
    child = torch.empty(Vc, K2_TAPS, dtype=torch.int32, device=dev)
    parent = torch.empty(V, dtype=torch.int32, device=dev)
    up = torch.empty(V, K2_TAPS, dtype=torch.int32, device=dev)
    crow = crow.to(torch.int64).contiguous()
    L.call("pcs_sparse_coarse_maps", crow, tap, V, Vc, child, parent, up, st)
    return svc, CoarseLink(child, parent, tap, up, V, Vc)


def _conv_rows(link, x, cin, w, cout, bias, y, ydt, epi=None):
    """y[f] = b + W[tap[f]] x[parent[f]]: one tap per output row (pcs_sparse_conv_rows); epi: L.forward_call's."""
    pin, pout, _, tap_off, P = link.up_pairs()
    assert P == link.fine, "the up map has one pair per fine voxel"
    L.forward_call("pcs_sparse_conv_rows", (pin, pout, ct.addressof(tap_off), K2_TAPS, link.fine, x, cin, w, cout, bias, y,
                                            ydt), epi, L.stream_ptr(x.device))


def _conv_cells(link, x, cin, w, cout, bias, y, ydt):
    """y[m] = b + sum_t W[t] x[child[m][t]]: the 8-tap gather, through the pair lists or in tiles."""
    _conv_taps(link.child, link.down_pairs() if link.use_pairs() else None, x, cin, w, cout, bias, y, ydt)


class _StrideConvFn(torch.autograd.Function):
    """Both k = 2, s = 2 layers, w in kernel layout [Cout, 8 * Cin] (fp32 master), channel counts
    off the 64 multiple zero-padded (exact, as _SubMConvFn).
      down: y_c[m] = b + sum_t W_t x_f[child[m][t]];  dx_f[f] = W_tap(f)^T dy[parent[f]]
      up:   y_f[f] = b + W_tap(f) x_c[parent[f]];     dx_c[m] = sum_t W_t^T dy[child[m][t]]
    The weight gradient sums dy[out] (x) x[in] over the pairs of the forward's map."""

    @staticmethod
    def forward(ctx, x, wk, bias, link, out_dtype, up):
        y, xk, wb, _ = _sparse_forward(x, wk, bias, link, out_dtype, up)
        ctx.save_for_backward(xk, wb)
        ctx.link, ctx.up = link, up
        # the up map's tile-gather weight gradient would run 8 taps for the one each row has: the
        # up layer takes the pair lists at every width
        ctx.wpairs = up or (PAIR_WGRAD and xk.shape[1] * wb.shape[0] <= PAIR_WGRAD_MAX_CH2)
        ctx.cfg = (bias is not None, x.shape[1], wk.shape[0])
        return y

    @staticmethod
    def backward(ctx, dy):
        xk, wb = ctx.saved_tensors
        link, up = ctx.link, ctx.up
        has_bias, cin, cout = ctx.cfg
        rows_in, cin_k = xk.shape
        rows_out = link.fine if up else link.coarse
        cout_k = wb.shape[0]
        dyb = _bf16_2d(_pad_channels(dy, cout_k), rows_out, cout_k)
        dx = dwk = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(rows_in, cin_k, dtype=torch.bfloat16, device=xk.device)
            (_conv_cells if up else _conv_rows)(link, dyb, cout_k, _weight_t(wb, K2_TAPS), cin_k, None, dx, L.BF16)
            if cin_k != cin:
                dx = dx[:, :cin].contiguous()
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            dwk, db = _sparse_wgrad(link.up if up else link.child, link.up_pairs if up else link.down_pairs, xk, dyb,
                                    cin, cout, has_bias, ctx.wpairs)
        return dx, dwk, db, None, None, None


def _stride_conv3d(x, weight, link, bias, out_dtype, up, epi=None):
    """sparse_conv3d_down or (up) sparse_conv_transpose3d_up, or (epi) the same layer under fold.conv_bn's
    epilogue."""
    if tuple(weight.shape[2:]) != (2, 2, 2):
        raise ValueError(f"{'sparse_conv_transpose3d_up' if up else 'sparse_conv3d_down'} is the 2x2x2, stride-2 form")
    return _layer(_StrideConvFn, _sparse_forward, epi, x, _kernel_weight(weight, up), bias, link, out_dtype, up)


def sparse_conv3d_down(x_fine, weight, link: CoarseLink, bias=None, out_dtype=torch.bfloat16):
    """k = 2, s = 2 convolution from the fine voxels of link to its coarse voxels: x_fine bf16
    [Vf, Cin], weight [Cout, Cin, 2, 2, 2] (torch Conv3d layout, fp32), bias [Cout] or None; returns
    [Vc, Cout].  On a dense grid that is zero off the occupied fine voxels, the output at the
    coarse voxels equals Conv3d(k=2, s=2)'s there; every other coarse site would hold the bias
    alone and is not represented."""
    return _stride_conv3d(x_fine, weight, link, bias, out_dtype, False)


def sparse_conv_transpose3d_up(x_coarse, weight, link: CoarseLink, bias=None, out_dtype=torch.bfloat16):
    """k = 2, s = 2 transposed convolution from the coarse voxels of link back to its fine voxels:
    x_coarse bf16 [Vc, Cin], weight [Cin, Cout, 2, 2, 2] (torch ConvTranspose3d layout, fp32), bias
    [Cout] or None; returns [Vf, Cout].  On a dense coarse grid that is zero off the coarse voxels,
    the output at the fine occupied voxels equals ConvTranspose3d(k=2, s=2)'s there.  It takes the
    link of the encoder (an inverse convolution): the decoder returns to exactly the encoder's
    voxel set, the other fine sites of an occupied cell are not represented."""
    return _stride_conv3d(x_coarse, weight, link, bias, out_dtype, True)


class SparseDownConv3d(torch.nn.Module):
    """sparse_conv3d_down with nn.Conv3d(cin, cout, 2, 2)'s parameter layout and init."""

    def __init__(self, cin, cout, bias=True):
        super().__init__()
        ref = torch.nn.Conv3d(cin, cout, 2, 2, bias=bias)
        self.weight, self.bias = ref.weight, ref.bias

    def _conv(self, epi, x, link, out_dtype):
        return _stride_conv3d(x, self.weight, link, self.bias, out_dtype, False, epi)

    def forward(self, x, link: CoarseLink, out_dtype=torch.bfloat16):
        return self._conv(None, x, link, out_dtype)


class SparseUpConv3d(torch.nn.Module):
    """sparse_conv_transpose3d_up with nn.ConvTranspose3d(cin, cout, 2, 2)'s parameter layout and
    init."""

    def __init__(self, cin, cout, bias=True):
        super().__init__()
        ref = torch.nn.ConvTranspose3d(cin, cout, 2, 2, bias=bias)
        self.weight, self.bias = ref.weight, ref.bias

    def _conv(self, epi, x, link, out_dtype):
        return _stride_conv3d(x, self.weight, link, self.bias, out_dtype, True, epi)

    def forward(self, x, link: CoarseLink, out_dtype=torch.bfloat16):
        return self._conv(None, x, link, out_dtype)


__all__ = ["CH_ALIGN", "CoarseLink", "SparseDownConv3d", "SparseUpConv3d", "SparseVoxels", "SubMConv3d", "SubMConv3dCat",
           "coarsen", "sparse_conv3d_down", "sparse_conv_transpose3d_up", "sparse_from_keys", "sparse_voxels",
           "submanifold_conv3d", "submanifold_conv3d_cat"]
