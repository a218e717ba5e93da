"""Point -> voxel path on the device (north-star voxel vocabulary).

The reference segments raw points (P:98-133); it has no voxel grid.  This module adds the
north star's "point->voxel scatter" and "hash-indexed gather" around the unchanged model:

    vb = voxelize(rb, grid=256, lo=(-1,-1,-1), hi=(1,1,1), num_classes=C)   # pcs_voxelize
    points, labels, masks = pad_on_device(vb.batch)                         # voxel batch
    logits = model(points)                                                   # [B, Nv, C]
    point_logits = to_points(logits, vb)                                     # pcs_gather_rows

A voxel is one occupied cell of a G^3 lattice per scene: (mean x, mean y, mean z, summed e)
of its points, the most frequent label, and its point count.  Integer outputs (voxel ids,
voxel order, inverse map, counts, labels) are bit-exact with oracle/voxel_oracle.py; its
semantics are build-defined ("not reference parity").
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib as L
from .data import RaggedBatch


@dataclass
class VoxelBatch:
    batch: RaggedBatch            # voxels as a CSR batch: points [V,4], labels [V], offsets [B+1]
    counts: torch.Tensor          # int64 [V] points per voxel
    voxel_of_point: torch.Tensor  # int64 [T] global voxel index of every input point
    grid: int


def _box(lo, hi):
    lo = [float(v) for v in lo]
    hi = [float(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3 or any(h <= l for l, h in zip(lo, hi)):
        raise ValueError("lo / hi must be 3 bounds with hi > lo")
    return lo + hi


def voxel_ids(points: torch.Tensor, grid: int, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
    """int64 voxel id of each point (points: fp32 [T, 4] on the device)."""
    if not points.is_cuda:
        raise RuntimeError("voxel_ids runs on a HIP device only (no CPU fallback)")
    pts = points.contiguous().float()
    out = torch.empty(pts.shape[0], dtype=torch.int64, device=pts.device)
    L.call("pcs_voxel_ids", pts, pts.shape[0], int(grid), *_box(lo, hi), out, L.stream_ptr())
    return out


def voxelize(rb: RaggedBatch, grid: int, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), num_classes: int = 2,
             device=None) -> VoxelBatch:
    """Occupied-voxel scatter of a CSR batch (pcs_voxelize).  One host read (the voxel count)
    sizes the outputs."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda":
        raise RuntimeError("voxelize runs on a HIP device only (no CPU fallback)")
    pts = rb.points.to(device, torch.float32).contiguous()
    lab = rb.labels.to(device, torch.int64).contiguous() if rb.labels is not None else None
    off = rb.offsets.to(device, torch.int64).contiguous()
    B, T = off.numel() - 1, pts.shape[0]
    if T == 0:
        raise ValueError("voxelize needs at least one point")
    ws = torch.empty(int(L.load().pcs_voxelize_workspace(T)), dtype=torch.uint8, device=device)
    vop = torch.empty(T, dtype=torch.int64, device=device)
    vpts = torch.empty(T, 4, dtype=torch.float32, device=device)
    vlab = torch.empty(T, dtype=torch.int64, device=device)
    vcnt = torch.empty(T, dtype=torch.int64, device=device)
    voff = torch.empty(B + 1, dtype=torch.int64, device=device)
    nv = torch.empty(1, dtype=torch.int64, device=device)
    L.call("pcs_voxelize", pts, lab, off, B, T, int(grid), *_box(lo, hi), int(num_classes), ws, ws.numel(), vop, vpts,
           vlab, vcnt, voff, nv, L.stream_ptr(device))
    V = int(nv.item())
    return VoxelBatch(RaggedBatch(vpts[:V], vlab[:V], voff), vcnt[:V], vop, int(grid))


def to_points(voxel_logits: torch.Tensor, vb: VoxelBatch) -> torch.Tensor:
    """Per-point outputs [T, C] from per-voxel outputs: padded [B, Nv, C] (the model's output
    on pad_on_device(vb.batch)) or flat [V, C] (pcs_voxel_padded_index + pcs_gather_rows)."""
    out_dev = voxel_logits.device
    x = voxel_logits.contiguous().float()
    T = vb.voxel_of_point.numel()
    C = x.shape[-1]
    if x.dim() == 3:
        B, Nv = x.shape[0], x.shape[1]
        idx = torch.empty(T, dtype=torch.int64, device=out_dev)
        L.call("pcs_voxel_padded_index", vb.voxel_of_point, T, vb.batch.offsets, B, Nv, idx, L.stream_ptr(out_dev))
        src = x.view(B * Nv, C)
    else:
        idx, src = vb.voxel_of_point, x
    out = torch.empty(T, C, dtype=torch.float32, device=out_dev)
    L.call("pcs_gather_rows", src, src.stride(0), idx, T, C, out, L.stream_ptr(out_dev))
    return out


# ---------------------------------------------------------------------------------------------
# Dense 3-D convolutions on channels-last voxel grids (pcs_conv3d*, csrc/conv3d.hip): the north
# star's U-Net building blocks -- the 3x3x3 stencil (k=3, s=1, p=1), the 2x2x2 stride-2
# downsampling and its transposed upsampling.  Build-defined like the rest of this module: the
# reference has no voxel grid, parity is against torch's conv3d / conv_transpose3d (fp64).
# Activations are [B, D, H, W, C] bf16 (channels innermost); parameters keep torch's layouts
# (Conv3d [Cout, Cin, k, k, k], ConvTranspose3d [Cin, Cout, k, k, k]) in fp32, cast to bf16 per
# call by pcs_cast_weight.
# ---------------------------------------------------------------------------------------------

def _out_size(d, k, s, p, transposed, op=0):
    return (d - 1) * s - 2 * p + k + op if transposed else (d + 2 * p - k) // s + 1


def _geom(B, grid_in, cin, cout, k, s, p, transposed, op=(0, 0, 0)):
    """Conv3dGeom of one call.  op = torch's output_padding (transposed form only, 0 <= op < s per
    dimension): the trailing output planes a strided convolution's floor division skips, which the
    input gradient of that convolution needs to cover its whole input grid."""
    op = (op,) * 3 if isinstance(op, int) else tuple(op)
    if any(o < 0 or o >= max(s, 1) for o in op) or (any(op) and not transposed):
        raise ValueError(f"output_padding {op} must satisfy 0 <= op < stride = {s} (transposed form only)")
    out = [_out_size(d, k, s, p, transposed, o) for d, o in zip(grid_in, op)]
    if min(out) <= 0:
        raise ValueError(f"empty output grid {out} for input {list(grid_in)}, k={k}, s={s}, p={p}")
    return L.Conv3dGeom(B=B, Di=grid_in[0], Hi=grid_in[1], Wi=grid_in[2], Do=out[0], Ho=out[1], Wo=out[2],
                        Cin=cin, Cout=cout, k=k, s=s, p=p, transposed=int(transposed))


def _bf16_2d(t, rows, cols):
    """bf16 copy of a [rows, cols] tensor on the device (pcs_cast_weight for fp32 input)."""
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        return t
    out = torch.empty(rows, cols, dtype=torch.bfloat16, device=t.device)
    L.call("pcs_cast_weight", t.float(), rows, cols, cols, L.BF16, out, None, L.stream_ptr(t.device))
    return out


CH_ALIGN = 64   # channel multiple of the sparse conv kernels' 64-wide tiles (sparse.py)
DENSE_CH_ALIGN = 32   # the dense conv3d kernels' tiles: 64 channels, or 32 for a 32-channel level


def _ceil(c, m=CH_ALIGN):
    return (c + m - 1) // m * m


def _pad_channels(t, c_to):
    """[..., C] -> [..., c_to] with zero channels appended (a device copy; no-op when C == c_to)."""
    if t.shape[-1] == c_to:
        return t.contiguous()
    out = t.new_zeros(*t.shape[:-1], c_to)
    out[..., : t.shape[-1]] = t
    return out


def _conv_operands(x, wk, bias, taps, align):
    """(xk, wb, bk, cin_k, cout_k) of every convolution here, dense or sparse: channel counts off
    the align multiple run zero-padded, x with zero input channels, the kernel-layout weight wk
    [Cout, taps * Cin] (fp32 master; wb in bf16) and the bias with zero output channels, and the
    padded output / gradient channels are sliced off.  Zero channels contribute exact zeros, so
    results equal the unpadded convolution's."""
    cin, cout = x.shape[-1], wk.shape[0]
    cin_k, cout_k = _ceil(cin, align), _ceil(cout, align)
    if (cin_k, cout_k) != (cin, cout):
        wp = wk.new_zeros(cout_k, taps, cin_k)
        wp[:cout, :, :cin] = wk.reshape(cout, taps, cin)
        wk = wp.reshape(cout_k, taps * cin_k)
    bk = None if bias is None else _pad_channels(bias.float(), cout_k)
    return _pad_channels(x, cin_k), _bf16_2d(wk, cout_k, taps * cin_k), bk, cin_k, cout_k


def _unpad(y, cout):
    """y without the output channels _conv_operands padded."""
    return y if y.shape[-1] == cout else y[..., :cout].contiguous()


def _kernel_weight(weight, transposed=False):
    """The kernel layout [Cout, taps * Cin] of a parameter in torch's: Conv3d's [Cout, Cin, k, k, k] or
    (transposed) ConvTranspose3d's [Cin, Cout, k, k, k]."""
    w = weight.permute(1, 2, 3, 4, 0) if transposed else weight.permute(0, 2, 3, 4, 1)
    return w.reshape(w.shape[0], -1)


def _layer(fn, forward, epi, *args):
    """One convolution layer, dense or sparse: fn.apply(*args) under autograd, whose forward is
    forward(*args); with an epilogue (fold.conv_bn, inference) that function alone, with nothing kept
    for a backward.  Either way the operands, the route and the launch are forward's."""
    return fn.apply(*args) if epi is None else forward(*args, epi=epi)[0]


def _weight_t(wb, taps):
    """wb [Cout, taps * Cin] transposed per tap (pcs_conv3d_weight_t): an input gradient's weight."""
    cout_k, cin_k = wb.shape[0], wb.shape[1] // taps
    wt = torch.empty(cin_k, taps * cout_k, dtype=torch.bfloat16, device=wb.device)
    L.call("pcs_conv3d_weight_t", wb, cout_k, taps, cin_k, wt, L.stream_ptr(wb.device))
    return wt


def _wgrad(name, head, nbytes, taps, cin, cout, cin_k, cout_k, has_bias, dev):
    """(dwk, db) of the weight-gradient entry point name(*head, workspace, nbytes, dW, db, stream),
    without the channels _conv_operands padded."""
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
    dwk = torch.empty(cout_k, taps * cin_k, dtype=torch.float32, device=dev)
    db = torch.empty(cout_k, dtype=torch.float32, device=dev) if has_bias else None
    L.call(name, *head, ws, nbytes, dwk, db, L.stream_ptr(dev))
    if (cin_k, cout_k) != (cin, cout):
        dwk = dwk.reshape(cout_k, taps, cin_k)[:cout, :, :cin].reshape(cout, taps * cin)
        db = db[:cout] if has_bias else None
    return dwk, db


def _conv3d_forward(x, wk, bias, k, s, p, transposed, out_dtype, op, epi=None):
    """The forward of every single-source dense convolution, unfused (pcs_conv3d) or with the epilogue
    epi of fold.conv_bn (pcs_conv3d_affine): x bf16 [B, D, H, W, Cin], wk the kernel-layout weight
    [Cout, k^3 * Cin] (fp32 master).  Returns (y, xk, wb): y without the padded channels, and the
    operands as the kernel read them, which the backward keeps."""
    if not x.is_cuda:
        raise RuntimeError("pcs_amd conv3d runs on a HIP device only (no CPU fallback)")
    if x.dtype != torch.bfloat16 or x.dim() != 5:
        raise ValueError("x must be a bf16 [B, D, H, W, C] channels-last voxel grid")
    B, D, H, W, cin = x.shape
    cout, taps = wk.shape[0], k ** 3
    if wk.shape[1] != taps * cin:
        raise ValueError(f"weight has {wk.shape[1] // taps} input channels, x has {cin}")
    xk, wb, bk, cin_k, cout_k = _conv_operands(x, wk, bias, taps, DENSE_CH_ALIGN)
    g = _geom(B, (D, H, W), cin_k, cout_k, k, s, p, transposed, op)
    epi = epi and epi(cout, cout_k, (B, g.Do, g.Ho, g.Wo, cout), x.device)
    y = torch.empty(B, g.Do, g.Ho, g.Wo, cout_k, dtype=out_dtype, device=x.device)
    L.forward_call("pcs_conv3d", (g, xk, wb, bk, y, L.dtype_code(out_dtype, what="out_dtype")), epi,
                   L.stream_ptr(x.device))
    return _unpad(y, cout), xk, wb


class _Conv3dFn(torch.autograd.Function):
    """y = conv(x, w) + b with w in kernel layout [Cout, taps * Cin] (fp32 master).  Multiples of
    32 run natively (a 32-channel U-Net level on 32-channel tiles); other channel counts (a first
    layer on raw point features) run zero-padded (_conv_operands)."""

    @staticmethod
    def forward(ctx, x, wk, bias, k, s, p, transposed, out_dtype, op):
        y, xk, wb = _conv3d_forward(x, wk, bias, k, s, p, transposed, out_dtype, op)
        ctx.save_for_backward(xk, wb)
        ctx.cfg = (k, s, p, transposed, bias is not None, op, x.shape[-1], wk.shape[0])
        return y

    @staticmethod
    def backward(ctx, dy):
        xk, wb = ctx.saved_tensors
        k, s, p, transposed, has_bias, op, cin, cout = ctx.cfg
        B, D, H, W, cin_k = xk.shape
        cout_k = wb.shape[0]
        taps = k ** 3
        g = _geom(B, (D, H, W), cin_k, cout_k, k, s, p, transposed, op)
        M = B * g.Do * g.Ho * g.Wo
        dyb = _bf16_2d(_pad_channels(dy, cout_k).reshape(M, cout_k), M, cout_k)
        dev, st = xk.device, L.stream_ptr(xk.device)
        dx = dwk = db = None
        if ctx.needs_input_grad[0]:
            # the input gradient of a convolution is the transposed convolution of dy with W_t^T
            # (and vice versa): same k, s, p, grids swapped.  A strided convolution whose floor
            # division skipped trailing input planes gets them back as the transposed form's
            # output_padding; a transposed one's own output_padding planes are read as rows of dy.
            wt = _weight_t(wb, taps)
            back_op = (0, 0, 0)
            if not transposed:
                back_op = tuple(d - _out_size(o, k, s, p, True) for d, o in zip((D, H, W), (g.Do, g.Ho, g.Wo)))
            gb = _geom(B, (g.Do, g.Ho, g.Wo), cout_k, cin_k, k, s, p, not transposed, back_op)
            if (gb.Do, gb.Ho, gb.Wo) != (D, H, W):
                raise ValueError("input gradient: the strided output grid does not map back onto the input grid")
            dx = torch.empty_like(xk)
            L.call("pcs_conv3d", gb, dyb, wt, None, dx, L.BF16, st)
            if cin_k != cin:
                dx = dx[..., :cin].contiguous()
        if ctx.needs_input_grad[1] or (has_bias and ctx.needs_input_grad[2]):
            nbytes = L.workspace("pcs_conv3d_wgrad_workspace", g)
            dwk, db = _wgrad("pcs_conv3d_wgrad", (g, xk, dyb), nbytes, taps, cin, cout, cin_k, cout_k, has_bias, dev)
        return dx, dwk, db, None, None, None, None, None, None


def _conv3d(x, weight, bias, stride, padding, out_dtype, epi=None, transposed=False, output_padding=0):
    """conv3d / conv_transpose3d, or (epi) the same layer under fold.conv_bn's epilogue."""
    op = output_padding
    op = (int(op),) * 3 if isinstance(op, int) else tuple(int(o) for o in op)
    return _layer(_Conv3dFn, _conv3d_forward, epi, x, _kernel_weight(weight, transposed), bias, weight.shape[2],
                  int(stride), int(padding), transposed, out_dtype, op)


def conv3d(x, weight, bias=None, stride=1, padding=0, out_dtype=torch.bfloat16):
    """torch.nn.functional.conv3d on a channels-last bf16 grid x [B, D, H, W, Cin];
    weight [Cout, Cin, k, k, k] (torch layout, fp32), bias [Cout] or None."""
    return _conv3d(x, weight, bias, stride, padding, out_dtype)


def conv_transpose3d(x, weight, bias=None, stride=2, padding=0, out_dtype=torch.bfloat16, output_padding=0):
    """torch.nn.functional.conv_transpose3d on a channels-last bf16 grid x [B, D, H, W, Cin];
    weight [Cin, Cout, k, k, k] (torch layout, fp32), bias [Cout] or None; output_padding as
    torch's (an int or 3 ints, each < stride)."""
    return _conv3d(x, weight, bias, stride, padding, out_dtype, None, True, output_padding)


class Conv3d(torch.nn.Module):
    """nn.Conv3d(cin, cout, k, stride, padding) with torch's parameter layout and init, on
    channels-last bf16 voxel grids (pcs_conv3d)."""

    def __init__(self, cin, cout, kernel_size=3, stride=1, padding=1, bias=True):
        super().__init__()
        ref = torch.nn.Conv3d(cin, cout, kernel_size, stride, padding, bias=bias)
        self.weight, self.bias = ref.weight, ref.bias
        self.stride, self.padding = stride, padding

    def _conv(self, epi, x, out_dtype):   # forward, or with epi the layer under fold.conv_bn
        return _conv3d(x, self.weight, self.bias, self.stride, self.padding, out_dtype, epi)

    def forward(self, x, out_dtype=torch.bfloat16):
        return self._conv(None, x, out_dtype)


class ConvTranspose3d(torch.nn.Module):
    """nn.ConvTranspose3d(cin, cout, k, stride, padding) with torch's parameter layout and init,
    on channels-last bf16 voxel grids (pcs_conv3d, transposed form)."""

    def __init__(self, cin, cout, kernel_size=2, stride=2, padding=0, output_padding=0, bias=True):
        super().__init__()
        ref = torch.nn.ConvTranspose3d(cin, cout, kernel_size, stride, padding, output_padding, bias=bias)
        self.weight, self.bias = ref.weight, ref.bias
        self.stride, self.padding, self.output_padding = stride, padding, output_padding

    def _conv(self, epi, x, out_dtype):
        return _conv3d(x, self.weight, self.bias, self.stride, self.padding, out_dtype, epi, True, self.output_padding)

    def forward(self, x, out_dtype=torch.bfloat16):
        return self._conv(None, x, out_dtype)


# ---- the two-source stencil (pcs_conv3d_cat*, include/pcs_dense.h): a decoder's convolution of
# (up, skip) without the concatenated grid
def _conv3d_cat_forward(xa, xb, wk, bias, out_dtype, epi=None):
    """_conv3d_forward (k = 3, s = 1, p = 1) on [xa | xb] along channels, ca, cb and cout multiples of 32
    (pcs_conv3d_cat; pcs_conv3d_cat_affine with the epilogue epi).  Returns (y, xa, xb, wb)."""
    B, D, H, W, ca = xa.shape
    cb, cout = xb.shape[-1], wk.shape[0]
    xa, xb = xa.contiguous(), xb.contiguous()
    wb = _bf16_2d(wk, cout, 27 * (ca + cb))
    bk = None if bias is None else bias.float().contiguous()
    g = _geom(B, (D, H, W), ca + cb, cout, 3, 1, 1, False)
    epi = epi and epi(cout, cout, (B, D, H, W, cout), xa.device)
    y = torch.empty(B, D, H, W, cout, dtype=out_dtype, device=xa.device)
    L.forward_call("pcs_conv3d_cat", (g, xa, ca, xb, cb, wb, bk, y, L.dtype_code(out_dtype, what="out_dtype")), epi,
                   L.stream_ptr(xa.device))
    return y, xa, xb, wb


class _Conv3dCatFn(torch.autograd.Function):
    """_Conv3dFn (k = 3, s = 1, p = 1) on x = [xa | xb] along channels (ca, cb and cout multiples of
    32), which is never built: the kernels read the two grids, autograd keeps xa and xb themselves,
    and one stencil pass over dy writes both input gradients.  Tiles, k-step order and workspace are
    _Conv3dFn's at ca + cb input channels."""

    @staticmethod
    def forward(ctx, xa, xb, wk, bias, out_dtype):
        y, *saved = _conv3d_cat_forward(xa, xb, wk, bias, out_dtype)
        ctx.save_for_backward(*saved)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        xa, xb, wb = ctx.saved_tensors
        (B, D, H, W, ca), cb, cout = xa.shape, xb.shape[-1], wb.shape[0]
        dev, st, M = xa.device, L.stream_ptr(xa.device), B * D * H * W
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_w = ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3])
        dyb = _bf16_2d(dy.reshape(M, cout), M, cout)
        dxa = dxb = dwk = db = None
        if need_a or need_b:
            wt = _weight_t(wb, 27)   # [ca + cb, 27 * cout]: a row block per source
            if need_a and need_b:
                dxa, dxb = torch.empty_like(xa), torch.empty_like(xb)
                gb = _geom(B, (D, H, W), cout, ca + cb, 3, 1, 1, True)
                L.call("pcs_conv3d_cat_dgrad", gb, dyb, wt, dxa, ca, dxb, cb, L.BF16, st)
            else:   # one source only: the single-source stencil on that source's rows of W^T
                c, rows = (ca, wt[:ca]) if need_a else (cb, wt[ca:])
                dx = torch.empty(B, D, H, W, c, dtype=torch.bfloat16, device=dev)
                L.call("pcs_conv3d", _geom(B, (D, H, W), cout, c, 3, 1, 1, True), dyb, rows.contiguous(), None, dx,
                       L.BF16, st)
                dxa, dxb = (dx, None) if need_a else (None, dx)
        if need_w:
            g = _geom(B, (D, H, W), ca + cb, cout, 3, 1, 1, False)
            nbytes = L.workspace("pcs_conv3d_wgrad_workspace", g)
            dwk, db = _wgrad("pcs_conv3d_cat_wgrad", (g, xa, ca, xb, cb, dyb), nbytes, 27, ca + cb, cout, ca + cb, cout,
                             ctx.has_bias, dev)
        return dxa, dxb, dwk, db, None


def _conv3d_cat(xa, xb, weight, bias, out_dtype, epi=None):
    """conv3d_cat, or (epi) the same layer, with the same torch.cat fall-back, under fold.conv_bn's epilogue."""
    if not (xa.is_cuda and xb.is_cuda):
        raise RuntimeError("pcs_amd conv3d runs on a HIP device only (no CPU fallback)")
    for name, t in (("xa", xa), ("xb", xb)):
        if t.dtype != torch.bfloat16 or t.dim() != 5:
            raise ValueError(f"{name} must be a bf16 [B, D, H, W, C] channels-last voxel grid")
    if xa.shape[:4] != xb.shape[:4]:
        raise ValueError(f"xa and xb must share their grid: {list(xa.shape[:4])} and {list(xb.shape[:4])}")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("out_dtype must be torch.bfloat16 or torch.float32")
    ca, cb, cout = xa.shape[-1], xb.shape[-1], weight.shape[0]
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3):
        raise ValueError("conv3d_cat is the 3x3x3 form")
    if weight.shape[1] != ca + cb:
        raise ValueError(f"weight has {weight.shape[1]} input channels, xa and xb have {ca} + {cb}")
    if bias is not None and bias.shape != (cout,):
        raise ValueError(f"bias must be [{cout}]")
    if ca % DENSE_CH_ALIGN or cb % DENSE_CH_ALIGN or cout % DENSE_CH_ALIGN or ca == 0 or cb == 0:
        return _conv3d(torch.cat([xa, xb], -1), weight, bias, 1, 1, out_dtype, epi)
    return _layer(_Conv3dCatFn, _conv3d_cat_forward, epi, xa, xb, _kernel_weight(weight), bias, out_dtype)


def conv3d_cat(xa, xb, weight, bias=None, out_dtype=torch.bfloat16):
    """conv3d(torch.cat([xa, xb], -1), weight, bias, stride=1, padding=1) without the concatenated
    grid, and bit-identical to it (the same k-step and summation order): xa bf16 [B, D, H, W, CA], xb
    bf16 [B, D, H, W, CB], weight [Cout, CA + CB, 3, 3, 3] (the concatenated layer's, fp32), bias
    [Cout] or None.  The forward writes and autograd keeps no [.., CA + CB] tensor, and the backward
    writes the two input gradients from one stencil pass over dy (None for an input that needs none).
    The two-source kernels take CA, CB and Cout in multiples of 32; any other width runs torch.cat
    and conv3d (zero-padded there): those shapes have no two-source path."""
    return _conv3d_cat(xa, xb, weight, bias, out_dtype)


class Conv3dCat(torch.nn.Module):
    """Conv3d(ca + cb, cout, 3, padding=1) applied to the channel concatenation of two grids without
    building it (conv3d_cat): a U-Net decoder's convolution of (up, skip).  The parameters are exactly
    nn.Conv3d(ca + cb, cout, 3, padding=1)'s, so state dicts load into Conv3d(ca + cb, cout) and back.
    Widths off the multiple of 32 run torch.cat and the single-source layer."""

    def __init__(self, ca, cb, cout, bias=True):
        super().__init__()
        ref = torch.nn.Conv3d(ca + cb, cout, 3, 1, 1, bias=bias)
        self.weight, self.bias = ref.weight, ref.bias
        self.ca, self.cb = ca, cb

    def _conv(self, epi, xa, xb, out_dtype):
        if xa.shape[-1] != self.ca or xb.shape[-1] != self.cb:
            raise ValueError(f"Conv3dCat({self.ca}, {self.cb}): got {xa.shape[-1]} and {xb.shape[-1]} channels")
        return _conv3d_cat(xa, xb, self.weight, self.bias, out_dtype, epi)

    def forward(self, xa, xb, out_dtype=torch.bfloat16):
        return self._conv(None, xa, xb, out_dtype)
