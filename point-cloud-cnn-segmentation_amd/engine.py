"""Kernel orchestration for one PointNetSegmentation training / inference pass.

Host side of the hot path: allocates (through torch's caching allocator) the points-major
activation buffers, and launches the HIP kernels of libpcs.so in dependency order on the
current stream.  Nothing here computes on the CPU; every numeric op is a C-ABI call.

Per layer l the forward stores only Y_l = conv_l(a_{l-1}) (pre-BN, fp32 or bf16);
a_l = relu(bn_l(Y_l)) [* dropout] is recomputed inside whichever kernel consumes it.
The exception is the 1024-wide pair conv5 / global_feat: conv5 runs twice (a statistics pass,
then a pass that applies bn5 + ReLU on the way out), so a5 = relu(bn5(y5)) is stored instead of
y5, and global_feat's output is never stored (its epilogue keeps only BN statistics and the
max-pool candidates).  Both 1024-deep global_feat GEMMs then read a5 raw, which lets them stage
it HBM -> LDS by DMA (csrc/gemm_glds.hip).
The backward stores dZ_l = dL/d(BN_l output) after the ReLU / dropout masks and forms
dy_l = alpha*dZ_l + beta + gamma*Y_l on the fly in the dgrad / wgrad kernels.

Which kernels a pass takes is resolved once (resolve_paths) into the Paths record the forward
stores on Saved; every stage of both passes branches on that record only.  The stages, in order:
  forward   _trunk (conv1..conv4), _conv5 (bn5 statistics, BN + ReLU pass), _global_feat (Gram and
            statistics, signed weights, pool, finalize), _seg (scene bias, seg_conv1/2 or _seg12,
            seg_conv3), _head
  backward  _bwd_seg32 (head reduce, seg_conv3, seg_conv2), _bwd_pool (repeat / cat / max-pool /
            bn_global), _bwd_seg1_local, bucket "seg", _bwd_global_dgrad, _bwd_global_wgrad, bucket
            "global", _bwd_conv5, _bwd_trunk (conv4..conv1), bucket "tail"

Reference map (point_cloud_segmentation.py, P:<line>):
  forward P:98-133, loss P:216/251, backward P:254, running stats (nn.BatchNorm1d).
"""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass, field

import torch

from . import _lib as L

BN_EPS = 1e-5
MAX_INPUT_DIM = 8     # conv1 kernels (csrc/small.hip) are instantiated for K = 1..8
MAX_CLASSES = 256     # head kernels (csrc/small.hip: 16 / 64 classes, and the wide head up to 256)
BN_MOMENTUM = 0.1
DROPOUT_P = 0.3

# (conv, Cin, Cout, bn) in registration order; Cin of conv1 / Cout of seg_conv4 filled in
CONVS = [
    ("conv1", None, 64, "bn1"),
    ("conv2", 64, 64, "bn2"),
    ("conv3", 64, 64, "bn3"),
    ("conv4", 64, 128, "bn4"),
    ("conv5", 128, 1024, "bn5"),
    ("global_feat", 1024, 1024, "bn_global"),
    ("seg_conv1", 1088, 512, "bn_seg1"),
    ("seg_conv2", 512, 256, "bn_seg2"),
    ("seg_conv3", 256, 128, "bn_seg3"),
    ("seg_conv4", 128, None, None),
]
BNS = [(bn, cout) for _, _, cout, bn in CONVS if bn]
_LAYERS = {conv: (cin, cout, bn) for conv, cin, cout, bn in CONVS}


def param_layout(num_classes: int, input_dim: int = 4):
    """[(name, shape)] of the parameters in registration order (== module.parameters())."""
    out = []
    for conv, cin, cout, _ in CONVS:
        cin = input_dim if cin is None else cin
        cout = num_classes if cout is None else cout
        out += [(f"{conv}.weight", (cout, cin, 1)), (f"{conv}.bias", (cout,))]
    for bn, c in BNS:
        out += [(f"{bn}.weight", (c,)), (f"{bn}.bias", (c,))]
    return out


# Flat fp32 buffers (parameters / gradients, optim.flatten_parameters): the parameters are
# grouped by when the backward finishes their gradients, so each all-reduce bucket (§8 e) is
# one contiguous range issued as soon as the backward has written it:
#   "seg"    seg_conv1..seg_conv4 + the EXTRA tail (loss numerator, CE weight sum, valid
#            count): ready once seg_conv1's local input/weight gradient has run;
#   "global" global_feat: ready after the Gram-form weight gradient (mid-backward);
#   "tail"   the 9 BatchNorms and conv1..conv5: ready at the end.
FLAT_EXTRA = 4
_SEG = ("seg_conv1", "seg_conv2", "seg_conv3", "seg_conv4")
_EARLY_CONVS = ("conv1", "conv2", "conv3", "conv4", "conv5")


def flat_layout(num_classes: int, input_dim: int = 4):
    """[(name, shape)] in flat-buffer order (see above); registration order is param_layout."""
    reg = dict(param_layout(num_classes, input_dim))
    names = [f"{bn}.{w}" for bn, _ in BNS for w in ("weight", "bias")]
    for conv in _EARLY_CONVS + ("global_feat",) + _SEG:
        names += [f"{conv}.weight", f"{conv}.bias"]
    return [(n, reg[n]) for n in names]


def flat_offsets(num_classes: int, input_dim: int = 4):
    """name -> element offset in the flat buffers; the EXTRA tail starts at the total."""
    offs, off = {}, 0
    for n, shape in flat_layout(num_classes, input_dim):
        offs[n] = off
        off += int(torch.Size(shape).numel())
    return offs, off


def bucket_ranges(num_classes: int, input_dim: int = 4):
    """Gradient all-reduce buckets: name -> [lo, hi) element range of the flat gradient
    buffer (which carries FLAT_EXTRA scalars after the parameters)."""
    offs, total = flat_offsets(num_classes, input_dim)
    return {"seg": (offs["seg_conv1.weight"], total + FLAT_EXTRA),
            "global": (offs["global_feat.weight"], offs["seg_conv1.weight"]),
            "tail": (0, offs["global_feat.weight"])}


def check_dims(num_classes: int, input_dim: int):
    """The reference accepts any input_dim / num_classes (P:66-83; num_classes comes from the
    data, P:153); the kernels cover input_dim 1..8 (conv1 is unrolled over K) and 1..256
    classes (the head keeps seg_conv4's fp32 weight in LDS: 128 KB at 256 classes)."""
    if not 1 <= int(input_dim) <= MAX_INPUT_DIM:
        raise ValueError(f"pcs_amd supports input_dim 1..{MAX_INPUT_DIM} (the reference's points carry "
                         f"4: x, y, z, e); got {input_dim}")
    if not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"pcs_amd supports 1..{MAX_CLASSES} classes (seg_conv4 + CE head kernel); "
                         f"got {num_classes}")


def _dt(dtype: str):
    """(C-ABI dtype, torch dtype) of the stored activations.  "fp8" is the bf16 path with the
    wide layer (a5 = relu(bn5(y5)) and global_feat's operands) in fp8 e4m3."""
    if dtype == "fp32":
        return L.F32, torch.float32
    if dtype in ("bf16", "fp8"):
        return L.BF16, torch.bfloat16
    raise ValueError(f"compute dtype must be 'fp32', 'bf16' or 'fp8', got {dtype!r}")


@dataclass(frozen=True)
class Paths:
    """Which kernels one pass takes: resolved once by the forward (resolve_paths), stored on Saved, and the only thing
    the stages of the forward and the backward branch on."""
    flags: int              # the PCS_FLAG_* bits every launch of the pass carries
    bf16: bool              # bf16 activation storage ("bf16" and "fp8")
    wide_fast: bool         # stored-a5 Gram + conv5 column sums, Gram-derived bn_global statistics,
    #                         fused conv2-4 / seg_conv2-3 backward, folded seg_conv1 backward
    glds: bool              # signed-W pool forward; pool rows added after the LDS-DMA input gradient
    fp8: bool               # a5 and global_feat's operands in e4m3
    fused12: bool           # seg_conv1 + seg_conv2 forward in one pass (pcs_fwd_seg12)
    trunk32: bool           # eval: conv1..conv4 in fp32, conv5 on a 16-bit split of a4
    gram4_stats: bool       # bn5's statistics from the Gram of a4
    draw_beside_gram: bool  # dropout keep bits drawn beside the Gram of a5, not at the start


def resolve_paths(dtype: str, flags: int = 0, eval_trunk: str = "fp32", fused_seg12: bool = True,
                  draw_beside_gram: bool = True, dropout_draw: str = "paired", *, train: bool, masks_given: bool) -> Paths:
    """The path record of one pass (pure: no library, no device)."""
    bf16 = dtype in ("bf16", "fp8")
    wide_fast = bf16 and not (flags & L.FLAG_GENERIC)
    return Paths(flags=flags, bf16=bf16, wide_fast=wide_fast, glds=wide_fast and not (flags & L.FLAG_NO_GLDS),
                 fp8=dtype == "fp8", fused12=bool(train and wide_fast and fused_seg12),
                 trunk32=not train and bf16 and eval_trunk == "fp32", gram4_stats=bool(train and bf16),
                 draw_beside_gram=bool(train and not masks_given and wide_fast and draw_beside_gram
                                       and dropout_draw != "independent"))


@dataclass
class BNCoef:
    """Per-BN vectors produced by the forward finalisation (all fp32 [C] / [B,C])."""
    mean: torch.Tensor
    rstd: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    scene_sum: torch.Tensor

    def bnrelu(self):
        """The PRO_BNRELU prologue's members of a GEMM that consumes relu(bn(Y))."""
        return dict(pa=self.scale, pb=self.shift)


@dataclass
class Saved:
    """Everything the backward needs from one forward."""
    B: int
    N: int
    train: bool
    paths: Paths = None                           # the kernels this pass took (resolve_paths)
    ys: dict = field(default_factory=dict)        # conv name -> Y tensor [M, C]
    bn: dict = field(default_factory=dict)        # bn name -> BNCoef
    masks: tuple = (None, None)                   # dropout keep bits (seg1 out, seg2 out)
    g: torch.Tensor = None
    am: torch.Tensor = None
    ysel: torch.Tensor = None
    x: torch.Tensor = None
    logits: torch.Tensor = None
    head: dict = None                             # the head's backward buffers (HEAD_CE forward)
    wc: dict = None                               # cast weights used by this pass
    gram4: tuple = None                           # (G, S) of a4 when the forward computed it
    gram2: object = None                          # conv3's per-chunk [G | S] records of a2 (fused seg12)
    a5_colsum: torch.Tensor = None                # bf16: per-chunk column sums of a5 (conv5 epilogue)
    gram5: tuple = None                           # bf16/fp8: (G, per-scene S, workspace) of a5, from the forward
    wg_eff: torch.Tensor = None                   # global_feat's weight as the forward GEMM saw it (fp32)
    sbias_s1: torch.Tensor = None                 # [B, 512] per-scene (centred) bias of the stored seg_conv1 output
    mask_ready: object = None                     # torch.cuda.Event recorded after a side-stream draw of masks


def _f32(dev, *shape):
    return torch.empty(*shape, dtype=torch.float32, device=dev)


def _struct(cls, **members):
    """A C-ABI argument struct; members given as tensors become device pointers (None = NULL)."""
    a = cls()
    for k, v in members.items():
        setattr(a, k, L.ptr(v) if torch.is_tensor(v) else v)
    return a


class _Bwd:
    """Shared state of one backward call.  Buffer placement moves kernel times, so nothing is released
    early: ``keep`` is never pruned, ``st`` is replaced only by the next layer's buffer."""

    def __init__(self, gflat, offsets, bufA):
        self.gflat, self.offsets = gflat, offsets
        self.coefs = {}            # bn -> (alpha, beta, gamma) of dy = alpha dZ + beta + gamma Y
        self.bufA = bufA           # ping-pong dZ buffers [M * 1024]
        self.bufB = None           # (allocated after bn_seg3's coefficients)
        self.keep = []             # alive until the call returns (the allocator is stream-ordered)
        self.st = None             # S1 / S2 partials of the input gradient just computed
        self.keep_scale = 1.0 / (1.0 - DROPOUT_P)

    def G(self, name):
        """The flat gradient buffer from a parameter's slot on."""
        return self.gflat[self.offsets[name]:]


class Engine:
    """Launches the PointNetSegmentation kernels for one compute dtype and device."""

    def __init__(self, num_classes: int, dtype: str = "fp32", input_dim: int = 4, eval_trunk: str = "fp32"):
        check_dims(num_classes, input_dim)
        if eval_trunk not in ("fp32", "bf16"):
            raise ValueError(f"eval_trunk must be 'fp32' or 'bf16', got {eval_trunk!r}")
        self.input_dim = input_dim
        self.C = num_classes
        self.dtype = dtype
        self.dt, self.tdt = _dt(dtype)
        # fp8: conv5 stores a5 as e4m3 and global_feat runs on MX-scaled fp8 MFMA (W rows quantized with one E8M0
        # scale each, pcs_quant_fp8_rows), forward and input gradient
        self.fp8 = dtype == "fp8"
        self.a5_dt = L.FP8 if self.fp8 else self.dt
        # bf16 / fp8 EVAL forward: the narrow trunk conv1..conv4 (<= 128 channels, 10 % of the activation bytes)
        # stored and computed in fp32, conv5 on a 16-bit split of a4 (pcs_bnrelu_bf16); the trained network amplifies
        # the trunk's bf16 rounding into logit-margin error that moves mIoU by > 1e-3.  "bf16"
        # keeps the whole eval forward on bf16 storage (the training step's precision).
        self.eval_trunk = eval_trunk
        self.layout = param_layout(num_classes, input_dim)          # registration order
        self.numel = {n: int(torch.Size(s).numel()) for n, s in self.layout}
        self.offsets, self.total_params = flat_offsets(num_classes, input_dim)   # flat order
        self.buckets = bucket_ranges(num_classes, input_dim)
        self._geo = {}
        self._side = {}   # device -> side stream
        self.flags = 0       # L.FLAG_GENERIC forces the generic GEMM (cross-checks)
        self.timing = None   # dict tag -> [(start, end) torch.cuda.Event] when profiling
        self.timing_tags = None   # set of tags to bracket (None = every tagged launch)
        # test hooks for the global max-pool's rows (P:114): record_pool_rows keeps a copy of the argmax rows [B,
        # 1024] of the last forward in last_pool_rows; pool_rows_override (int32 [B, 1024] global rows) replaces them
        # before the backward routes the pooled gradient, so a bf16 step can be compared with the fp32 step through
        # the same rows (tests/test_gpu_fullsize.py).  Never set on the product path.
        self.record_pool_rows = False
        self.last_pool_rows = None
        self.pool_rows_override = None
        # test hooks for the pre-pool backward at full size (tests/test_gpu_fullsize.py): capture (a dict) receives
        # the operands and outputs of global_feat's input gradient and conv5's backward kernels; perturb = {"dz5":
        # (c0, c1, scale)} scales columns c0..c1 of dz5 after global_feat's input gradient (a simulated kernel error,
        # the negative control); {"a5": (rows, cols, value)} writes value into a5[rows, cols] after conv5's forward (a
        # diverged activation: NaN through the max-pool, tests/test_gpu_pool_nan.py). Never set on the product path.
        self.capture = None
        self.perturb = None
        # bf16 / fp8 training forward: seg_conv1's local half and seg_conv2 in one streaming pass (pcs_fwd_seg12,
        # bn_seg1's statistics from the Gram of a2); False runs the two pcs_gemm passes (cross-checks)
        self.fused_seg12 = True
        # bf16 training step: draw the dropout keep bits beside the Gram of a5 (bounded grid, in its idle VALU issue)
        # instead of at the start of the forward with a full grid
        self.draw_beside_gram = True
        # "paired" (default): pcs_dropout_bits (elements 2k, 2k + 1 share a byte pair of their uniforms);
        # "independent": pcs_dropout_bits_independent, i.i.d. keep bits as nn.Dropout (P:96) at twice the Philox
        # calls, drawn at the start of the forward (parity runs)
        self.dropout_draw = "paired"
        L.load()

    def _launch(self, tag, name, *args):
        """C-ABI call, bracketed by HIP events on the launch stream when timing is on."""
        if self.timing is None or tag is None or (self.timing_tags is not None and tag not in self.timing_tags):
            return L.call(name, *args)
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        r = L.call(name, *args)
        en.record()
        self.timing.setdefault(tag, []).append((st, en))
        return r

    # ------------------------------------------------------------------ helpers
    def _dims(self, sv):
        """(B, N, M, device, stream) of a pass."""
        return sv.B, sv.N, sv.B * sv.N, sv.x.device, L.stream_ptr()

    def _side_stream(self, dev):
        """A per-device HIP stream for work with no data dependence on the trunk (dropout bits)."""
        st = self._side.get(dev)
        if st is None:
            st = self._side.setdefault(dev, torch.cuda.Stream(device=dev))
        return st

    @staticmethod
    def _gemm_args(B, N, K, ncols, dtype, pro=L.PRO_RAW, epi=L.EPI_FWD, cps=0, flags=0, **members):
        return _struct(L.GemmArgs, num_scenes=B, scene_rows=N, K=K, Ncols=ncols, dtype=dtype, prologue=pro,
                       epilogue=epi, chunks_per_scene=cps, flags=flags, **members)

    def geometry(self, B, N, K, ncols, pro=L.PRO_BNRELU, epi=L.EPI_FWD, dtype=None, flags=None):
        """(chunks_per_scene, rows_per_chunk) of the kernel pcs_gemm picks for these args."""
        dtype = self.dt if dtype is None else dtype
        flags = self.flags if flags is None else flags
        key = (B, N, K, ncols, pro, epi, flags, dtype)
        if key not in self._geo:
            a = self._gemm_args(B, N, K, ncols, dtype, pro, epi, 0, flags)
            rpc = L.workspace("pcs_gemm_geometry", a)
            self._geo[key] = (a.chunks_per_scene, rpc)
        return self._geo[key]

    def _empty(self, *shape, dtype=None, device):
        return torch.empty(*shape, dtype=dtype or self.tdt, device=device)

    def cast_weights(self, P):
        """fp32 parameters -> compute-dtype W and W^T copies (every call: params may change)."""
        dev = P["conv2.weight"].device
        wc = {}
        s = L.stream_ptr()
        for conv, cin, cout, _ in CONVS:
            if conv in ("conv1", "seg_conv4"):
                continue
            W = P[f"{conv}.weight"]
            rows, ld = W.shape[0], W.shape[1]
            cols = 64 if conv == "seg_conv1" else ld     # seg_conv1: local half only
            Wc = self._empty(rows, cols, device=dev)
            WcT = self._empty(cols, rows, device=dev)
            L.call("pcs_cast_weight", W, rows, cols, ld, self.dt, Wc, WcT, s)
            wc[conv] = (Wc, WcT)
        if self.fp8:
            wc["global_feat_fp8"] = self._quant_fp8(P["global_feat.weight"])
        return wc

    def _quant_fp8(self, W):
        """(e4m3 rows, E8M0 row scales, fp32 dequantized copy) of an fp32 [rows, cols(, 1)] matrix."""
        W = W.reshape(W.shape[0], -1)
        rows, cols = W.shape
        dev = W.device
        Wq = torch.empty(rows, cols, dtype=torch.uint8, device=dev)
        sc = torch.empty(rows, dtype=torch.uint8, device=dev)
        deq = _f32(dev, rows, cols)
        L.call("pcs_quant_fp8_rows", W, rows, cols, W.stride(0), Wq, sc, deq, L.stream_ptr())
        return Wq, sc, deq

    def _bn_finalize(self, P, bufs, sv, bnname, stats, C, cps, rpc, offset=None):
        """BN coefficients for stored activations that omit ``offset`` (the conv bias)."""
        B, N, _, dev, _ = self._dims(sv)
        coef = BNCoef(*(_f32(dev, C) for _ in range(4)), _f32(dev, B, C))
        g, b = P[f"{bnname}.weight"], P[f"{bnname}.bias"]
        if sv.train:
            rm, rv = bufs.get(f"{bnname}.running_mean"), bufs.get(f"{bnname}.running_var")
            upd = int(rm is not None and rv is not None)
            L.call("pcs_bn_fwd_finalize", stats, B, N, C, cps, rpc, g, b, offset, rm, rv, BN_MOMENTUM, BN_EPS, upd,
                   coef.mean, coef.rstd, coef.scale, coef.shift, coef.scene_sum, L.stream_ptr())
        else:
            L.call("pcs_bn_eval_coefs", g, b, bufs[f"{bnname}.running_mean"], bufs[f"{bnname}.running_var"], offset,
                   BN_EPS, C, coef.scale, coef.shift, L.stream_ptr())
        return coef

    def _gemm(self, sv, K, ncols, pro, epi, A, W, C, *, tag=None, dtype=None, extra_flags=0, **fields):
        """One pcs_gemm of the pass ``sv``; ``fields`` as in _gemm_args."""
        dtype = self.dt if dtype is None else dtype
        flags = sv.paths.flags
        cps, _ = self.geometry(sv.B, sv.N, K, ncols, pro, epi, dtype, flags)
        fields.setdefault("a_keep_scale", 1.0)
        fields.setdefault("c_keep_scale", 1.0)
        a = self._gemm_args(sv.B, sv.N, K, ncols, dtype, pro, epi, cps, flags | extra_flags, A=A, W=W, C=C, **fields)
        self._launch(tag, "pcs_gemm", a, L.stream_ptr())

    def _wgrad_args(self, sv, cout, cin, dy_mode, x_mode, dW, ldw=0, x_keep_scale=1.0, **members):
        return _struct(L.WgradArgs, num_scenes=sv.B, scene_rows=sv.N, Cout=cout, Cin=cin, dtype=self.dt, dy_mode=dy_mode,
                       x_mode=x_mode, x_keep_scale=x_keep_scale, dW=dW, ldw=ldw, flags=sv.paths.flags, **members)

    def _wgrad(self, sv, cout, cin, dy_mode, x_mode, dW, conv1=False, tag=None, **kw):
        a = self._wgrad_args(sv, cout, cin, dy_mode, x_mode, dW, **kw)
        if conv1:
            a.splits_per_scene = max(1, min((1024 + sv.B - 1) // sv.B, (sv.N + 255) // 256))
            nbytes = sv.B * a.splits_per_scene * cout * cin * 4
        else:
            nbytes = L.workspace("pcs_wgrad_workspace", a)
        ws = _f32(dW.device, max(nbytes // 4, 1))
        a.partial = ws.data_ptr()
        self._launch(tag, "pcs_conv1_wgrad" if conv1 else "pcs_wgrad", a, L.stream_ptr())
        return ws  # keep alive until the stream consumes it (caching allocator is stream-ordered)

    def _rounded(self, W):
        """fp32 copy of W as the forward's compute-dtype GEMM saw it (pcs_round_weight)."""
        if self.dt == L.F32:
            return W
        out = torch.empty_like(W)
        L.call("pcs_round_weight", W, W.numel(), self.dt, out, L.stream_ptr())
        return out

    def _gram(self, Y, s_, t_, B, N, C, tag=None):
        """(G, S) = (a^T a, column sums of a) for a = relu(Y*s + t) (pcs_gram)."""
        dev = Y.device
        G, S = _f32(dev, C, C), _f32(dev, C)
        sps = ct.c_int32(0)
        nbytes = L.workspace("pcs_gram_workspace", B, N, C, self.dt, ct.byref(sps))
        ws = _f32(dev, max(nbytes // 4, 1))
        self._launch(tag, "pcs_gram", Y, s_, t_, B, N, C, self.dt, sps.value, ws, G, S, L.stream_ptr())
        return G, S, ws

    def _gram_raw(self, a5, G, beside=None):
        """G = a5^T a5 of the stored (post-ReLU) a5, read raw on the LDS-DMA kernel (pcs_gram_raw; the column sums
        come from conv5's epilogue).  ``beside()`` runs once the workspace is allocated, just ahead of the
        launch.  Returns the workspace."""
        M = a5.shape[0]
        nbytes = L.workspace("pcs_gram_raw_workspace", M, 1024)
        ws = _f32(a5.device, nbytes // 4)
        if beside is not None:
            beside()
        self._launch("wgrad:global_feat", "pcs_gram_raw", a5, M, 1024, self.a5_dt, ws, nbytes, G, L.stream_ptr())
        return ws

    # ------------------------------------------------------------------ forward
    def forward(self, P, bufs, x, *, train, masks=None, seed=0, head_mode=L.HEAD_FWD,
                labels=None, class_weight=None, wsum=None, want_logits=True, saved=None):
        """Forward pass.  P: name -> fp32 parameter tensor; bufs: BN running buffers.

        ``masks`` = (bits1 [M,64] u8, bits2 [M,32] u8) replays dropout keep bits; otherwise
        train mode draws them with Philox from ``seed``.  With ``head_mode=HEAD_CE`` the
        head kernel also computes the weighted CE loss and starts the backward (fused
        train step); returns the Saved context (plus head outputs in ``saved.head``).
        """
        if not x.is_cuda:
            raise RuntimeError("pcs_amd runs on a HIP device only (no CPU fallback)")
        B, N, D = x.shape
        if D != self.input_dim:
            raise ValueError(f"expected x of shape (B, N, {self.input_dim}), got {tuple(x.shape)}")
        x = x.contiguous().float()
        sv = Saved(B=B, N=N, train=train) if saved is None else saved
        sv.B, sv.N, sv.train, sv.x = B, N, train, x
        sv.gram4 = None   # (a reused Saved must not carry the previous pass's Gram)
        sv.paths = pt = resolve_paths(self.dtype, self.flags, self.eval_trunk, self.fused_seg12, self.draw_beside_gram,
                                      self.dropout_draw, train=train, masks_given=masks is not None)
        # name -> a stage's temporary that stays allocated until the forward returns, or until
        # the name is assigned again (the allocation pattern is pinned, see _Bwd)
        live = {}
        if train and masks is None and not pt.draw_beside_gram:
            self._draw_masks(sv, seed)
        sv.wc = self.cast_weights(P)
        self._trunk(P, bufs, sv)
        self._conv5(P, bufs, sv, live)
        self._global_feat(P, bufs, sv, live, seed)
        self._seg(P, bufs, sv, live, masks)
        # head: seg_conv4 (+ CE and the start of the backward when fused)
        sv.logits = _f32(x.device, B, N, self.C) if want_logits else None
        if head_mode == L.HEAD_CE:
            sv.head = self._head(P, sv, L.HEAD_CE, labels=labels, class_weight=class_weight, wsum=wsum)
        else:
            self._head(P, sv, L.HEAD_FWD)
        return sv

    def _draw_masks(self, sv, seed, max_wg=0):
        """Philox keep bits (ALU-bound, no data dependence) drawn on a side stream beside the trunk's kernels; the
        stream waits for everything enqueued before (the buffers may reuse memory the previous kernels still read) and
        seg_conv2 waits for it."""
        _, _, M, dev, _ = self._dims(sv)
        sv.masks = m1, m2 = tuple(torch.empty(M, w, dtype=torch.uint8, device=dev) for w in (64, 32))
        side = self._side_stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            ss = L.stream_ptr()
            for i, (m, width) in enumerate(((m1, 512), (m2, 256))):
                if self.dropout_draw == "independent":
                    L.call("pcs_dropout_bits_independent", seed, i, M, width, DROPOUT_P, m, ss)
                else:
                    L.call("pcs_dropout_bits_bounded", seed, i, M, width, DROPOUT_P, m, max_wg, ss)
            sv.mask_ready = torch.cuda.Event()
            sv.mask_ready.record(side)
        m1.record_stream(side)
        m2.record_stream(side)

    def _stats_buf(self, sv, K, ncols):
        """(per-chunk BN statistics buffer, chunks per scene, rows per chunk) of a forward GEMM."""
        cps, rpc = self.geometry(sv.B, sv.N, K, ncols, flags=sv.paths.flags)
        return _f32(sv.x.device, sv.B * cps, ncols, 2), cps, rpc

    def _bridge(self, sv, conv, bn, K, split):
        """relu(bn(Y)) of an fp32 trunk output as bf16 (split: [hi | lo], pcs_bnrelu_bf16)."""
        _, _, M, dev, s = self._dims(sv)
        out = self._empty(M, 2 * K if split else K, device=dev)
        c = sv.bn[bn]
        L.call("pcs_bnrelu_bf16", sv.ys[conv], M, K, c.scale, c.shift, int(split), out, s)
        return out

    def _layer(self, P, bufs, sv, conv, src, offset=None, A_raw=None, K=None, **kw):
        """Y = conv(relu(bn(Y_src))) with its BN statistics and coefficients (``offset``: the conv bias by
        default).  ``dtype=L.F32``: the eval path's fp32 trunk (fp32 weights); ``A_raw``: a bf16 activation bridged
        from that trunk, read as it is; ``K``: the columns of W to use."""
        M, dev = sv.B * sv.N, sv.x.device
        cin, ncols, bnname = _LAYERS[conv]
        K = K or cin
        st, cps, rpc = self._stats_buf(sv, K, ncols) if sv.train else (None, 0, 0)
        f32 = kw.get("dtype") == L.F32
        y = self._empty(M, ncols, device=dev, dtype=torch.float32 if f32 else None)
        W = P[f"{conv}.weight"] if f32 else sv.wc[conv][0]
        pro, A = L.PRO_RAW, A_raw
        if A_raw is None:
            pro, A = L.PRO_BNRELU, sv.ys[src]
            kw.update(sv.bn[_LAYERS[src][2]].bnrelu())
        self._gemm(sv, K, ncols, pro, L.EPI_FWD, A, W, y, stats=st, tag=f"fwd:{conv}", **kw)
        sv.ys[conv] = y
        sv.bn[bnname] = self._bn_finalize(P, bufs, sv, bnname, st, ncols, cps, rpc,
                                          P[f"{conv}.bias"] if offset is None else offset)

    def _trunk(self, P, bufs, sv):
        """conv1..conv4 (P:105-109).  Stored pre-BN activations omit the conv bias (BN cancels it exactly; it only
        shifts running_mean), which keeps them centred: full precision in fp32/bf16.  bf16 / fp8 eval: in fp32
        (self.eval_trunk, see __init__)."""
        B, N, M, dev, s = self._dims(sv)
        pt, train, D = sv.paths, sv.train, self.input_dim
        # conv1 (K=4), on the generic 128-row geometry
        y1 = self._empty(M, 64, device=dev, dtype=torch.float32 if pt.trunk32 else None)
        a = self._gemm_args(B, N, D, 64, L.F32, flags=L.FLAG_GENERIC)
        rpc, cps = L.workspace("pcs_gemm_geometry", a), a.chunks_per_scene
        st = _f32(dev, B * cps, 64, 2) if train else None
        a = self._gemm_args(B, N, D, 64, L.F32 if pt.trunk32 else self.dt, cps=cps, A=sv.x,
                            W=P["conv1.weight"], C=y1, bias=None, stats=st)
        self._launch("fwd:conv1", "pcs_conv1_fwd", a, s)
        sv.ys["conv1"] = y1
        sv.bn["bn1"] = self._bn_finalize(P, bufs, sv, "bn1", st, 64, cps, rpc, P["conv1.bias"])
        tkw = {"dtype": L.F32} if pt.trunk32 else {}
        self._layer(P, bufs, sv, "conv2", "conv1", **tkw)
        # the fused seg_conv1 + seg_conv2 forward takes bn_seg1's statistics from the Gram of a2,
        # which conv3's streaming pass forms from the operand it already has in LDS
        if pt.fused12:
            sv.gram2 = _f32(dev, B * self.geometry(B, N, 64, 64, flags=pt.flags)[0], 64 * 64 + 64)
        self._layer(P, bufs, sv, "conv3", "conv2", **tkw, **({"gram": sv.gram2} if pt.fused12 else {}))
        self._layer(P, bufs, sv, "conv4", "conv3", **tkw)

    def _conv5(self, P, bufs, sv, live):
        """conv5 (P:110): bn5's statistics first, then the GEMM with bn5 + ReLU applied in the epilogue, storing a5 =
        relu(bn5(y5)) for global_feat.  fp32: a statistics-only pass of the GEMM.  bf16: from the Gram of a4 (which
        conv5's weight gradient needs anyway), mean = W5 S4 / M and M2 = w (G4 - S4 S4^T / M) w^T per channel."""
        B, N, M, dev, s = self._dims(sv)
        pt, train, W5 = sv.paths, sv.train, sv.wc["conv5"][0]
        st, cps, rpc = (None, 0, 0)
        if pt.gram4_stats:
            c4 = sv.bn["bn4"]
            sv.gram4 = self._gram(sv.ys["conv4"], c4.scale, c4.shift, B, N, 128, tag="fwd_stats:conv5")
            st, cps, rpc = _f32(dev, B, 1024, 2), 1, N
            L.call("pcs_bn_stats_from_gram", sv.gram4[0], sv.gram4[1], M, W5, self.dt, 128, 1024, 128, B, st, s)
        elif train:
            st, cps, rpc = self._stats_buf(sv, 128, 1024)
            self._gemm(sv, 128, 1024, L.PRO_BNRELU, L.EPI_FWD, sv.ys["conv4"], W5, None,
                       stats=st, tag="fwd_stats:conv5", **sv.bn["bn4"].bnrelu())
        live["stats"] = st   # (released when global_feat's statistics buffer replaces it)
        sv.bn["bn5"] = c5 = self._bn_finalize(P, bufs, sv, "bn5", st, 1024, cps, rpc, P["conv5.bias"])
        a5 = self._empty(M, 1024, device=dev, dtype=torch.uint8 if pt.fp8 else None)
        # bf16: the epilogue also sums a5's columns per chunk (S of global_feat's Gram-form
        # weight gradient; the LDS-DMA Gram kernel computes G only)
        sv.a5_colsum = None
        if train and pt.wide_fast:
            cps5c, _ = self.geometry(B, N, 128, 1024, L.PRO_BNRELU, L.EPI_BNRELU, flags=pt.flags)
            sv.a5_colsum = _f32(dev, B * cps5c, 1024, 2)
        kw = dict(es=c5.scale, et=c5.shift, tag="fwd:conv5", extra_flags=L.FLAG_C_FP8 if pt.fp8 else 0)
        if pt.trunk32:
            # a4 to 16 significant bits: [hi | lo] (K = 256) against [W5 | W5]
            live["W5s"] = W5s = torch.cat([W5, W5], dim=1)
            self._gemm(sv, 256, 1024, L.PRO_RAW, L.EPI_BNRELU, self._bridge(sv, "conv4", "bn4", 128, True), W5s, a5,
                       **kw)
        else:
            self._gemm(sv, 128, 1024, L.PRO_BNRELU, L.EPI_BNRELU, sv.ys["conv4"], W5, a5, stats=sv.a5_colsum,
                       **kw, **sv.bn["bn4"].bnrelu())
        if self.perturb is not None and "a5" in self.perturb:   # test hook: before anything reads a5
            rows, cols, value = self.perturb["a5"]
            if pt.fp8:   # e4m3 bytes: 0x7f is its NaN
                a5[rows, cols] = 0x7f if value != value else int(torch.tensor(value).to(torch.float8_e4m3fn).view(torch.uint8))
            else:
                a5[rows, cols] = value
        sv.ys["a5"] = a5

    def _global_gram_stats(self, P, sv, live, seed):
        """bf16 / fp8 training: bn_global's statistics from the Gram of a5 -- computed here rather than in the
        backward, whose Gram-form weight gradient reuses it -- and conv5's per-chunk column sums
        (pcs_bn_stats_from_gram_scenes).  The dropout draw goes beside the Gram, MFMA-bound at 214 / 216 VGPRs x 2
        waves per SIMD, with three 256-thread workgroups per CU (24 VGPRs a wave: they fit beside it and use its idle
        VALU issue; 0.77 ms per call against 0.83 with two, the Gram and the step unchanged, tools/draw_wg.py)."""
        B, N, _, dev, s = self._dims(sv)
        pt, a5 = sv.paths, sv.ys["a5"]
        Wg = P["global_feat.weight"].reshape(1024, -1)
        sv.wg_eff = sv.wc["global_feat_fp8"][2] if pt.fp8 else self._rounded(Wg)
        G5 = _f32(dev, 1024, 1024)
        max_wg = 3 * torch.cuda.get_device_properties(dev).multi_processor_count
        gws = self._gram_raw(a5, G5, beside=(lambda: self._draw_masks(sv, seed, max_wg)) if pt.draw_beside_gram else None)
        # per-scene column sums of a5 from conv5's per-chunk partials (chunks are scene-aligned)
        live["Sb2"] = Sb2 = _f32(dev, B, 1024, 2)
        L.call("pcs_reduce_partials_grouped", sv.a5_colsum, B, sv.a5_colsum.shape[0] // B, 2048, 1.0, Sb2, s)
        Sb = Sb2[..., 0].contiguous()
        live["stats"] = st = _f32(dev, B, 1024, 2)
        qbytes = L.workspace("pcs_bn_stats_from_gram_scenes_workspace", 1024, 1024)
        live["qws"] = qws = torch.empty(qbytes // 8, dtype=torch.float64, device=dev)
        self._launch("stats:global_feat", "pcs_bn_stats_from_gram_scenes", G5, Sb, N, sv.wg_eff,
                     L.F32, 1024, 1024, 1024, B, qws, qbytes, st, s)
        sv.gram5 = (G5, Sb, gws)

    def _global_feat(self, P, bufs, sv, live, seed):
        """global_feat (P:113-114): a5 W^T with max-pool partials (and, on the fp32 / generic paths, BN statistics) in
        the epilogue; the 1024-wide output itself is never stored. With Gram-derived statistics (_global_gram_stats)
        the LDS-DMA forward runs the max-pool epilogue only."""
        B, N, _, dev, s = self._dims(sv)
        pt, wc, a5 = sv.paths, sv.wc, sv.ys["a5"]
        cps_g, rpc_g = self.geometry(B, N, 1024, 1024, L.PRO_RAW, L.EPI_FWD, flags=pt.flags)
        live["pool"] = pool = _f32(dev, B * cps_g, 1024, 4)
        sv.gram5 = None
        if sv.train and pt.wide_fast:
            self._global_gram_stats(P, sv, live, seed)
            st_g, cps_st, rpc_st = None, 1, N
        else:
            live["stats"] = st_g = _f32(dev, B * cps_g, 1024, 2) if sv.train else None
            cps_st, rpc_st = cps_g, rpc_g
        # (es = bn_global's gamma: its sign tells the pool which extremum pcs_pool_finalize uses;
        # without statistics on the LDS-DMA kernel, W's rows come pre-multiplied by that sign,
        # PCS_FLAG_POOL_SIGNED_W, and the pool keeps a plain column max)
        gamma_g = P["bn_global.weight"]
        Wf, kw = wc["global_feat"][0], dict(extra_flags=0)
        if pt.fp8:
            Wf, kw = wc["global_feat_fp8"][0], dict(w_scale=wc["global_feat_fp8"][1], extra_flags=L.FLAG_AW_FP8)
        if st_g is None and pt.glds:
            live["Wsg"] = Wsg = torch.empty_like(Wf)
            L.call("pcs_sign_rows", Wf, self.a5_dt, 1024, 1024, gamma_g, Wsg, s)
            Wf, kw["extra_flags"] = Wsg, kw["extra_flags"] | L.FLAG_POOL_SIGNED_W
        self._gemm(sv, 1024, 1024, L.PRO_RAW, L.EPI_FWD, a5, Wf, None, stats=st_g, pool=pool, es=gamma_g,
                   tag="fwd:global_feat", **kw)
        sv.bn["bn_global"] = cg = self._bn_finalize(P, bufs, sv, "bn_global", live["stats"], 1024, cps_st, rpc_st,
                                                    P["global_feat.bias"])
        sv.g = _f32(dev, B, 1024)
        sv.am = torch.empty(B, 1024, dtype=torch.int32, device=dev)
        sv.ysel = _f32(dev, B, 1024)
        L.call("pcs_pool_finalize", pool, B, N, 1024, cps_g, cg.scale, cg.shift, sv.g, sv.am, sv.ysel, s)
        if self.record_pool_rows:              # test hooks: the max-pool's rows
            self.last_pool_rows = sv.am.clone()
        if self.pool_rows_override is not None:
            sv.am.copy_(self.pool_rows_override)

    def _masks(self, sv, masks):
        """(keep bits after bn_seg1, after bn_seg2, keep scale) of the pass (P:124, P:126)."""
        _, _, M, dev, _ = self._dims(sv)
        m1 = m2 = None
        if sv.train and masks is not None:
            m1, m2 = masks
            # the kernels read M x 512 / M x 256 keep bits: a mask for another batch
            # shape (e.g. a DataParallel replica's chunk) would be read out of bounds
            if any(tuple(m.shape) != (M, w) or m.dtype != torch.uint8 or m.device != dev for m, w in ((m1, 64), (m2, 32))):
                raise ValueError(f"dropout masks must be uint8 [{M}, 64] and [{M}, 32] on {dev}, got "
                                 f"{tuple(m1.shape)} {m1.dtype} and {tuple(m2.shape)} {m2.dtype}")
            m1, m2 = m1.contiguous(), m2.contiguous()
        elif sv.train:
            m1, m2 = sv.masks
            torch.cuda.current_stream(dev).wait_event(sv.mask_ready)   # drawn on the side stream
        sv.masks = (m1, m2)
        return m1, m2, 1.0 / (1.0 - DROPOUT_P) if sv.train else 1.0

    def _seg(self, P, bufs, sv, live, masks):
        """seg_conv1 = local 64->512 GEMM + per-scene bias (W_global . g_b + b), seg_conv2 and seg_conv3 behind the
        dropouts (P:117-127).  The per-scene bias is centred over the scenes; its mean joins the BN offset."""
        B, _, _, dev, s = self._dims(sv)
        pt = sv.paths
        sbias = _f32(dev, B, 512)
        live["soff"] = soff = _f32(dev, 512)
        Ws1 = P["seg_conv1.weight"]
        L.call("pcs_scene_gemv", sv.g, B, 1024, Ws1, Ws1.shape[1], 64, P["seg_conv1.bias"], 512, sbias, soff, s)
        sv.sbias_s1 = sbias   # the stored Y'_seg1 = a2 W_l^T + sbias[b] (the folded backward)
        if not pt.fused12:    # (fused: with seg_conv2 below, pcs_fwd_seg12)
            self._layer(P, bufs, sv, "seg_conv1", "conv2", soff, K=64, scene_bias=sbias,
                        A_raw=self._bridge(sv, "conv2", "bn2", 64, False) if pt.trunk32 else None)
        m1, m2, keep = self._masks(sv, masks)
        if pt.fused12:
            self._seg12(P, bufs, sv, sv.wc, sbias, soff, m1, keep)
        else:
            self._layer(P, bufs, sv, "seg_conv2", "seg_conv1", a_mask=m1, a_keep_scale=keep)
        self._layer(P, bufs, sv, "seg_conv3", "seg_conv2", a_mask=m2, a_keep_scale=keep)

    def _seg12(self, P, bufs, sv, wc, sbias, soff, m1, keep):
        """seg_conv1 (local half + scene bias) and seg_conv2 forward in one pass (P:117-125; pcs_fwd_seg12).  bn_seg1's
        batch statistics come first, from the Gram of a2 = relu(bn2(y2)) and its per-scene column sums (pcs_gram,
        pcs_bn_stats_gram_sbias), with the bf16-rounded W_l the pass multiplies by."""
        B, N, M, dev, s = self._dims(sv)
        c2 = sv.bn["bn2"]
        # conv3's per-chunk [G | S] records of a2 -> per scene, then G2 over the scenes
        rec = 64 * 64 + 64
        cps3 = sv.gram2.shape[0] // B
        per_scene = _f32(dev, B, rec)
        L.call("pcs_reduce_partials_grouped", sv.gram2, B, cps3, rec, 1.0, per_scene, s)
        tot = _f32(dev, rec)
        L.call("pcs_reduce_partials", per_scene, B, rec, 1.0, tot, 1, rec, s)
        G2 = tot[:64 * 64]
        Sb = per_scene[:, 64 * 64:].contiguous()
        Ws1 = P["seg_conv1.weight"]
        Ws1_r = self._rounded(Ws1)
        st1 = _f32(dev, B, 512, 2)
        L.call("pcs_bn_stats_gram_sbias", G2, Sb, B, N, Ws1_r, Ws1.shape[1], 64, 512, sbias, st1, s)
        sv.bn["bn_seg1"] = c1 = self._bn_finalize(P, bufs, sv, "bn_seg1", st1, 512, 1, N, soff)
        y1, y2 = self._empty(M, 512, device=dev), self._empty(M, 256, device=dev)
        a = _struct(L.Seg12Args, num_scenes=B, scene_rows=N, y2=sv.ys["conv2"], s2=c2.scale, t2=c2.shift,
                    W1=wc["seg_conv1"][0], sbias=sbias, Y1=y1, s1=c1.scale, t1=c1.shift, keep1=m1, keep_scale=keep,
                    W2=wc["seg_conv2"][0], Y2=y2)
        rpc, cps = L.workspace("pcs_fwd_seg12_geometry", a), a.chunks_per_scene
        st2 = _f32(dev, B * cps, 256, 2)
        a.stats = L.ptr(st2)
        self._launch("fwd:seg_conv1+2", "pcs_fwd_seg12", a, s)
        sv.ys["seg_conv1"], sv.ys["seg_conv2"] = y1, y2
        sv.bn["bn_seg2"] = self._bn_finalize(P, bufs, sv, "bn_seg2", st2, 256, cps, rpc, P["seg_conv2.bias"])

    def _head(self, P, sv, mode, labels=None, class_weight=None, wsum=None, dlogits=None):
        """seg_conv4 + (CE | given dlogits) + head backward; returns the backward buffers."""
        B, N, _, dev, s = self._dims(sv)
        c3 = sv.bn["bn_seg3"]
        ha = _struct(L.HeadArgs, num_scenes=B, scene_rows=N, Cin=128, num_classes=self.C, dtype=self.dt, mode=mode,
                     Y=sv.ys["seg_conv3"], s=c3.scale, t=c3.shift, W=P["seg_conv4.weight"], bias=P["seg_conv4.bias"],
                     logits=sv.logits if mode != L.HEAD_BWD else None)
        hb = None
        if mode != L.HEAD_FWD:
            L.workspace("pcs_head_geometry", ha)
            nch = B * ha.chunks_per_scene
            hb = dict(dZ=torch.empty(B * N * 1024, dtype=self.tdt, device=dev), stats=_f32(dev, nch, 128, 2),
                      wpartial=_f32(dev, nch, self.C * 129), loss_partial=_f32(dev, nch), cps=ha.chunks_per_scene,
                      nch=nch)
            ha.dZ, ha.stats = L.ptr(hb["dZ"]), L.ptr(hb["stats"])
            ha.wpartial, ha.loss_partial = L.ptr(hb["wpartial"]), L.ptr(hb["loss_partial"])
            ha.mean, ha.rstd = L.ptr(c3.mean), L.ptr(c3.rstd)
        if mode == L.HEAD_CE:
            ha.labels, ha.class_weight, ha.wsum = L.ptr(labels), L.ptr(class_weight), L.ptr(wsum)
        if mode == L.HEAD_BWD:
            dl = dlogits.reshape(B * N, self.C) if dlogits.dim() == 3 else dlogits
            if dl.dtype != torch.float32:
                dl = dl.float()
            ha.dlogits = L.ptr(dl)
            ha.dl_stride_row, ha.dl_stride_col = dl.stride(0), dl.stride(1)
            hb["dl"] = dl
        self._launch(f"head:{mode}", "pcs_head", ha, s)
        return hb

    # ------------------------------------------------------------------ backward
    def backward(self, P, sv, gflat, dlogits=None, on_bucket=None):
        """Backward pass: every parameter gradient is written into the flat fp32 buffer ``gflat`` (flat order, see
        flat_layout).  Uses the head buffers of a fused CE forward, or runs the head backward on caller-supplied
        ``dlogits``.  ``on_bucket(name)`` is called as soon as the kernels writing gradient bucket ``name``
        (bucket_ranges) have been enqueued, so a data-parallel caller can start its all-reduce there."""
        bucket = on_bucket or (lambda name: None)
        if not sv.train:
            raise RuntimeError("backward needs a train-mode forward (BatchNorm batch statistics)")
        hb = self._head(P, sv, L.HEAD_BWD, dlogits=dlogits) if dlogits is not None else sv.head
        bw = _Bwd(gflat, self.offsets, hb["dZ"])
        scene_s1 = self._bwd_seg32(P, sv, bw, hb)
        sp = self._bwd_pool(P, sv, bw, scene_s1)
        dA2 = self._bwd_seg1_local(P, sv, bw)
        bucket("seg")
        Wg_r, st5, cps5 = self._bwd_global_dgrad(P, sv, bw, sp)
        self._bwd_global_wgrad(P, sv, bw, sp, Wg_r)
        bucket("global")
        self._bwd_conv5(P, sv, bw, st5, cps5)
        self._bwd_trunk(P, sv, bw, dA2)
        bucket("tail")
        return hb

    def _bn_bwd(self, P, sv, bw, bnname, conv, stats, cps, scene_s1=None):
        """bn's (alpha, beta, gamma) into bw.coefs; its and the conv bias's gradients."""
        B, N, _, dev, s = self._dims(sv)
        fc = sv.bn[bnname]
        C = fc.mean.shape[0]
        al, be, ga = (_f32(dev, C) for _ in range(3))
        L.call("pcs_bn_bwd_finalize", stats, B, N, C, cps, fc.mean, fc.rstd, P[f"{bnname}.weight"], fc.scene_sum, al,
               be, ga, bw.G(f"{bnname}.weight"), bw.G(f"{bnname}.bias"), bw.G(f"{conv}.bias"), scene_s1, s)
        bw.coefs[bnname] = (al, be, ga)

    def _wgrad_bn(self, sv, bw, conv, dz, prev, x_mask=None, cin=None, ldw=0):
        """conv's weight gradient from dy = alpha dZ + beta + gamma Y and its input relu(bn(Y_prev)) (pcs_wgrad)."""
        al, be, ga = bw.coefs[_LAYERS[conv][2]]
        pc = sv.bn[_LAYERS[prev][2]]
        bw.keep.append(self._wgrad(
            sv, _LAYERS[conv][1], cin or _LAYERS[conv][0], L.PRO_BWD, L.PRO_BNRELU, bw.G(f"{conv}.weight"), ldw=ldw,
            tag=f"wgrad:{conv}", dZ=dz, Y=sv.ys[conv], alpha=al, beta=be, gamma=ga, X=sv.ys[prev], s=pc.scale,
            t=pc.shift, x_mask=x_mask, x_keep_scale=bw.keep_scale if x_mask is not None else 1.0))

    def _bwd_layer(self, P, sv, bw, conv, dz, prev, out, c_mask=None, addend=None, per_scene=False):
        """Both gradients of layer ``conv`` (dz -> out) in one pass (csrc/fused_bwd.hip) where the fused kernel covers
        the shape (bf16), otherwise the pcs_gemm(DGRAD) + pcs_wgrad pair; then the BatchNorm of ``prev``
        backward.  Returns that BN's per-scene S1 (``per_scene``)."""
        B, N, _, dev, s = self._dims(sv)
        pt, WT = sv.paths, sv.wc[conv][1]
        cin, cout, bn = _LAYERS[conv]
        al, be, ga = bw.coefs[bn]
        pc = sv.bn[_LAYERS[prev][2]]
        f = dict(A2=sv.ys[conv], pa=al, pb=be, pc=ga, Yp=sv.ys[prev], es=pc.scale, et=pc.shift, emean=pc.mean,
                 erstd=pc.rstd, c_mask=c_mask, c_keep_scale=bw.keep_scale if c_mask is not None else 1.0, addend=addend)
        nbytes = -1
        if pt.wide_fast:
            a = self._gemm_args(B, N, cout, cin, self.dt, L.PRO_BWD, L.EPI_DGRAD, 0, pt.flags, A=dz, W=WT, C=out,
                                a_keep_scale=1.0, **f)
            # the one unchecked size query: a negative return means "not this kernel's shape"
            nbytes = L.load().pcs_dgrad_wgrad_bn_workspace(ct.byref(a))
        if nbytes > 0:
            cps = a.chunks_per_scene
            st = _f32(dev, B * cps, cin, 2)
            ws = _f32(dev, nbytes // 4)
            a.stats = L.ptr(st)
            self._launch(f"dgrad+wgrad:{conv}", "pcs_dgrad_wgrad_bn", a, ws, bw.G(f"{conv}.weight"), 0, s)
            bw.keep.append(ws)
        else:
            cps, _ = self.geometry(B, N, cout, cin, L.PRO_BWD, L.EPI_DGRAD, flags=pt.flags)
            st = _f32(dev, B * cps, cin, 2)
            self._gemm(sv, cout, cin, L.PRO_BWD, L.EPI_DGRAD, dz, WT, out, stats=st, tag=f"dgrad:{conv}", **f)
            self._wgrad_bn(sv, bw, conv, dz, prev, x_mask=c_mask)
        bw.st = st   # (the previous layer's statistics are released only now)
        scene_s1 = _f32(dev, B, pc.mean.shape[0]) if per_scene else None
        self._bn_bwd(P, sv, bw, _LAYERS[prev][2], prev, st, cps, scene_s1)
        return scene_s1

    def _bwd_seg32(self, P, sv, bw, hb):
        """seg_conv4's gradient from the head's partials, then seg_conv3 and seg_conv2 (inputs:
        dropout(relu(bn_seg2(y_s2))), dropout(relu(bn_seg1(y_s1)))); returns bn_seg1's per-scene S1."""
        _, _, M, dev, s = self._dims(sv)
        m1, m2 = sv.masks
        # seg_conv4: weight and bias are adjacent in the flat buffer
        L.call("pcs_reduce_partials", hb["wpartial"], hb["nch"], self.C * 129, 1.0, bw.G("seg_conv4.weight"),
               self.C * 129, self.C * 129, s)
        self._bn_bwd(P, sv, bw, "bn_seg3", "seg_conv3", hb["stats"], hb["cps"])
        bw.bufB = torch.empty(M * 1024, dtype=self.tdt, device=dev)
        self._bwd_layer(P, sv, bw, "seg_conv3", bw.bufA, "seg_conv2", bw.bufB, c_mask=m2)
        return self._bwd_layer(P, sv, bw, "seg_conv2", bw.bufB, "seg_conv1", bw.bufA, c_mask=m1, per_scene=True)

    def _bwd_pool(self, P, sv, bw, scene_s1):
        """repeat/cat + max-pool + bn_global backward (P:113-120, pcs_pool_bwd): bn_global's coefficients into
        bw.coefs; returns the pooled rows' coefficients sp [B, 1024]."""
        B, N, _, dev, s = self._dims(sv)
        a1, b1, g1 = bw.coefs["bn_seg1"]
        cg = sv.bn["bn_global"]
        bw.coefs["bn_global"] = ag, bg, gg = tuple(_f32(dev, 1024) for _ in range(3))
        sp = _f32(dev, B, 1024)
        csum = _f32(dev, B, 512)
        Ws1 = P["seg_conv1.weight"]
        pa = _struct(L.PoolBwdArgs, num_scenes=B, scene_rows=N, Cs=512, Cg=1024, col_off=64, s1_alpha=a1, s1_beta=b1,
                     s1_gamma=g1, s1_scene_s1=scene_s1, s1_scene_sum=sv.bn["bn_seg1"].scene_sum, W_s1=Ws1,
                     ldw=Ws1.shape[1], g=sv.g, ysel=sv.ysel, g_mean=cg.mean, g_rstd=cg.rstd,
                     g_gamma=P["bn_global.weight"], g_scene_sum=cg.scene_sum, dW_s1_global=bw.G("seg_conv1.weight"),
                     csum=csum, alpha=ag, beta_c=bg, gamma_c=gg, dgamma=bw.G("bn_global.weight"),
                     dbeta=bw.G("bn_global.bias"), dbias=bw.G("global_feat.bias"), sp=sp)
        L.call("pcs_pool_bwd", pa, s)
        bw.keep.append(csum)
        return sp

    def _bwd_seg1_local(self, P, sv, bw):
        """seg_conv1's local half: dW[:, :64], and its contribution dA2 to a2's gradient (raw; conv3's input gradient
        adds it), which it returns."""
        B, N, M, dev, s = self._dims(sv)
        a1, b1, g1 = bw.coefs["bn_seg1"]
        dz_s1, ys, Ws1 = bw.bufA, sv.ys, P["seg_conv1.weight"]
        dA2 = torch.empty(M, 64, dtype=self.tdt, device=dev)
        if not sv.paths.wide_fast:
            self._gemm(sv, 512, 64, L.PRO_BWD, L.EPI_RAW, dz_s1, sv.wc["seg_conv1"][1], dA2,
                       A2=ys["seg_conv1"], pa=a1, pb=b1, pc=g1, tag="dgrad:seg_conv1")
            self._wgrad_bn(sv, bw, "seg_conv1", dz_s1, "conv2", cin=64, ldw=Ws1.shape[1])
            return dA2
        # folded form, one pass over dz_s1 and y2 (csrc/fused_bwd.hip): with dy = a1 dz +
        # b1 + g1 Y' and Y' = a2 W_l^T + sbias[b] (the stored pre-BN output),
        #   dA2 = dz (diag(a1) W_l) + a2 H + cvec[b],  H = W_l^T diag(g1) W_l,
        #   dW_l = diag(a1) dz^T a2 + b1 (x) S + diag(g1) (W_l G2 + sum_b sbias[b] (x) S_b)
        # (G2 = a2^T a2, S_b = per-scene column sums of a2), so bn_seg1's Y' is not read
        p2 = sv.bn["bn2"]
        Ws1_r = self._rounded(Ws1)     # the W_l the forward GEMM used
        WaT, Hs1 = self._empty(64, 512, device=dev), self._empty(64, 64, device=dev)
        # no cvec output: the folded kernel forms its per-scene cvec_b itself (folded_cvec_kernel)
        L.call("pcs_bn_fold", Ws1_r, 512, 64, Ws1.shape[1], a1, b1, g1, self.dt, WaT, None, Hs1, s)
        fa = self._wgrad_args(sv, 512, 64, L.PRO_RAW, L.PRO_BNRELU, bw.G("seg_conv1.weight"), ldw=Ws1.shape[1],
                              dZ=dz_s1, alpha=a1, beta=b1, gamma=g1, X=ys["conv2"], s=p2.scale, t=p2.shift)
        nbytes = L.workspace("pcs_dgrad_wgrad_folded_workspace", fa)
        ws1 = _f32(dev, nbytes // 4)
        fa.partial = ws1.data_ptr()
        self._launch("dgrad+wgrad:seg_conv1", "pcs_dgrad_wgrad_folded", fa, WaT, Hs1, Ws1_r, sv.sbias_s1, dA2, s)
        bw.keep.append((ws1, Ws1_r, WaT, Hs1))
        return dA2

    def _bwd_global_dgrad(self, P, sv, bw, sp):
        """global_feat's input gradient in folded form (P:113 at P:254): with dy_g = beta_g +
        gamma_g * y_g + (max-pool rows) and y_g = a5 Wg^T,
          dA5 = a5 H + 1 c^T + sum_b sp[b, c] Wg[c, :] at the row am[b, c],
        H = Wg^T diag(gamma_g) Wg, c = Wg^T beta_g (pcs_bn_fold); the epilogue masks with
        a5 > 0 (bn5's ReLU) and sums S1 = sum dz5; S2 comes from R = dz5^T a4 (_bwd_conv5).
        Leaves dz5 in bufB; returns (the W the forward GEMM used, S1 partials, chunks per scene)."""
        B, N, M, dev, s = self._dims(sv)
        pt, a5, dz5 = sv.paths, sv.ys["a5"], bw.bufB
        bg, gg = bw.coefs["bn_global"][1:]
        # the W the forward GEMM used (see pcs_round_weight; fp8: the dequantized e4m3 rows)
        Wg_r = sv.wg_eff if sv.gram5 is not None else \
            sv.wc["global_feat_fp8"][2] if pt.fp8 else self._rounded(P["global_feat.weight"])
        cvec = _f32(dev, 1024)
        # fp8: H in fp32, then e4m3 rows with one scale each (H is symmetric: row n = column n)
        Hg = _f32(dev, 1024, 1024) if pt.fp8 else self._empty(1024, 1024, device=dev)
        L.call("pcs_bn_fold", Wg_r, 1024, 1024, Wg_r.shape[1], None, bg, gg, L.F32 if pt.fp8 else self.dt, None, cvec, Hg,
               s)
        pool_rows = dict(pool_idx=sv.am, pool_coef=sp, pool_w=Wg_r, pool_ldw=Wg_r.shape[1], pool_c=1024)
        if pt.fp8:
            Hq, hsc, _ = self._quant_fp8(Hg)   # (the dequantized copy lives until `_` is next assigned)
            Hg = (Hg, Hq, hsc)
            W, kw = Hq, dict(w_scale=hsc, extra_flags=L.FLAG_AW_FP8)
        else:
            # glds: the LDS-DMA kernel without the max-pool rows (no ordinary global loads in its
            # epilogue); otherwise the rows in the epilogue, with the W the forward GEMM used
            W, kw = Hg, ({} if pt.glds else pool_rows)
        cps5, _ = self.geometry(B, N, 1024, 1024, L.PRO_RAW, L.EPI_DGRAD, flags=pt.flags)
        st5 = _f32(dev, B * cps5, 1024, 2)
        self._gemm(sv, 1024, 1024, L.PRO_RAW, L.EPI_DGRAD, a5, W, dz5, bias=cvec, Yp=a5, stats=st5,
                   tag="dgrad:global_feat", **kw)
        if pt.fp8 or pt.glds:
            # the max-pool rows' sparse term, with the W the forward GEMM used; S1 in both
            L.call("pcs_pool_rows_add", dz5, self.dt, a5, self.a5_dt, B, N, 1024, sv.am, sp, Wg_r, Wg_r.shape[1], 1024,
                   st5, cps5, s)
        if self.perturb is not None and "dz5" in self.perturb:   # test hooks
            c0, c1, scale = self.perturb["dz5"]
            dz5.view(M, 1024)[:, c0:c1].mul_(scale)
        if self.capture is not None:
            self.capture.update(dz5=dz5.view(M, 1024).clone(), a5=a5, H=Hg, cvec=cvec, am=sv.am.clone(),
                                sp=sp.clone(), Wg_r=Wg_r)
        bw.keep.append((Hg, cvec))
        return Wg_r, st5, cps5

    def _bwd_global_wgrad(self, P, sv, bw, sp, Wg_r):
        """global_feat's weight gradient from the Gram of a5: the symmetric a5^T a5 (upper tiles) + an O(C^3) assemble
        instead of the M x 1024 x 1024 GEMM."""
        B, N, _, dev, s = self._dims(sv)
        a5 = sv.ys["a5"]
        _, bg, gg = bw.coefs["bn_global"]
        ones = torch.ones(1024, dtype=torch.float32, device=dev)
        zeros = torch.zeros(1024, dtype=torch.float32, device=dev)
        raw = sv.paths.wide_fast and sv.a5_colsum is not None
        # (with the forward's Gram this buffer is released unused: part of the pinned pattern)
        gram = _f32(dev, 1024, 1024) if sv.gram5 is not None or raw else None
        if sv.gram5 is not None:
            # computed in the forward (bn_global's statistics); S = sum of the per-scene sums
            gram, Sb, ws = sv.gram5
            colsum = _f32(dev, 1024)
            L.call("pcs_reduce_partials", Sb, B, 1024, 1.0, colsum, 1024, 1024, s)
        elif raw:
            # a5 is the activation itself: LDS-DMA Gram; S from conv5's per-chunk column sums
            ws = self._gram_raw(a5, gram)
            cs2 = _f32(dev, 1024, 2)
            L.call("pcs_reduce_partials", sv.a5_colsum, sv.a5_colsum.shape[0], 2048, 1.0, cs2, 2048, 2048, s)
            colsum = cs2[:, 0].contiguous()
            bw.keep.append(cs2)
        else:
            gram, colsum, ws = self._gram(a5, ones, zeros, B, N, 1024, tag="wgrad:global_feat")
        self._launch("wgrad_asm:global_feat", "pcs_gram_wgrad", gram, colsum, Wg_r, P["global_feat.weight"].shape[1],
                     bg, gg, sp, sv.am, a5, ones, zeros, B, 1024, 1024, self.a5_dt, None, None,
                     bw.G("global_feat.weight"), 1024, s)
        bw.keep.append((ones, zeros, gram, colsum, ws, Wg_r))

    def _bwd_conv5(self, P, sv, bw, st5, cps5):
        """conv5 (128 -> 1024): R = dz5^T a4 gives bn5's S2 (y5 = a4 W5^T is not stored) and
        the alpha-term of dW5; then the folded input gradient and the Gram-form dW5:
          dA4 = dz5 (diag(alpha5) W5) + a4 (W5^T diag(gamma5) W5) + W5^T beta5
          dW5 = diag(alpha5) R + beta5 (x) colsum(a4) + diag(gamma5) W5 (a4^T a4)
        Leaves dz4 in bufA."""
        B, N, M, dev, s = self._dims(sv)
        dz5, y4, cap = bw.bufB, sv.ys["conv4"], self.capture
        pc4, pc5 = sv.bn["bn4"], sv.bn["bn5"]
        r5 = _f32(dev, 1024, 128)
        bw.keep.append(self._wgrad(sv, 1024, 128, L.PRO_RAW, L.PRO_BNRELU, r5, tag="wgrad:conv5",
                                   dZ=dz5, X=y4, s=pc4.scale, t=pc4.shift))
        if cap is not None:
            cap.update(r5=r5.clone(), y4=y4, s4=pc4.scale, t4=pc4.shift)
        L.call("pcs_bn_s2_from_r", st5, B * cps5, 1024, r5, sv.wc["conv5"][0], self.dt, 128, 128, pc5.mean, pc5.rstd, s)
        self._bn_bwd(P, sv, bw, "bn5", "conv5", st5, cps5)
        al5, be5, ga5 = bw.coefs["bn5"]
        W5_r = self._rounded(P["conv5.weight"])
        ws_t, c5, h4 = self._empty(128, 1024, device=dev), _f32(dev, 128), self._empty(128, 128, device=dev)
        L.call("pcs_bn_fold", W5_r, 1024, 128, 128, al5, be5, ga5, self.dt, ws_t, c5, h4, s)
        # one pass: [dz5 | a4] [Ws ; H4] + c5 (PCS_PRO_CAT), then bn4's ReLU mask and S1 / S2
        cps4, _ = self.geometry(B, N, 1024 + 128, 128, L.PRO_CAT, L.EPI_DGRAD, flags=sv.paths.flags)
        bw.st = _f32(dev, B * cps4, 128, 2)
        self._gemm(sv, 1024 + 128, 128, L.PRO_CAT, L.EPI_DGRAD, dz5, ws_t, bw.bufA, K1=1024, A2=y4,
                   W2=h4, pa=pc4.scale, pb=pc4.shift, bias=c5, Yp=y4, es=pc4.scale, et=pc4.shift,
                   emean=pc4.mean, erstd=pc4.rstd, stats=bw.st, tag="dgrad:conv5")
        if cap is not None:
            cap.update(dz4=bw.bufA[:M * 128].view(M, 128).clone(), ws_t=ws_t, h4=h4, c5=c5)
        g4, s4, ws4 = sv.gram4 if sv.gram4 is not None else \
            self._gram(y4, pc4.scale, pc4.shift, B, N, 128, tag="gram:conv4")
        self._launch("wgrad_asm:conv5", "pcs_gram_wgrad", g4, s4, W5_r, 128, be5, ga5, None, None, None, None, None, B,
                     1024, 128, self.dt, r5, al5, bw.G("conv5.weight"), 128, s)
        bw.keep.append((ws_t, c5, h4, r5, g4, s4, ws4, W5_r))
        self._bn_bwd(P, sv, bw, "bn4", "conv4", bw.st, cps4)

    def _bwd_trunk(self, P, sv, bw, dA2):
        """conv4..conv1: the dZ buffers ping-pong; conv3's input gradient adds seg_conv1's dA2."""
        self._bwd_layer(P, sv, bw, "conv4", bw.bufA, "conv3", bw.bufB)
        self._bwd_layer(P, sv, bw, "conv3", bw.bufB, "conv2", bw.bufA, addend=dA2)
        self._bwd_layer(P, sv, bw, "conv2", bw.bufA, "conv1", bw.bufB)
        al, be, ga = bw.coefs["bn1"]
        bw.keep.append(self._wgrad(sv, 64, self.input_dim, L.PRO_BWD, L.PRO_RAW, bw.G("conv1.weight"),
                                   ldw=self.input_dim, conv1=True, tag="wgrad:conv1", dZ=bw.bufB, Y=sv.ys["conv1"],
                                   alpha=al, beta=be, gamma=ga, X=sv.x))
