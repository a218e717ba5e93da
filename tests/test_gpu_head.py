"""pcs_head (seg_conv4 + weighted CE + head backward) on its own through the C ABI, every kernel
it dispatches to, against the fp64 head_ref of tests/small_refs.py (proved against torch autograd
in tests/test_small_refs.py):

  stream  head_stream_kernel<C>          bf16, CE, C <= 4, no logits buffer
  small   head_small_kernel<T, C, MODE>  C <= 4 otherwise
  mid16   head_kernel<T, MODE, 16>       5 <= C <= 16
  mid64   head_kernel<T, MODE, 64>       17 <= C <= 64
  wide    head_wide_kernel<T, MODE>      65 <= C <= 256

in fp32 and bf16 storage and the three modes, at both sides of every dispatch edge and of the wide
head's 8- and 16-class ownership groups, on ragged scenes and chunks.

Inputs: |s| in [0.5, 1.5] with a quarter of the channels negative, t ~ 0.5 N(0,1),
Y ~ 1.5 N(0,1) + 0.2 in the storage dtype; wherever |Y*s + t| < 1e-3 in fp64, Y is replaced by
the stored value of (+-0.05 - t)/s, and the builder asserts min |Y*s + t| >= 1e-3, so that no fp32
rounding can flip a ReLU against the reference.  No element is left out of any comparison.

Bounds (small_refs.head_bounds; none tuned on GPU output) come from the reference's absolute
sums: one rounding for a, a 129-term chain for a logit, exp / log at 2 ulp each propagated
through the softmax, a C-term chain for dl W (plus 2^-8 |ref| for a bf16 dZ), and
rows-per-chunk-term sums for S1 / S2 / dW / db / loss.  stats, wpartial and loss_partial are
summed over the chunks in fp64 first (the kernels chunk the rows differently).  Every output is
prefilled with NaN and followed by a guard region that must stay untouched; dZ must be exactly 0
where the reference's a is 0.  The worst err / bound ratio per kernel class, dtype and output is
printed when the module finishes (pytest -s); a bf16 dZ comes close to 1 by construction (the
unit roundoff of bf16 is 2^-8, so its term of the bound is exactly one rounding)."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

import small_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32 = np.float32
CIN = 128
GUARD = 512                 # elements after every output
SENTINEL = 1234.0           # the guard is compared in its own dtype (bf16 stores 1232)
CLASSES = [1, 2, 4, 5, 16, 17, 33, 64, 65, 100, 255, 256]
ONE_PER_KERNEL = [2, 16, 64, 256]            # with bf16 + CE + logits NULL / given: all five kernels
DTYPES = ["f32", "bf16"]
RATIOS = {}


def kernel_class(C, dtype, mode, logits_given):
    if C <= 4:
        return "stream" if (dtype == "bf16" and mode == R.HEAD_CE and not logits_given) else "small"
    return "mid16" if C <= 16 else "mid64" if C <= 64 else "wide"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst err / bound per kernel class, storage dtype and output:")
    for (k, dtype, name), v in sorted(RATIOS.items()):
        print(f"  {k:7s} {dtype:5s} {name:9s} {v:.3f}")


def stored(a, dtype):
    """a in the storage dtype, as a torch tensor (host)."""
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(torch.bfloat16 if dtype == "bf16" else torch.float32)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


class Out:
    """n elements of NaN and a guard region of GUARD sentinels after them."""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        self.t = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=DEV)
        self.t[n:] = SENTINEL
        self.guard = self.t[n:].clone()

    def ptr(self):
        return self.t.data_ptr()

    def get(self, *shape):
        return self.t[:self.n].double().cpu().numpy().reshape(shape)

    def intact(self):
        return bool(torch.equal(self.t[self.n:], self.guard))


@functools.lru_cache(maxsize=16)
def inputs(B, N, C, dtype, logit_peak=None):
    """The synthetic operands of one (shape, class count, dtype), as the fp32 / bf16 values the
    kernel reads.  With logit_peak, W is scaled so that the largest fp64 |logit| is about it."""
    r = np.random.default_rng([B, N, C, dtype == "bf16"])
    M = B * N
    s = (r.uniform(0.5, 1.5, CIN) * np.where(r.random(CIN) < 0.25, -1.0, 1.0)).astype(F32)
    t = (0.5 * r.standard_normal(CIN)).astype(F32)
    mean = (0.3 * r.standard_normal(CIN)).astype(F32)
    rstd = np.abs(1.0 + 0.1 * r.standard_normal(CIN)).astype(F32)
    s64, t64 = s.astype(np.float64), t.astype(np.float64)
    Y = stored(1.5 * r.standard_normal((M, CIN)) + 0.2, dtype)
    z = Y.double().numpy() * s64 + t64
    near = np.abs(z) < 1e-3
    moved = stored((np.where(z >= 0, 0.05, -0.05) - t64) / s64 * np.ones_like(z), dtype)
    Y = torch.where(torch.from_numpy(near), moved, Y)
    z = Y.double().numpy() * s64 + t64
    assert np.abs(z).min() >= 1e-3, np.abs(z).min()      # a condition on the inputs, not a tolerance
    W = (0.1 * r.standard_normal((C, CIN))).astype(F32)
    bias = (0.2 * r.standard_normal(C)).astype(F32)
    if logit_peak:
        peak = np.abs(np.maximum(z, 0.0) @ W.astype(np.float64).T).max()
        W = (W * (logit_peak / peak)).astype(F32)
        lg = np.maximum(z, 0.0) @ W.astype(np.float64).T + bias
        assert 80.0 <= np.abs(lg).max() <= 100.0, np.abs(lg).max()
    labels = r.integers(0, C, M)
    labels[r.random(M) < 0.25] = -1
    cw = r.uniform(0.5, 1.5, C).astype(F32)
    if C >= 2:
        cw[C // 2] = 0.0                                   # a class of weight exactly 0
    dlog = (0.1 * r.standard_normal((M, C))).astype(F32)
    host = dict(Y=Y.double().numpy(), s=s, t=t, mean=mean, rstd=rstd, W=W, bias=bias, cw=cw,
                labels=labels, dlog=dlog, near=int(near.sum()), open=float((z > 0).mean()))
    device = dict(Y=Y.to(DEV), s=dev(s), t=dev(t), mean=dev(mean), rstd=dev(rstd), W=dev(W), bias=dev(bias),
                  cw=dev(cw))
    return host, device


def weight_sum(cw, labels, C):
    ok = (labels >= 0) & (labels < C)
    return F32(cw.astype(np.float64)[labels[ok]].sum()) if ok.any() else F32(1.0)


@functools.lru_cache(maxsize=16)
def reference(B, N, C, dtype, mode, logit_peak=None):
    """head_ref on the module's default labels / dlogits of these inputs (computed once, shared)."""
    h, _ = inputs(B, N, C, dtype, logit_peak)
    return ref_of(h, mode, h["labels"], weight_sum(h["cw"], h["labels"], C), h["dlog"])


def ref_of(h, mode, labels=None, wsum=None, dlog=None):
    return R.head_ref(h["Y"], h["s"], h["t"], h["mean"], h["rstd"], h["W"], h["bias"], mode, labels=labels,
                      class_weight=h["cw"], wsum=wsum, dlogits=dlog)


def run(B, N, C, dtype, mode, d, cps=0, logits_given=True, labels=None, wsum=None, dlogits=None, strides=None):
    """One pcs_head call into NaN-filled, guarded outputs sized from pcs_head_geometry.  dlogits:
    a device tensor with element strides (row, col).  Returns what the mode writes (fp64, host),
    rows per chunk and chunks per scene."""
    import pcs_amd._lib as L
    M = B * N
    a = L.HeadArgs(num_scenes=B, scene_rows=N, Cin=CIN, num_classes=C, dtype=L.BF16 if dtype == "bf16" else L.F32,
                   mode=mode, chunks_per_scene=cps, Y=d["Y"].data_ptr(), s=d["s"].data_ptr(), t=d["t"].data_ptr(),
                   W=d["W"].data_ptr(), bias=d["bias"].data_ptr())
    bufs = {}
    if logits_given:
        bufs["logits"] = Out(M * C)
        a.logits = bufs["logits"].ptr()
    keep = []
    if mode == R.HEAD_CE:
        lab = dev(labels, torch.int64)
        keep.append(lab)
        a.labels, a.class_weight = lab.data_ptr(), d["cw"].data_ptr()
        if wsum is not None:
            ws = dev(np.array([wsum], F32))
            keep.append(ws)
            a.wsum = ws.data_ptr()
    if mode == R.HEAD_BWD:
        a.dlogits, (a.dl_stride_row, a.dl_stride_col) = dlogits.data_ptr(), strides
    rpc = L.load().pcs_head_geometry(ct.byref(a))     # fills chunks_per_scene for this kernel
    cps = a.chunks_per_scene
    assert rpc > 0 and cps >= 1 and rpc * cps >= N and rpc * (cps - 1) < N, (rpc, cps, N)   # no empty chunk
    nch = B * cps
    if mode != R.HEAD_FWD:
        bufs["dZ"] = Out(M * CIN, torch.bfloat16 if dtype == "bf16" else torch.float32)
        bufs["stats"] = Out(nch * CIN * 2)
        bufs["wpartial"] = Out(nch * C * (CIN + 1))
        a.dZ, a.stats, a.wpartial = bufs["dZ"].ptr(), bufs["stats"].ptr(), bufs["wpartial"].ptr()
        a.mean, a.rstd = d["mean"].data_ptr(), d["rstd"].data_ptr()
    if mode == R.HEAD_CE:
        bufs["loss_partial"] = Out(nch)
        a.loss_partial = bufs["loss_partial"].ptr()
    L.call("pcs_head", ct.byref(a), L.stream_ptr())
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert b.intact(), f"guard region after {name} overwritten"
    out = dict(rpc=int(rpc), cps=int(cps), nch=nch)
    if logits_given:
        out["logits"] = bufs["logits"].get(M, C)
    if mode != R.HEAD_FWD:
        out["dZ"] = bufs["dZ"].get(M, CIN)
        out["stats"] = bufs["stats"].get(nch, CIN, 2)
        out["wpartial"] = bufs["wpartial"].get(nch, C * (CIN + 1))
    if mode == R.HEAD_CE:
        out["loss_partial"] = bufs["loss_partial"].get(nch)
    return out


def check(out, ref, h, C, dtype, mode, logits_given, tag):
    """Every output the mode writes against the reference, each element within its bound (a NaN
    left from the prefill fails)."""
    k = kernel_class(C, dtype, mode, logits_given)
    key = ("bounds", out["rpc"])                        # shared with the reference they belong to
    if key not in ref:
        ref[key] = R.head_bounds(ref, h["W"], mode, out["rpc"], bf16_dz=dtype == "bf16")
    bnd = ref[key]
    got = {}
    if logits_given:
        got["logits"] = out["logits"]
    if mode != R.HEAD_FWD:
        got["dz"] = out["dZ"]
        st = out["stats"].sum(0)
        got["S1"], got["S2"] = st[:, 0], st[:, 1]
        wp = out["wpartial"].sum(0)
        got["dW"], got["db"] = wp[:C * CIN].reshape(C, CIN), wp[C * CIN:]
        assert np.isfinite(out["stats"]).all() and np.isfinite(out["wpartial"]).all(), f"{tag}: a partial is not finite"
        assert (out["dZ"][ref["a"] == 0] == 0).all(), f"{tag}: dZ not 0 behind a closed ReLU"
    if mode == R.HEAD_CE:
        assert np.isfinite(out["loss_partial"]).all(), f"{tag}: a loss partial is not finite"
        got["loss_sum"] = out["loss_partial"].sum()
    for name, g in got.items():
        ratio = R.assert_within(g, ref[name], bnd[name], f"{tag} [{k}] {name}")
        RATIOS[(k, dtype, name)] = max(RATIOS.get((k, dtype, name), 0.0), ratio)


def run_check(B, N, C, dtype, mode, cps=0, logits_given=True, logit_peak=None, labels=None, use_wsum=True):
    """The call on the default labels / contiguous dlogits of these inputs (or the given labels),
    checked against the (shared) reference."""
    h, d = inputs(B, N, C, dtype, logit_peak)
    kw = {}
    if mode == R.HEAD_CE:
        lab = h["labels"] if labels is None else labels
        kw = dict(labels=lab, wsum=weight_sum(h["cw"], lab, C) if use_wsum else None)
        ref = reference(B, N, C, dtype, mode, logit_peak) if labels is None and use_wsum else \
            ref_of(h, mode, lab, kw["wsum"])
    else:
        if mode == R.HEAD_BWD:
            kw = dict(dlogits=dev(h["dlog"]), strides=(C, 1))
        ref = reference(B, N, C, dtype, mode, logit_peak)
    out = run(B, N, C, dtype, mode, d, cps=cps, logits_given=logits_given, **kw)
    check(out, ref, h, C, dtype, mode, logits_given,
          f"B={B} N={N} C={C} {dtype} mode={mode} cps={out['cps']} logits={'given' if logits_given else 'NULL'}")
    return out, ref


# ---------------------------------------------------------------------------------------
# the grid: every class count, dtype and mode
# ---------------------------------------------------------------------------------------
# (B, N, chunks_per_scene asked for): ragged for the 16- and 64-row tiles; exactly one 64-row tile;
# shorter than any tile; several tiles per chunk with a ragged last one (auto, 1 and 2 chunks)
GRID = [(2, 333, 0), (3, 64, 0), (1, 15, 0), (2, 1001, 0), (2, 1001, 1), (2, 1001, 2)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,N,cps", GRID)
@pytest.mark.parametrize("C", CLASSES)
def test_head_matches_fp64(C, B, N, cps, dtype):
    """FWD, CE without and with a logits buffer (for bf16 and C <= 4: the stream and the register
    kernel) and BWD, each against the reference.  A quarter of the labels are -1, one class has
    weight 0, wsum is a device scalar."""
    h, _ = inputs(B, N, C, dtype)
    assert 0.3 < h["open"] < 0.7                                  # about half the ReLUs open
    run_check(B, N, C, dtype, R.HEAD_FWD, cps)
    run_check(B, N, C, dtype, R.HEAD_CE, cps, logits_given=False)
    out, _ = run_check(B, N, C, dtype, R.HEAD_CE, cps, logits_given=True)
    run_check(B, N, C, dtype, R.HEAD_BWD, cps, logits_given=False)
    if cps:
        assert out["cps"] == cps


# ---------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("logits_given", [False, True])
@pytest.mark.parametrize("C", [1, 4, 5, 17, 65, 256])
def test_ce_without_wsum(C, dtype, logits_given):
    """wsum == NULL: the gradient is not divided."""
    _, ref = run_check(2, 333, C, dtype, R.HEAD_CE, logits_given=logits_given, use_wsum=False)
    assert ref["gscale"] == 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("logits_given", [False, True])
@pytest.mark.parametrize("C", ONE_PER_KERNEL)
def test_ce_one_chunk_all_ignored(C, dtype, logits_given):
    """Every label of one whole chunk is -1: that chunk's partials are exactly 0 and its dZ rows
    are written (0); the rest is unchanged."""
    B, N, rpc = 2, 1001, 512                                         # 16 tiles of 64 rows in 2 chunks
    h, _ = inputs(B, N, C, dtype)
    lab = h["labels"].copy()
    lab[N + rpc:2 * N] = -1                                         # the second chunk of the second scene
    out, ref = run_check(B, N, C, dtype, R.HEAD_CE, cps=2, logits_given=logits_given, labels=lab)
    assert out["cps"] == 2 and out["rpc"] == rpc
    assert (out["loss_partial"][3] == 0).all() and (out["wpartial"][3] == 0).all() and (out["stats"][3] == 0).all()
    assert (out["dZ"][N + rpc:] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("logits_given", [False, True])
@pytest.mark.parametrize("C", ONE_PER_KERNEL)
def test_ce_all_ignored(C, dtype, logits_given):
    """Every label -1: the loss and all gradients are exactly 0 (the bounds are 0), dZ is written."""
    B, N = 2, 333
    lab = np.full(B * N, -1, np.int64)
    out, ref = run_check(B, N, C, dtype, R.HEAD_CE, logits_given=logits_given, labels=lab)
    assert ref["loss_sum"] == 0 and not ref["dl"].any()
    for name in ("dZ", "stats", "wpartial", "loss_partial"):
        assert (out[name] == 0).all(), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("logits_given", [False, True])
@pytest.mark.parametrize("C", ONE_PER_KERNEL)
def test_ce_out_of_range_labels_are_ignored(C, dtype, logits_given):
    """Labels < -1 or >= C count as ignored in all five kernels, whatever their low 32 bits."""
    B, N = 2, 333
    h, _ = inputs(B, N, C, dtype)
    lab = h["labels"].copy()
    odd = np.array([-2, -100, C, C + 7, 1 << 32, (1 << 32) + C - 1, -(1 << 32), (1 << 31) + 1, -(1 << 31),
                    np.iinfo(np.int64).max, np.iinfo(np.int64).min], np.int64)
    rows = np.random.default_rng(C).permutation(B * N)[:4 * len(odd)]
    lab[rows] = np.tile(odd, 4)
    out, ref = run_check(B, N, C, dtype, R.HEAD_CE, logits_given=logits_given, labels=lab)
    assert not ref["valid"][rows].any() and not ref["dl"][rows].any()
    assert (out["dZ"][rows] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("logits_given", [False, True])
@pytest.mark.parametrize("C", ONE_PER_KERNEL)
def test_ce_large_logits(C, dtype, logits_given):
    """W scaled so that the fp64 logits reach |z| of 80 to 100: a softmax without the max
    subtracted would overflow; loss and dl (through dZ, dW, db) stay within their bounds."""
    out, ref = run_check(2, 333, C, dtype, R.HEAD_CE, logits_given=logits_given, logit_peak=90.0)
    assert 80.0 <= np.abs(ref["logits"]).max() <= 100.0


LAYOUTS = ["contiguous", "transposed", "padded"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("B,N", [(2, 333), (1, 15)])
@pytest.mark.parametrize("C", [1, 3, 4, 5, 16, 17, 64, 65, 255])
def test_bwd_dlogits_layouts(C, B, N, layout, dtype):
    """dlogits as [M, C], as a [C, M] buffer viewed transposed and as a row-padded view, with a
    logits buffer.  The backing buffer holds independent random values and is long enough for
    either order of the two strides, so a kernel that swapped them would read other values."""
    M = B * N
    h, d = inputs(B, N, C, dtype)
    sr, sc = {"contiguous": (C, 1), "transposed": (1, M), "padded": (C + 3, 1)}[layout]
    big = max(sr, sc)
    back = (0.1 * np.random.default_rng([M, C, sr]).standard_normal((M - 1 + C - 1) * big + 1)).astype(F32)
    dl = back[np.arange(M)[:, None] * sr + np.arange(C)[None, :] * sc]
    if C > 1:
        assert not np.array_equal(dl, back[np.arange(M)[:, None] * sc + np.arange(C)[None, :] * sr])
    ref = ref_of(h, R.HEAD_BWD, dlog=dl)
    out = run(B, N, C, dtype, R.HEAD_BWD, d, logits_given=True, dlogits=dev(back), strides=(sr, sc))
    check(out, ref, h, C, dtype, R.HEAD_BWD, True, f"{layout} B={B} N={N} C={C} {dtype}")
