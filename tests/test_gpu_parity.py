"""Parity of the HIP path (through the C ABI) against the numpy oracle and the reference's
golden vectors.

fp32 path: logits within 1e-4 max-norm-relative (BASELINE north star); argmax bit-exact
outside a 1e-4 tie margin; gradients within 2e-3 L2-norm-relative per tensor.  The
gradient bound is looser than the logits bound because fp32 forward rounding (~4e-6
relative at seg_conv2/3, the same order as the reference's own fp32 error vs the fp64
oracle) can flip a ReLU whose fp64 pre-activation is within ~1e-6 of 0; one flipped
(point, channel) changes a BN-bias gradient by that point's dz (measured 2e-4..3e-3 of
the tensor's max entry on train_c2, where the oracle has |z| = 3.1e-6 at seg_conv3).  An
implementation error shows up as O(1e-1..1) instead.  Per-kernel exactness of the unfused
backward GEMMs (pcs_wgrad, pcs_gemm with PCS_PRO_BWD) is asserted in test_gpu_bwd_unfused.py,
so the 2e-3 bound here is about ReLU flips only.
bf16 path: bounded by bf16 storage itself (a numpy bf16-rounding emulation of the forward
gives 6.6e-2 logits error on train_c2): logits < 1e-1, argmax agreement > 95 %, gradient
cosine similarity > 0.85 per tensor (measured 0.90..0.9996 on train_c2; BN in train
mode amplifies bf16 rounding, early layers lowest)."""
import numpy as np
import pytest
import torch

import pointnet_oracle as orc
from golden_util import CASES, inputs, load, rel_err

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def _model(sd, C, dtype="fp32", train=True):
    from pcs_amd.model import PointNetSegmentation
    m = PointNetSegmentation(C, compute_dtype=dtype).to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    m.train(train)
    return m


def _bits(masks):
    return tuple(torch.from_numpy(np.packbits(m, axis=1, bitorder="little")).to(DEV) for m in masks)


def _grad_errs(model, grads, cosine=False):
    """L2-norm-relative error per tensor (or 1 - cosine similarity); the conv biases that
    BN cancels (analytic gradient 0, both sides fp noise) are measured against the
    largest gradient norm instead of their own."""
    gmax = max(np.linalg.norm(v) for v in grads.values())
    errs = {}
    for n, p in model.named_parameters():
        gv = p.grad.detach().cpu().numpy().reshape(-1).astype(np.float64)
        rv = grads[n].reshape(-1)
        noisy = n.endswith(".bias") and not n.startswith(("bn", "seg_conv4"))
        if cosine:
            if noisy or np.linalg.norm(rv) < 1e-9 * gmax:   # analytically ~0 gradients
                continue
            errs[n] = float(1 - gv @ rv / (np.linalg.norm(gv) * np.linalg.norm(rv) + 1e-30))
        else:
            scale = 1e-3 * gmax if noisy else max(np.linalg.norm(rv), 1e-3 * gmax)
            errs[n] = float(np.linalg.norm(gv - rv) / scale)
    return errs


@pytest.mark.parametrize("name", CASES)
def test_logits_fp32_match_oracle_and_golden(name):
    g = load(name)
    sd, pts, lab, msk, masks = inputs(g)
    train = bool(g["train"])
    m = _model(sd, int(g["C"]), train=train)
    if train:
        m.set_dropout_masks(*_bits(masks))
    with torch.no_grad():
        out = m(torch.from_numpy(pts).to(DEV)).cpu().numpy()
    ref, _ = orc.forward(sd, pts, train=train, masks=masks)
    assert rel_err(out, ref) < 1e-4
    assert rel_err(out, g["logits"]) < 1e-4
    # labels: bit-exact argmax outside the tie margin
    top2 = np.sort(ref, axis=-1)[..., -2:]
    margin = (top2[..., 1] - top2[..., 0]) > 1e-4 * np.abs(ref).max()
    assert (out.argmax(-1) == ref.argmax(-1))[margin].all()


@pytest.mark.parametrize("name", [c for c in CASES if not c.startswith("eval")])
def test_autograd_backward_fp32_matches_oracle(name):
    g = load(name)
    sd, pts, lab, msk, masks = inputs(g)
    C = int(g["C"])
    m = _model(sd, C)
    m.set_dropout_masks(*_bits(masks))
    out = m(torch.from_numpy(pts).to(DEV))
    crit = torch.nn.CrossEntropyLoss(ignore_index=-1, weight=torch.tensor(g["weight"], device=DEV))
    loss = crit(out.contiguous().view(-1, C), torch.from_numpy(lab).to(DEV).view(-1))
    loss.backward()
    rloss, _, grads, cache = orc.train_step(sd, pts, lab, g["weight"], masks=masks)
    assert abs(loss.item() - rloss) < 1e-5 * max(1.0, abs(rloss))
    errs = _grad_errs(m, grads)
    bad = {k: v for k, v in errs.items() if v > 2e-3}
    assert not bad, bad
    # BN running statistics after the train forward (momentum 0.1, unbiased var)
    sd2 = orc.update_running_stats(sd, cache)
    for k, v in m.state_dict().items():
        if "running" in k:
            np.testing.assert_allclose(v.cpu().numpy(), sd2[k], rtol=2e-5, atol=1e-6, err_msg=k)
        if "num_batches_tracked" in k:
            assert int(v) == 1


@pytest.mark.parametrize("name", ["train_c2", "train_c3_ragged_bnrand"])
def test_fused_train_step_fp32(name):
    """Fused CE + backward + Adam (one kernel stream) == reference step (P:241-255)."""
    from pcs_amd.optim import FusedAdam, flat_buffers
    from pcs_amd.train import FusedTrainStep
    g = load(name)
    sd, pts, lab, msk, masks = inputs(g)
    C = int(g["C"])
    m = _model(sd, C)
    opt = FusedAdam(m, lr=1e-3, weight_decay=1e-4)
    step = FusedTrainStep(m, opt, class_weight=g["weight"])
    loss = step(torch.from_numpy(pts).to(DEV), torch.from_numpy(lab).to(DEV), masks=_bits(masks))
    torch.cuda.synchronize()
    rloss, _, grads, _ = orc.train_step(sd, pts, lab, g["weight"], masks=masks)
    assert abs(loss.item() - rloss) < 1e-5 * max(1.0, abs(rloss))
    errs = _grad_errs(m, grads)
    bad = {k: v for k, v in errs.items() if v > 2e-3}
    assert not bad, bad
    # the parameters after the fused Adam step == Adam applied to the kernel's gradients
    names = [n for n, _ in m.named_parameters()]
    ours = {n: p.grad.detach().cpu().numpy().astype(np.float64) for n, p in m.named_parameters()}
    new = orc.adam_step({n: sd[n].astype(np.float64) for n in names}, ours, {})
    for n, p in m.named_parameters():
        np.testing.assert_allclose(p.detach().cpu().numpy(), new[n], rtol=0, atol=2e-6, err_msg=n)
    # against the reference's own Adam-updated samples.  A first Adam step moves each entry
    # by ~lr*sign(g): an entry lands within 2*lr of the reference wherever its gradient is
    # smaller than the fp32 perturbation of one ReLU-boundary flip (see module docstring;
    # 4 % of the sampled entries on train_c2), so the bound is 2.1e-3 everywhere and 1e-5
    # for >= 95 % of the samples.
    close = total = 0
    for n, p in m.named_parameters():
        idx = g[f"gidx/{n}"]
        d = np.abs(p.detach().cpu().numpy().reshape(-1)[idx] - g[f"pval/{n}"])
        assert d.max() <= 2.1e-3, n
        close += int((d <= 1e-5).sum())
        total += d.size
    assert close >= 0.95 * total, (close, total)
    pflat, gflat = flat_buffers(m)
    assert pflat.numel() == sum(p.numel() for p in m.parameters())


def test_cfg1_size_fp32_parity():
    """BASELINE configs[0] shape: B=4 x 4096-point clouds on a 32^3 lattice, C=2."""
    from pcs_amd.data import synthetic_batch
    sd = orc.init_params(2, 99, bn_affine_random=True)
    pts, lab, _ = synthetic_batch(1234, [4096, 3000, 4096, 2500], 2, grid=32)
    masks = orc.dropout_masks(5, pts.shape[0] * pts.shape[1])
    w = np.array([0.6, 1.4], np.float32)
    m = _model(sd, 2)
    m.set_dropout_masks(*_bits(masks))
    out = m(torch.from_numpy(pts).to(DEV))
    crit = torch.nn.CrossEntropyLoss(ignore_index=-1, weight=torch.tensor(w, device=DEV))
    loss = crit(out.contiguous().view(-1, 2), torch.from_numpy(lab).to(DEV).view(-1))
    loss.backward()
    rloss, rlogits, grads, _ = orc.train_step(sd, pts, lab, w, masks=masks)
    assert rel_err(out.detach().cpu().numpy(), rlogits) < 1e-4
    errs = _grad_errs(m, grads)
    bad = {k: v for k, v in errs.items() if v > 2e-3}
    assert not bad, bad


def test_bf16_path_tracks_oracle():
    """bf16 storage / MFMA with fp32 accumulation (bounds: module docstring)."""
    g = load("train_c2")
    sd, pts, lab, msk, masks = inputs(g)
    m = _model(sd, 2, dtype="bf16")
    m.set_dropout_masks(*_bits(masks))
    out = m(torch.from_numpy(pts).to(DEV))
    crit = torch.nn.CrossEntropyLoss(ignore_index=-1, weight=torch.tensor(g["weight"], device=DEV))
    loss = crit(out.contiguous().view(-1, 2), torch.from_numpy(lab).to(DEV).view(-1))
    loss.backward()
    rloss, rlogits, grads, _ = orc.train_step(sd, pts, lab, g["weight"], masks=masks)
    o = out.detach().cpu().numpy()
    print("bf16 logits rel err", rel_err(o, rlogits))
    assert rel_err(o, rlogits) < 1e-1
    assert (o.argmax(-1) == rlogits.argmax(-1)).mean() > 0.95
    assert abs(loss.item() - rloss) < 1e-2
    errs = _grad_errs(m, grads, cosine=True)
    print("bf16 1-cos", errs)
    bad = {k: v for k, v in errs.items() if v > 0.15}
    assert not bad, bad


def test_dropout_bits_statistics_and_determinism():
    import pcs_amd._lib as L
    M, C = 65536, 512
    a = torch.empty(M, C // 8, dtype=torch.uint8, device=DEV)
    b = torch.empty_like(a)
    c = torch.empty_like(a)
    L.call("pcs_dropout_bits", 123, 0, M, C, 0.3, L.ptr(a), L.stream_ptr())
    L.call("pcs_dropout_bits", 123, 0, M, C, 0.3, L.ptr(b), L.stream_ptr())
    L.call("pcs_dropout_bits", 123, 1, M, C, 0.3, L.ptr(c), L.stream_ptr())
    bits = np.unpackbits(a.cpu().numpy(), axis=1, bitorder="little")
    assert abs(bits.mean() - 0.7) < 2e-3
    assert torch.equal(a, b) and not torch.equal(a, c)
    # channels are independent: per-channel keep rates all near 0.7
    assert np.abs(bits.mean(0) - 0.7).max() < 0.02
    # elements 2k and 2k+1 share one byte pair of their 16-bit uniforms (the high byte of one is
    # the low byte of the other, csrc/small.hip dropout_bits_kernel): their joint keep rate is
    # the exact enumeration over the two bytes, ~0.49 = 0.7^2
    thr = int(0.3 * 65536.0 + 0.5)
    r = np.arange(256)
    u_a = (r[:, None] << 8) | r[None, :]
    u_b = (r[None, :] << 8) | r[:, None]
    joint = float(((u_a >= thr) & (u_b >= thr)).mean())
    both = float((bits[:, 0::2] & bits[:, 1::2]).mean())
    assert abs(joint - 0.49) < 5e-3 and abs(both - joint) < 3e-3, (joint, both)
    # elements of different pairs are independent
    cross = float((bits[:, 0::4] & bits[:, 2::4]).mean())
    assert abs(cross - 0.49) < 3e-3, cross
    # a bounded grid (words strided over few workgroups) draws the same bits, ragged tail included
    for wg in (1, 7, 512):
        d = torch.zeros(M - 3, C // 8, dtype=torch.uint8, device=DEV)
        L.call("pcs_dropout_bits_bounded", 123, 0, M - 3, C, 0.3, L.ptr(d), wg, L.stream_ptr())
        assert torch.equal(d, a[:M - 3])
    # the ends of p: 0 keeps everything; within 2^-17 of 1 (threshold 65536) keeps nothing
    e = torch.zeros(257, C // 8, dtype=torch.uint8, device=DEV)
    L.call("pcs_dropout_bits", 123, 0, 257, C, 0.0, L.ptr(e), L.stream_ptr())
    assert bool((e == 255).all())
    L.call("pcs_dropout_bits", 123, 0, 257, C, 1.0 - 2.0 ** -20, L.ptr(e), L.stream_ptr())
    assert bool((e == 0).all())


def test_dropout_bits_independent_draw():
    """pcs_dropout_bits_independent (opt-in, PointNetSegmentation(dropout_draw="independent")):
    i.i.d. keep bits as nn.Dropout (P:96): marginal 0.7, adjacent elements' joint keep 0.49
    (the paired default gives 0.490463), deterministic per (seed, offset); the model's
    training forward draws exactly these bits."""
    import pcs_amd._lib as L
    from pcs_amd.model import PointNetSegmentation
    M, C = 65536, 512
    a, b, c, pr = (torch.empty(M, C // 8, dtype=torch.uint8, device=DEV) for _ in range(4))
    s = L.stream_ptr()
    L.call("pcs_dropout_bits_independent", 123, 0, M, C, 0.3, L.ptr(a), s)
    L.call("pcs_dropout_bits_independent", 123, 0, M, C, 0.3, L.ptr(b), s)
    L.call("pcs_dropout_bits_independent", 123, 1, M, C, 0.3, L.ptr(c), s)
    L.call("pcs_dropout_bits", 123, 0, M, C, 0.3, L.ptr(pr), s)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, pr)
    bits = np.unpackbits(a.cpu().numpy(), axis=1, bitorder="little")
    keep = 1.0 - int(0.3 * 65536.0 + 0.5) / 65536.0
    assert abs(bits.mean() - keep) < 2e-3
    assert np.abs(bits.mean(0) - keep).max() < 0.02
    for lag in (1, 2, 8, 16):   # adjacent, same Philox word, same call, next call
        both = float((bits[:, :-lag] & bits[:, lag:]).mean())
        assert abs(both - keep * keep) < 2e-3, (lag, both)
    e = torch.zeros(257, C // 8, dtype=torch.uint8, device=DEV)
    L.call("pcs_dropout_bits_independent", 123, 0, 257, C, 0.0, L.ptr(e), s)
    assert bool((e == 255).all())
    # the model option routes the training forward's draw here (both dropouts, offsets 0 / 1)
    m = PointNetSegmentation(2, compute_dtype="bf16", dropout_draw="independent").to(DEV).train()
    B, N = 2, 1000
    x = torch.randn(B, N, 4, device=DEV)
    eng = m._engine()
    sv = eng.forward(m._param_dict(), m._buffer_dict(), x, train=True, seed=77)
    torch.cuda.synchronize()
    for off, (K, got) in enumerate(((512, sv.masks[0]), (256, sv.masks[1]))):
        ref = torch.empty(B * N, K // 8, dtype=torch.uint8, device=DEV)
        L.call("pcs_dropout_bits_independent", 77, off, B * N, K, 0.3, L.ptr(ref), s)
        torch.cuda.synchronize()
        assert torch.equal(got, ref)
    with pytest.raises(ValueError):
        PointNetSegmentation(2, dropout_draw="iid")


def test_train_mode_random_dropout_runs_and_differs():
    sd = orc.init_params(2, 5)
    pts, _, _ = __import__("pcs_amd.data", fromlist=["x"]).synthetic_batch(3, [256, 256], 2)
    m = _model(sd, 2)
    x = torch.from_numpy(pts).to(DEV)
    with torch.no_grad():
        a = m(x)
        b = m(x)
    assert not torch.equal(a, b)           # fresh Philox draws each forward
    m.eval()
    with torch.no_grad():
        e1 = m(x)
        e2 = m(x)
    assert torch.equal(e1, e2)             # eval: deterministic, dropout off


def test_cpu_input_raises():
    sd = orc.init_params(2, 5)
    m = _model(sd, 2)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 16, 4))


def test_bf16_big_kernel_matches_generic_kernel():
    """The 256x256 wide-layer kernels (LDS-DMA and register-staged) and the generic 128-row
    kernel compute the same bf16 step.

    * Two launches of the default (LDS-DMA) path on identical inputs are bitwise identical.
    * register-staged 256x256 (FLAG_NO_GLDS) vs generic: both take global_feat's BN
      statistics and max-pool candidates from the bf16-rounded tile, so they differ only by
      fp32 summation order (measured r02: logits 2.8e-3, seg_conv <= 8.3e-4 norm-rel, cosine
      >= 0.99995): logits < 1e-2, seg_conv outputs < 1e-2 norm-relative, gradient cosine
      > 0.999 (tighter than the pre-LDS-DMA 2e-2 / 0.99).
    * LDS-DMA vs generic: the LDS-DMA kernel takes them from its fp32 accumulators, so the
      pooled g (and seg_conv1's per-scene bias W_g g) differ by up to one bf16 ulp per
      channel, which train-mode BN over these two small scenes amplifies through seg_conv1-3
      (measured r02: logits 2.49e-2, seg_conv 1.2-2.3e-2 norm-rel, cosine >= 0.934); bounds
      are the measured values plus a stated margin: logits < 4e-2, seg_conv < 4e-2,
      cosine > 0.92."""
    import pcs_amd._lib as L
    from pcs_amd.data import synthetic_batch
    sd = orc.init_params(3, 17, bn_affine_random=True)
    pts, lab, _ = synthetic_batch(77, [3000, 2100], 3, grid=32)
    masks = orc.dropout_masks(9, pts.shape[0] * pts.shape[1])
    bits = _bits(masks)
    x = torch.from_numpy(pts).to(DEV)
    outs = []
    for flags in (0, 0, L.FLAG_NO_GLDS, L.FLAG_GENERIC):
        m = _model(sd, 3, dtype="bf16")
        eng = m._engine()
        eng.flags = flags
        m.set_dropout_masks(*bits)
        out = m(x)
        crit = torch.nn.CrossEntropyLoss(ignore_index=-1)
        crit(out.contiguous().view(-1, 3), torch.from_numpy(lab).to(DEV).view(-1)).backward()
        sv = eng.forward(m._param_dict(), {}, x, train=True, masks=bits)
        outs.append((out.detach().float().cpu().numpy(),
                     {k: v.float().cpu().numpy() for k, v in sv.ys.items()},
                     {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()}))
    (o1, y1, g1), (o1b, y1b, g1b), (o3, y3, g3), (o2, y2, g2) = outs
    # two launches of the wide-layer path on identical inputs are bitwise identical (no
    # atomics on float data; a pipeline race would show up here first)
    assert np.array_equal(o1, o1b)
    for k in y1:
        assert np.array_equal(y1[k], y1b[k]), k
    for n in g1:
        assert np.array_equal(g1[n], g1b[n]), n

    def compare(tag, oa, ya, ga, ob, yb, gb, seg_tol, logit_tol, cos_min):
        for k in ya:
            d = np.abs(ya[k] - yb[k])
            if k.startswith("seg_conv"):
                nrm = float(np.linalg.norm(ya[k] - yb[k]) / np.linalg.norm(yb[k]))
                print(tag, k, "norm-rel", nrm)
                assert nrm < seg_tol, (tag, k, nrm)
            else:   # before the pool: a few bf16 ulps
                assert d.max() <= 4e-2 * np.abs(yb[k]).max() and d.mean() <= 2e-3 * np.abs(yb[k]).mean() + 1e-6, \
                    (tag, k, float(d.max()), float(d.mean()), float(np.abs(yb[k]).mean()))
        print(tag, "logits", rel_err(oa, ob))
        assert rel_err(oa, ob) < logit_tol, tag
        for n in ga:
            # BN-cancelled conv biases are noise; bn_global.bias is nonzero only through pooled
            # features whose relu sits at ~0 (a one-ulp bf16 difference decides which), so it
            # is not comparable between two accumulation orders.
            if (n.endswith(".bias") and not n.startswith(("bn", "seg_conv4"))) or n == "bn_global.bias":
                continue
            cs = (ga[n].ravel() @ gb[n].ravel()) / (np.linalg.norm(ga[n]) * np.linalg.norm(gb[n]) + 1e-30)
            print(tag, n, "cos", cs)
            assert cs > cos_min or np.linalg.norm(gb[n]) < 1e-9, (tag, n, cs)

    compare("noglds-vs-generic", o3, y3, g3, o2, y2, g2, 1e-2, 1e-2, 0.999)
    compare("glds-vs-generic", o1, y1, g1, o2, y2, g2, 4e-2, 4e-2, 0.92)
