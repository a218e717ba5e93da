"""predict() of the two voxel U-Nets on MI355X (SparseUNetSegmentation, VoxelUNetSegmentation; the
inference path of pcs_amd.fold: every convolution -> BatchNorm (+ residual) + ReLU as one kernel on the
running statistics).  Build-defined, not reference parity.

The structure is pinned without a tolerance: predict's logits are torch.equal to a composition written
out here from fold.conv_bn calls on the model's own submodules (each layer has its bit-identity and fp64
test in tests/test_gpu_fold_layers.py).  Then the whole model against the fp64 restatement of
tests/voxel_unet_refs.py at full occupancy, measured beside the existing eval forward; the labels; side
effects and determinism; and a swapped ragged batch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_unet_refs as vr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
SPARSE = dict(grid=16, widths=(64, 128, 128))
DENSE = dict(grid=8, widths=(32, 64, 64))


def _collate(clouds):
    from pcs_amd.data import ragged_collate
    return ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])


def _batch(grid, seed=21):
    """2 ragged scenes, occupancy 0.3."""
    from pcs_amd.data import jittered_clouds
    return _collate(jittered_clouds(seed, 2, grid=grid, occupancy=0.3, per_voxel=3))


def _randomise_bn(model, seed=9):
    """gamma with both signs, running_mean ~ N(0, 0.5), running_var ~ U(0.5, 2): nothing is at its init."""
    from pcs_amd.sparse_norm import SparseBatchNorm
    g = torch.Generator().manual_seed(seed)
    bns = [m for m in model.modules() if isinstance(m, SparseBatchNorm)]
    assert len(bns) == 16
    with torch.no_grad():
        for bn in bns:
            c = bn.num_features
            bn.weight.copy_((0.5 + torch.rand(c, generator=g)) * (torch.randint(0, 2, (c,), generator=g) * 2 - 1))
            bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
            bn.running_mean.copy_(torch.randn(c, generator=g) * 0.5)
            bn.running_var.copy_(0.5 + 1.5 * torch.rand(c, generator=g))
    return model


def _model(kind, lift="mean", seed=0, grid=None, widths=None):
    from pcs_amd.sparse_unet import SparseUNetSegmentation
    from pcs_amd.voxel_unet import VoxelUNetSegmentation
    cls, cfg = (SparseUNetSegmentation, SPARSE) if kind == "sparse" else (VoxelUNetSegmentation, DENSE)
    torch.manual_seed(seed)
    return _randomise_bn(cls(4, 2, widths or cfg["widths"], grid or cfg["grid"], LO, HI, lift=lift).to(DEV))


def _res(block, x, *tail):
    from pcs_amd.fold import conv_bn
    h = conv_bn(block.conv1, block.bn1, x, *tail)
    return conv_bn(block.conv2, block.bn2, h, *tail, residual=x)


def _hand_predict(model, rb, kind):
    """predict's logits written out layer by layer: conv_bn on the model's submodules, for any depth."""
    from pcs_amd.fold import conv_bn
    from pcs_amd.pointhead import point_head, point_lift_mean
    from pcs_amd.segmax import point_lift_max
    u_, pts = model.unet, rb.points.to(DEV).float()
    lift = point_lift_max if model.lift_mode == "max" else point_lift_mean
    with torch.no_grad():
        if kind == "sparse":
            from pcs_amd.pointvoxel import point_voxel_map
            from pcs_amd.sparse import coarsen, sparse_voxels
            from pcs_amd.voxel import voxelize
            levels, links = [sparse_voxels(rb, voxelize(rb, model.grid, LO, HI), LO, HI)], []
            for _ in range(u_.depth):
                svc, link = coarsen(levels[-1])
                levels.append(svc)
                links.append(link)
            pvm = point_voxel_map(rb, levels[0], LO, HI)
            x = lift(pts, model.lift.weight, model.lift.bias, pvm)
            lv = lambda l: (levels[l],)   # noqa: E731
            lk = lambda l: (links[l],)    # noqa: E731
        else:
            from pcs_amd.voxel_unet import dense_point_map
            G, B = model.grid, rb.offsets.numel() - 1
            pvm = dense_point_map(rb, G, LO, HI)
            x = lift(pts, model.lift.weight, model.lift.bias, pvm).view(B, G, G, G, -1)
            lv = lk = lambda l: ()        # noqa: E731
        skips = []
        for l in range(u_.depth):
            skips.append(_res(u_.enc[l], x, *lv(l)))
            x = conv_bn(u_.down[l], u_.down_bn[l], skips[l], *lk(l))
        x = _res(u_.bottom, x, *lv(u_.depth))
        for l in reversed(range(u_.depth)):
            up = conv_bn(u_.up[l], u_.up_bn[l], x, *lk(l))
            m = conv_bn(u_.merge[l], u_.merge_bn[l], up, skips[l], *lv(l))
            x = _res(u_.dec[l], m, *lv(l))
        return point_head(x.reshape(-1, x.shape[-1]), pvm, model.head.weight, model.head.bias)


@pytest.mark.parametrize("lift", ["mean", "max"])
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_predict_equals_the_hand_composition_and_labels_are_its_argmax(kind, lift):
    model = _model(kind, lift)
    rb = _batch(model.grid)
    labels, logits = model.predict(rb, return_logits=True)
    T = rb.points.shape[0]
    assert logits.dtype == torch.float32 and logits.shape == (T, 2) and torch.isfinite(logits).all()
    assert not logits.requires_grad
    assert torch.equal(logits, _hand_predict(model, rb, kind))
    assert labels.dtype == torch.int64 and labels.shape == (T,)
    assert torch.equal(labels, torch.argmax(logits, 1))
    assert torch.equal(model.predict(rb), labels)


# ---- full occupancy: against fp64, beside the existing eval forward
def _full_batch(grid=8, seed=5, extra=2):
    """tests/test_gpu_voxel_unet.py's batch: every cell of the 8^3 grid of both scenes holds its centre
    point plus a few random ones."""
    rng = np.random.default_rng(seed)
    h = 2.0 / grid
    ax = (-1.0 + (np.arange(grid) + 0.5) * h).astype(np.float32)
    centres = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    clouds = []
    for s in range(2):
        m = extra * grid ** 3 + 31 * s
        p = np.zeros((len(centres) + m, 4), np.float32)
        p[:len(centres), :3] = centres
        p[len(centres):, :3] = rng.uniform(-1, 1, (m, 3)).astype(np.float32)
        p[:, 3] = rng.exponential(size=len(p)).astype(np.float32)
        clouds.append((p, rng.integers(-1, 2, len(p)).astype(np.int64)))
    return clouds


_FP64 = {}


def _fp64_logits(lift):
    """The eval-mode fp64 logits of the (seed 3) state dict, once per lift: the reference of both models."""
    if lift not in _FP64:
        clouds = _full_batch()
        rb = _collate(clouds)
        dense = _model("dense", lift, seed=3, grid=8, widths=(32, 64, 128))
        sd = vr.params64(dense.state_dict())
        with torch.no_grad():
            ref = vr.model_logits(sd, np.concatenate([p for p, _ in clouds]), rb.offsets.numpy(), 8, LO, HI,
                                  training=False, lift=lift)
        _FP64[lift] = (rb, dense.state_dict(), ref)
    return _FP64[lift]


@pytest.mark.parametrize("lift", ["mean", "max"])
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_full_occupancy_against_fp64(kind, lift):
    """tests/test_gpu_voxel_unet.py's full-occupancy batch and widths (32, 64, 128) on grid 8, where both
    models are the fp64 function of tests/voxel_unet_refs.model_logits(training=False).  e_fold and e_eval
    are max|logits - fp64| / max|fp64| of predict and of the existing eval forward (model.eval();
    model(rb, fused=True)); the condition is e_fold <= 1.5 * e_eval.  The folded path drops one bf16
    rounding per layer, so it should be no worse; 1.5 covers one draw's rounding.  A wrong channel, a
    missing residual or a wrong activation moves the logits by order 1.

    Measured on MI355X, e_fold / e_eval (largest fp64 logit 0.464 with lift "mean", 0.496 with "max"), the
    same for the sparse and the dense model:
      lift "mean"   5.9316e-03 / 6.0471e-03
      lift "max"    5.6459e-03 / 7.0996e-03"""
    rb, state, ref = _fp64_logits(lift)
    model = _model(kind, lift, seed=4, grid=8, widths=(32, 64, 128))
    model.load_state_dict(state)
    model.train()
    _, logits = model.predict(rb, return_logits=True)
    model.eval()
    with torch.no_grad():
        ev = model(rb, fused=True)
    scale = float(ref.abs().max())
    e_fold = float((logits.double().cpu() - ref).abs().max()) / scale
    e_eval = float((ev.double().cpu() - ref).abs().max()) / scale
    print(f"full occupancy {kind} lift={lift}: e_fold {e_fold:.4e}  e_eval {e_eval:.4e}  (fp64 max abs {scale:.4e})")
    assert e_eval > 0 and np.isfinite(e_fold)
    assert e_fold <= 1.5 * e_eval, (e_fold, e_eval)


@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_side_effects_and_determinism(kind):
    model = _model(kind).train()
    rb = _batch(model.grid)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert any(k.endswith("num_batches_tracked") for k in before)
    la, a = model.predict(rb, return_logits=True)
    assert model.training and all(m.training for m in model.modules())
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not a.requires_grad and a.grad_fn is None and not la.requires_grad
    lb, b = model.predict(rb, return_logits=True)
    assert torch.equal(a, b) and torch.equal(la, lb)
    model.eval()
    lc, c = model.predict(rb, return_logits=True)
    assert not model.training and torch.equal(a, c) and torch.equal(la, lc)
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    assert all(p.grad is None for p in model.parameters())


@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_scene_swap(kind):
    """tests/test_gpu_sparse_unet.py::test_ragged_batch_and_ignored_labels's property and bound for predict:
    a point of the batch gets the same logits when the two scenes are swapped (the voxel rows move, the
    per-point rows follow the batch)."""
    from pcs_amd.data import RaggedBatch
    model = _model(kind)
    rb = _batch(model.grid, seed=5)
    counts = (rb.offsets[1:] - rb.offsets[:-1]).tolist()
    assert counts[0] != counts[1]
    T, n0 = rb.points.shape[0], counts[0]
    _, logits = model.predict(rb, return_logits=True)
    swapped = RaggedBatch(torch.cat([rb.points[n0:], rb.points[:n0]]), torch.cat([rb.labels[n0:], rb.labels[:n0]]),
                          torch.tensor([0, T - n0, T], dtype=torch.int64))
    _, ls = model.predict(swapped, return_logits=True)
    err = float((torch.cat([ls[T - n0:], ls[:T - n0]]) - logits).abs().max())
    print(f"scene swap ({kind}): max logit difference {err:.3e} at max |logit| {float(logits.abs().max()):.3e}")
    assert err < 1e-2 * float(logits.abs().max())
