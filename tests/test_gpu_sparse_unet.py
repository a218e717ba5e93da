"""The occupied-voxel U-Net (pcs_amd.sparse_unet: SparsePyramid, SparseUNet,
SparseUNetSegmentation) on MI355X, on grid 16, 2 scenes, occupancy 0.3, widths (64, 128, 128).  The
architecture is pinned without a new tolerance: the model's logits and every parameter gradient are
torch.equal to a composition written out here from the model's own submodules, with each merge
replaced by torch.cat + submanifold_conv3d on merge.weight (every layer underneath has its own fp64
test).  Then training, the state dict and a ragged batch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pcs_amd.sparse_unet import SparsePyramid, SparseUNet, SparseUNetSegmentation, sparse_pyramid

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
GRID, WIDTHS = 16, (64, 128, 128)

_BN = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
_RES = ["conv1.weight"] + [f"bn1.{k}" for k in _BN] + ["conv2.weight"] + [f"bn2.{k}" for k in _BN]
KEYS = ([f"unet.enc.{l}.{k}" for l in (0, 1) for k in _RES]
        + ["unet.down.0.weight", "unet.down.1.weight"] + [f"unet.down_bn.{l}.{k}" for l in (0, 1) for k in _BN]
        + [f"unet.bottom.{k}" for k in _RES]
        + ["unet.up.0.weight", "unet.up.1.weight"] + [f"unet.up_bn.{l}.{k}" for l in (0, 1) for k in _BN]
        + ["unet.merge.0.weight", "unet.merge.1.weight"] + [f"unet.merge_bn.{l}.{k}" for l in (0, 1) for k in _BN]
        + [f"unet.dec.{l}.{k}" for l in (0, 1) for k in _RES]
        + ["lift.weight", "lift.bias", "head.weight", "head.bias"])


def _batch(seed=21, grid=GRID, scenes=2):
    from pcs_amd.data import jittered_clouds, ragged_collate
    clouds = jittered_clouds(seed, scenes, grid=grid, occupancy=0.3, per_voxel=3)
    return ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])


def _level(rb, grid):
    from pcs_amd.sparse import sparse_voxels
    from pcs_amd.voxel import voxelize
    return sparse_voxels(rb, voxelize(rb, grid, LO, HI), LO, HI)


def _model(seed=0):
    torch.manual_seed(seed)
    return SparseUNetSegmentation(4, 2, WIDTHS, GRID, LO, HI).to(DEV)


def test_pyramid():
    rb = _batch()
    pyr = sparse_pyramid(_level(rb, GRID), 2)
    assert isinstance(pyr, SparsePyramid) and pyr.depth == 2
    assert [sv.grid for sv in pyr.levels] == [16, 8, 4] and len(pyr.links) == 2
    for l, link in enumerate(pyr.links):
        assert link.fine == pyr.levels[l].num_voxels and link.coarse == pyr.levels[l + 1].num_voxels
        assert pyr.levels[l + 1].num_voxels <= pyr.levels[l].num_voxels
    assert sparse_pyramid(pyr.levels[0], 0).links == []
    with pytest.raises(ValueError, match="12"):
        sparse_pyramid(_level(_batch(grid=12), 12), 3)
    with pytest.raises(ValueError):
        SparseUNet(WIDTHS).to(DEV)(torch.zeros(pyr.levels[0].num_voxels, 64, dtype=torch.bfloat16, device=DEV),
                                   sparse_pyramid(pyr.levels[0], 1))     # 3 widths need depth 2


def _hand_forward(model, rb):
    """SparseUNetSegmentation.forward written out layer by layer from the model's submodules; each
    merge is the concatenated layer: torch.cat([up, skip], 1) + submanifold_conv3d."""
    from pcs_amd.pointvoxel import devoxelize, point_voxel_map, voxel_mean
    from pcs_amd.sparse import coarsen, submanifold_conv3d
    u_ = model.unet
    sv0 = _level(rb, GRID)
    sv1, link0 = coarsen(sv0)
    sv2, link1 = coarsen(sv1)
    pvm = point_voxel_map(rb, sv0, LO, HI)
    x0 = voxel_mean(torch.relu(model.lift(rb.points.to(DEV).float())), pvm)
    e0 = u_.enc[0](x0, sv0)
    x1 = u_.down_bn[0](u_.down[0](e0, link0))
    e1 = u_.enc[1](x1, sv1)
    x2 = u_.down_bn[1](u_.down[1](e1, link1))
    c = u_.bottom(x2, sv2)
    up1 = u_.up_bn[1](u_.up[1](c, link1))
    m1 = u_.merge_bn[1](submanifold_conv3d(torch.cat([up1, e1], 1), u_.merge[1].weight, sv1))
    d1 = u_.dec[1](m1, sv1)
    up0 = u_.up_bn[0](u_.up[0](d1, link0))
    m0 = u_.merge_bn[0](submanifold_conv3d(torch.cat([up0, e0], 1), u_.merge[0].weight, sv0))
    d0 = u_.dec[0](m0, sv0)
    return model.head(devoxelize(d0, pvm))


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_model_equals_the_hand_composition(mode):
    rb = _batch()
    model = _model()
    model.train(mode == "train")
    labels = rb.labels.to(DEV)
    weight = torch.tensor([1.0, 2.0], device=DEV)
    out = {}
    for name, fwd in (("model", lambda: model(rb)), ("hand", lambda: _hand_forward(model, rb))):
        model.zero_grad(set_to_none=True)
        logits = fwd()
        F.cross_entropy(logits, labels, weight=weight, ignore_index=-1).backward()
        out[name] = (logits.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()})
    (la, ga), (lb, gb) = out["model"], out["hand"]
    assert la.dtype == torch.float32 and la.shape == (rb.points.shape[0], 2) and torch.isfinite(la).all()
    assert torch.equal(la, lb)
    assert set(ga) == {k for k in KEYS if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    for k in ga:
        assert torch.isfinite(ga[k]).all() and ga[k].abs().max() > 0, k
        assert torch.equal(ga[k], gb[k]), (k, float((ga[k] - gb[k]).abs().max()))


def test_trains_with_fused_adam():
    from pcs_amd.optim import FusedAdam
    from pcs_amd.sparse_norm import SparseBatchNorm
    rb = _batch()
    model = _model()
    opt = FusedAdam(model, lr=3e-3)
    labels = rb.labels.to(DEV)
    assert (labels == -1).any() and (labels >= 0).any()
    weight = torch.tensor([1.0, 2.0], device=DEV)
    bns = [m for m in model.modules() if isinstance(m, SparseBatchNorm)]
    assert len(bns) == 2 * 5 + 3 * 2                          # 5 residual blocks, down / up / merge per level
    losses = []
    for _ in range(8):
        loss = F.cross_entropy(model(rb), labels, weight=weight, ignore_index=-1)
        opt.zero_grad()
        loss.backward()
        for k, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), k
        for l, w in enumerate(WIDTHS[:-1]):
            g = model.unet.merge[l].weight.grad
            assert g[:, :w].abs().max() > 0 and g[:, w:].abs().max() > 0, l   # neither the up nor the skip branch is dead
        opt.step()
        losses.append(loss.item())
    print("losses", [round(v, 4) for v in losses])
    assert losses[-1] < losses[0]
    for m in bns:
        assert int(m.num_batches_tracked) == 8
        assert m.running_mean.abs().max() > 0 and (m.running_var - 1).abs().max() > 0
        assert torch.isfinite(m.running_mean).all() and torch.isfinite(m.running_var).all()


def test_state_dict():
    rb = _batch()
    model = _model()
    assert list(model.state_dict()) == KEYS
    model.train()
    with torch.no_grad():
        model(rb)                                             # move the running statistics off their init
    model.eval()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        a, b = model(rb), model(rb)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    fresh = _model(seed=1).eval()
    with torch.no_grad():
        assert not torch.equal(fresh(rb), a)
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh(rb), a)


def test_ragged_batch_and_ignored_labels():
    rb = _batch(seed=5)
    counts = (rb.offsets[1:] - rb.offsets[:-1]).tolist()
    assert counts[0] != counts[1]
    T = rb.points.shape[0]
    model = _model().eval()
    with torch.no_grad():
        logits = model(rb)
    assert logits.shape == (T, 2) and logits.dtype == torch.float32
    # point order: a point of the batch gets the same logits when the scenes are swapped (eval mode;
    # the voxel rows move, the per-point rows follow the batch)
    from pcs_amd.data import RaggedBatch
    n0 = counts[0]
    swapped = RaggedBatch(torch.cat([rb.points[n0:], rb.points[:n0]]), torch.cat([rb.labels[n0:], rb.labels[:n0]]),
                          torch.tensor([0, T - n0, T], dtype=torch.int64))
    with torch.no_grad():
        ls = model(swapped)
    err = float((torch.cat([ls[T - n0:], ls[:T - n0]]) - logits).abs().max())
    print("scene swap: max logit difference", err)
    assert err < 1e-2 * float(logits.abs().max())             # bf16 activations, a different summation order
    # rows with label -1 contribute no loss: no gradient reaches their logits, and changing which
    # rows are ignored changes the loss
    labels = rb.labels.to(DEV)
    keep = labels >= 0
    assert (~keep).any()
    lg = logits.detach().clone().requires_grad_()
    loss = F.cross_entropy(lg, labels, ignore_index=-1)
    loss.backward()
    assert not lg.grad[~keep].any() and lg.grad[keep].abs().max() > 0
    assert torch.allclose(loss, F.cross_entropy(lg[keep], labels[keep]))
    assert np.isfinite(loss.item())
