"""SparseUNetSegmentation(lift="max") on MI355X: the default path (voxel_max of relu(Linear)) against
the fused one (pcs_amd.segmax.point_lift_max), the loss step, and that lift="mean" is the model as it
was.  tests/test_gpu_sparse_unet.py's shape: grid 16, 2 scenes, occupancy 0.3, widths (64, 128, 128)."""
import pytest
import torch

from pcs_amd.sparse_unet import SparseUNetSegmentation

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
GRID, WIDTHS = 16, (64, 128, 128)
REL = 1e-2      # tests/test_gpu_point_head_model.py's bound of the fused against the default logits


def _batch(seed=21):
    from pcs_amd.data import jittered_clouds, ragged_collate
    clouds = jittered_clouds(seed, 2, grid=GRID, occupancy=0.3, per_voxel=3)
    return ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])


def _model(seed=0, **kw):
    torch.manual_seed(seed)
    return SparseUNetSegmentation(4, 2, WIDTHS, GRID, LO, HI, **kw).to(DEV)


def test_max_lift_fused_matches_the_default_in_eval_mode():
    rb = _batch()
    model = _model(lift="max")
    with torch.no_grad():
        for _ in range(3):                                       # move the running statistics
            model(rb)
    model.eval()
    with torch.no_grad():
        a, f, f2 = model(rb), model(rb, fused=True), model(rb, fused=True)
        mean = _model().eval()
        mean.load_state_dict(model.state_dict())
        other = mean(rb)
    assert f.dtype == torch.float32 and f.shape == a.shape and torch.isfinite(f).all()
    assert torch.equal(f, f2)
    err, top = float((a - f).abs().max()), float(a.abs().max())
    print(f"lift='max': fused against default logits: max difference {err:.3e}, max |logit| {top:.3e}; "
          f"against lift='mean' on the same parameters {float((a - other).abs().max()):.3e}")
    assert err < REL * top
    assert not torch.equal(a, other)                             # it is another function


def test_max_lift_loss_backward_reaches_every_parameter():
    rb = _batch()
    model = _model(lift="max").train()
    loss = model.loss(rb, torch.tensor([1.0, 2.0], device=DEV))
    loss.backward()
    assert torch.isfinite(loss)
    params = dict(model.named_parameters())
    assert {"lift.weight", "lift.bias", "head.weight", "head.bias"} <= set(params)
    for k, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k


def test_mean_lift_is_the_model_as_it_was():
    rb = _batch()
    a, b = _model().eval(), _model(lift="mean").eval()
    assert a.lift_mode == b.lift_mode == "mean"
    with torch.no_grad():
        assert torch.equal(a(rb), b(rb)) and torch.equal(a(rb, fused=True), b(rb, fused=True))


def test_state_dict_and_argument():
    assert list(_model(lift="max").state_dict()) == list(_model().state_dict())
    with pytest.raises(ValueError, match="median"):
        SparseUNetSegmentation(4, 2, WIDTHS, GRID, LO, HI, lift="median")
