"""Device side of SURVEY §8 f1/f3: pcs_confusion (vs numpy), predict() (vs the oracle's eval
forward on the reference golden case) and a save -> load -> predict round trip."""
import numpy as np
import pytest
import torch

import pointnet_oracle as orc
from golden_util import inputs, load

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("C", [2, 3, 13])
def test_confusion_matches_numpy(C):
    from pcs_amd.metrics import ConfusionMeter
    g = torch.Generator().manual_seed(C)
    meter = ConfusionMeter(C, DEV)
    ref = np.zeros((C, C), np.int64)
    for _ in range(2):
        z = torch.randn(3, 1001, C, generator=g)
        y = torch.randint(-1, C, (3, 1001), generator=g)
        meter.update(z.to(DEV), y.to(DEV))
        v = y.reshape(-1).numpy() >= 0
        np.add.at(ref, (y.reshape(-1).numpy()[v], z.reshape(-1, C).argmax(1).numpy()[v]), 1)
    assert np.array_equal(meter.cm.cpu().numpy(), ref)
    assert meter.compute()["points"] == int(ref.sum())


def test_predict_and_checkpoint_roundtrip(tmp_path):
    from pcs_amd.checkpoint import load_checkpoint, predict, save_checkpoint
    from pcs_amd.model import PointNetSegmentation
    g = load("eval_c2_bnrand")
    sd, pts, lab, msk, masks = inputs(g)
    m = PointNetSegmentation(int(g["C"])).to(DEV)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    x = torch.from_numpy(pts).to(DEV)
    pred = predict(m, x).cpu().numpy()
    logits, _ = orc.forward(sd, pts, train=False)
    top2 = np.sort(logits, axis=-1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 1e-4 * np.abs(logits).max()
    assert np.array_equal(pred[clear], logits.argmax(-1)[clear])
    path = tmp_path / "best_model.pth"
    save_checkpoint(path, m, epoch=1, data_parallel=True)
    m2, _ = load_checkpoint(path, device=DEV)
    assert torch.equal(predict(m2, x).cpu(), torch.from_numpy(pred))


def _special_logits(C, rows=600, seed=0):
    """Random logits whose first rows carry the cases torch.argmax settles by rule: a NaN
    counts as the maximum and the first one wins (also over +inf); otherwise the first
    maximum."""
    nan, inf = float("nan"), float("inf")
    z = torch.randn(rows, C, generator=torch.Generator().manual_seed(seed + C))
    mid, last = C // 2, C - 1
    z[0, 0] = nan                                  # NaN first
    z[1, mid] = nan                                # NaN in the middle
    z[2, last] = nan                               # NaN last
    z[3, mid], z[3, last] = nan, nan               # several NaNs
    z[4, max(last - 1, 0)], z[4, last] = inf, nan  # inf before a NaN
    z[5, 0], z[5, last] = nan, inf                 # NaN before an inf
    z[6, :] = -inf                                 # all -inf
    z[7, :] = 1.0                                  # every class ties
    z[8, mid], z[8, last] = 9.0, 9.0               # the maximum twice
    z[9, :] = nan                                  # all NaN
    z[10, mid], z[10, last] = inf, inf             # +inf twice
    z[11, 0], z[11, last] = -inf, nan              # -inf first, then a NaN
    return z


@pytest.mark.parametrize("C", [1, 2, 64, 65, 256])
def test_argmax_and_confusion_nan_order(C):
    """pcs_argmax and the argmax inside pcs_confusion (LDS histogram up to 64 classes, global
    atomics above) against torch.argmax on the CPU, rows of stride ld > C whose padding would
    win if it were read; labels -1 and C are skipped."""
    import pcs_amd._lib as L
    z = _special_logits(C)
    rows, ld = z.shape[0], C + 3
    buf = torch.full((rows, ld), float("nan"))
    buf[:, C + 1:] = float("inf")
    buf[:, :C] = z
    want = torch.argmax(z, dim=1)
    if C >= 3:
        assert want[:12].tolist() == [0, C // 2, C - 1, C // 2, C - 1, 0, 0, 0, C // 2, 0, C // 2, C - 1]
    g = torch.Generator().manual_seed(C)
    y = torch.randint(-1, C + 1, (rows,), generator=g)
    y[:12] = torch.arange(12) % C
    assert (y == -1).any() and (y == C).any()
    d_z, d_y = buf.to(DEV), y.to(DEV)
    out = torch.full((rows,), -1, dtype=torch.int64, device=DEV)
    cm = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    L.call("pcs_argmax", L.ptr(d_z), ld, rows, C, L.ptr(out), L.stream_ptr())
    L.call("pcs_confusion", L.ptr(d_z), ld, L.ptr(d_y), rows, C, L.ptr(cm), L.stream_ptr())
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got, want), [(i, z[i].tolist()[:4], int(got[i]), int(want[i]))
                                    for i in torch.nonzero(got != want).flatten().tolist()[:4]]
    ref = np.zeros((C, C), np.int64)
    v = ((y >= 0) & (y < C)).numpy()
    np.add.at(ref, (y.numpy()[v], want.numpy()[v]), 1)
    assert np.array_equal(cm.cpu().numpy(), ref)
    assert int(cm.sum()) == int(v.sum())


def test_confusion_meter_nan_logits():
    """ConfusionMeter on a diverged batch: the predictions are torch.argmax's."""
    from pcs_amd.metrics import ConfusionMeter
    z = torch.tensor([[1.0, float("nan"), 3.0], [1.0, float("inf"), float("nan")], [0.5, 0.25, 0.125]])
    y = torch.tensor([0, 1, -1])
    meter = ConfusionMeter(3, DEV).update(z.to(DEV), y.to(DEV))
    ref = np.zeros((3, 3), np.int64)
    ref[0, 1] = ref[1, 2] = 1                      # torch.argmax gives 1 and 2
    assert torch.argmax(z, 1).tolist() == [1, 2, 0]
    assert np.array_equal(meter.cm.cpu().numpy(), ref)
