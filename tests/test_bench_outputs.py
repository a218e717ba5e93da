"""bench.py's --dump-outputs writer and argument checks (CPU): the writer stores the loss, every
parameter's gradient and value and the BatchNorm running statistics as float32 .npy files named
after them, and --steps 0 is refused instead of timing nothing."""
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def test_dump_outputs_writes_named_float32_arrays(tmp_path):
    sys.path.insert(0, REPO)
    import bench
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.BatchNorm1d(5)).double()
    loss = m(torch.randn(7, 3, dtype=torch.float64)).square().mean()
    loss.backward()
    out = str(tmp_path / "nested" / "dump")
    bench.dump_outputs(out, m, loss)
    want = {"loss": loss.detach().reshape(1)}
    for n, p in m.named_parameters():
        want[f"grad.{n}"] = p.grad
        want[f"param.{n}"] = p.detach()
    want["buffer.1.running_mean"] = m[1].running_mean
    want["buffer.1.running_var"] = m[1].running_var
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)   # no num_batches_tracked
    for k, t in want.items():
        a = np.load(os.path.join(out, k + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(t.shape), k
        np.testing.assert_array_equal(a, t.to(torch.float32).numpy(), err_msg=k)


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2
    assert "--steps" in r.stderr
