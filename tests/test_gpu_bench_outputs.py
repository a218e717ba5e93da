"""bench.py on the device, in-process at a 16^3 grid (4 scenes x 4096 points): a plain run times
exactly --steps steps and reports nothing that needs runs of its own; --full adds the HIP-event
figures; --dump-outputs writes the last timed step's outputs, taken before --full's extra steps,
and the same arguments give the same inputs.

Run-to-run bound: the runs share inputs, initial weights and dropout seeds, so they differ only
by summation order (atomics, split reductions).  That moves a stored bf16 activation by a few
ulps at most (bf16 epsilon 2^-8 = 3.9e-3), so every gradient array agrees to 1e-2 of its norm
(norms below 1e-3 of the largest array's are rounding noise of analytically-zero gradients, the
BN-cancelled biases, and are measured against that floor, as tests/test_gpu_rccl.py does);
another seed or batch moves the gradients by O(1) of their norm."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID, SCENES = 16, 4
ARGS = ["--gpus", "1", "--grid", str(GRID), "--scenes", str(SCENES), "--steps", "1", "--warmup", "0"]


def _bench(monkeypatch, capsys, args):
    sys.path.insert(0, REPO)
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", [os.path.join(REPO, "bench.py")] + args)
    bench.main()
    cap = capsys.readouterr()
    lines = cap.out.strip().splitlines()
    assert len(lines) == 1, cap.out   # ONE result line
    return json.loads(lines[0]), cap.err


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def plain_dump(tmp_path_factory):
    """The plain run's line and dump, computed once and shared."""
    d = str(tmp_path_factory.mktemp("plain"))
    mp = pytest.MonkeyPatch()
    try:
        import contextlib
        import io
        buf = io.StringIO()
        sys.path.insert(0, REPO)
        import bench
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
            mp.delenv(k, raising=False)
        mp.setattr(sys, "argv", [os.path.join(REPO, "bench.py")] + ARGS + ["--dump-outputs", d])
        with contextlib.redirect_stdout(buf):
            bench.main()
    finally:
        mp.undo()
    return json.loads(buf.getvalue().strip().splitlines()[-1]), _load(d)


def _assert_same_step(a, b):
    assert sorted(a) == sorted(b)
    gmax = max(np.linalg.norm(v.astype(np.float64)) for k, v in b.items() if k.startswith("grad."))
    for k in b:
        x, y = a[k].astype(np.float64), b[k].astype(np.float64)
        if k.startswith("grad."):
            err = np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-3 * gmax)
            print(f"{k}: run-to-run {err:.2e}")
            assert err <= 1e-2, (k, err)
    assert abs(float(a["loss"][0]) - float(b["loss"][0])) <= 1e-2 * abs(float(b["loss"][0]))


def _assert_one_adam_step_from_init(arrays):
    """The dumped parameters are ONE Adam step (lr 1e-3) from the seeded initial weights: in the
    first step |m_hat / (sqrt(v_hat) + eps)| <= 1, so no entry moves further than lr (plus the
    fp32 rounding of the step size and of the entry)."""
    import torch
    from pcs_amd.model import PointNetSegmentation
    torch.manual_seed(0)
    moved = 0.0
    for n, p in PointNetSegmentation(2, compute_dtype="bf16").named_parameters():
        p = p.detach().numpy()
        d = np.abs(arrays[f"param.{n}"] - p)
        assert d.max() <= 1e-3 * (1 + 1e-4) + 1e-6 * np.abs(p).max(), n
        moved = max(moved, float(d.max()))
    assert moved >= 0.9e-3   # and the step was taken


def test_plain_run_times_the_steps_and_nothing_else(monkeypatch, capsys):
    rec, err = _bench(monkeypatch, capsys, ["--gpus", "1", "--grid", str(GRID), "--scenes", str(SCENES),
                                            "--steps", "3", "--warmup", "1"])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "M points/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["ms_per_step"] > 0
    # value and ms_per_step describe the same timed region: points per step / step time
    # (ms_per_step is rounded to 1e-3 ms: sub-millisecond steps here, hence the 1 % slack)
    points = SCENES * GRID ** 3
    assert rec["value"] == pytest.approx(points / rec["ms_per_step"] / 1e3, rel=1e-2)
    assert rec["roofline"] is None and rec["northstar_64x64"] is None and rec["cpu_baseline"] is None
    assert "per-kernel" not in err


def test_dump_holds_the_last_steps_outputs(plain_dump):
    from pcs_amd.model import PointNetSegmentation
    rec, arrays = plain_dump
    model = PointNetSegmentation(2, compute_dtype="bf16")
    want = {"loss": (1,)}
    for n, p in model.named_parameters():
        want[f"grad.{n}"] = want[f"param.{n}"] = tuple(p.shape)
    for n, b in model.named_buffers():
        if n.endswith(("running_mean", "running_var")):
            want[f"buffer.{n}"] = tuple(b.shape)
    assert sorted(arrays) == sorted(want)
    for k, a in arrays.items():
        assert a.dtype == np.float32 and a.shape == want[k] and np.isfinite(a).all(), k
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    assert float(arrays["loss"][0]) == pytest.approx(rec["loss"], abs=1e-6)
    assert any(np.abs(arrays[k]).max() > 0 for k in arrays if k.startswith("grad."))
    _assert_one_adam_step_from_init(arrays)


def test_same_arguments_give_the_same_step(plain_dump, monkeypatch, capsys, tmp_path):
    _bench(monkeypatch, capsys, ARGS + ["--dump-outputs", str(tmp_path)])
    _assert_same_step(_load(str(tmp_path)), plain_dump[1])


def test_full_adds_kernel_figures_and_dumps_before_its_extra_steps(plain_dump, monkeypatch, capsys, tmp_path):
    rec, err = _bench(monkeypatch, capsys, ARGS + ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)])
    assert rec["roofline"] is not None and rec["roofline"]["kernel"].endswith(":global_feat")
    assert rec["northstar_64x64"] is not None and rec["cpu_baseline"] is None
    assert "per-kernel" in err
    got = _load(str(tmp_path))
    _assert_same_step(got, plain_dump[1])
    # the dump is the timed step's, not the state after the two extra per-kernel steps (Adam
    # moves most entries by lr in each of them)
    _assert_one_adam_step_from_init(got)
