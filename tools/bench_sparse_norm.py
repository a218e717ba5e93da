"""Sparse BatchNorm (+ residual) + ReLU at BASELINE configs[2]'s scale: the occupied voxels of a
256^3 grid, 4 scenes at ~2 % occupancy, C = 64, bf16 in and out (pcs_amd.sparse_norm).

The forward and the backward of BN+ReLU and of BN+residual+ReLU are timed against two yardsticks:
    bytes   the algorithmic bytes: 4 passes over a [V, C] bf16 array forward (x twice, the residual
            or nothing, y; counted as 4 either way), 7 backward (dy, y, x, dz out; dz, x, dx out), over time
    torch   the torch composition on the same tensors, with autograd: F.batch_norm on an fp32
            up-cast, + residual, relu, a cast down
and the outputs and gradients of the two are compared.  Every figure is the median of `reps` single
launches of a whole forward (or backward) timed with device events after a warm-up, the two
alternating, in one process.
    timeout 900 python tools/bench_sparse_norm.py [reps >= 10] [occupancy] [grid] [out file]"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcs_amd.data import jittered_clouds, ragged_collate  # noqa: E402
from pcs_amd.sparse import sparse_voxels  # noqa: E402
from pcs_amd.sparse_norm import sparse_batch_norm  # noqa: E402
from pcs_amd.voxel import voxelize  # noqa: E402

BF = torch.bfloat16
FWD_PASSES, BWD_PASSES = 4, 7


def medians(fns, reps, warmup=3):
    """Median ms of each fn over reps single launches, the fns alternating."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for i, fn in enumerate(fns):
            ev[i][r][0].record()
            fn()
            ev[i][r][1].record()
    torch.cuda.synchronize()
    return [statistics.median(s.elapsed_time(e) for s, e in row) for row in ev]


def main():
    reps = max(10, int(sys.argv[1])) if len(sys.argv) > 1 else 30
    occ = float(sys.argv[2]) if len(sys.argv) > 2 else 0.02
    G = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    B, C = 4, 64
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    clouds = jittered_clouds(5, B, grid=G, occupancy=occ, per_voxel=2)
    rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])
    V = sparse_voxels(rb, voxelize(rb, G)).num_voxels
    array = V * C * 2
    say(f"grid {G}^3 x {B} scenes, occupancy {occ}: {V} voxels, C = {C}, bf16 -> bf16 ({array / 1e6:.1f} MB per [V, C] "
        f"array), median of {reps} launches; bytes = {FWD_PASSES} arrays forward, {BWD_PASSES} backward")

    torch.manual_seed(0)
    x = (torch.randn(V, C, device=dev) * 1.5 + 0.3).to(BF).requires_grad_()
    res = torch.randn(V, C, device=dev).to(BF).requires_grad_()
    dy = torch.randn(V, C, device=dev).to(BF)
    gamma = torch.empty(C, device=dev).uniform_(0.5, 1.5).requires_grad_()
    beta = (0.2 * torch.randn(C, device=dev)).requires_grad_()
    leaves = (x, res, gamma, beta)

    def hip(r):
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        return lambda: sparse_batch_norm(x, gamma, beta, rm, rv, True, relu=True, residual=r)

    def composition(r):
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)

        def fwd():
            t = F.batch_norm(x.float(), rm, rv, gamma, beta, True, 0.1, 1e-5)
            if r is not None:
                t = t + r.float()
            return torch.relu(t).to(BF)
        return fwd

    def grads(y):
        for t in leaves:
            t.grad = None
        y.backward(dy, retain_graph=True)
        return [t.grad for t in leaves]

    say(f"{'layer':28s} {'pass':9s} {'HIP ms':>8s} {'TB/s':>6s} {'torch ms':>9s} {'HIP/torch':>9s} {'max |diff|':>10s}")
    slower = []
    for name, r in (("BN + ReLU", None), ("BN + residual + ReLU", res)):
        f_hip, f_torch = hip(r), composition(r)
        h, t = medians([f_hip, f_torch], reps)
        y_hip, y_torch = f_hip(), f_torch()
        diff = float((y_hip.detach().float() - y_torch.detach().float()).abs().max())
        say(f"{name:28s} {'forward':9s} {h:8.3f} {FWD_PASSES * array / h / 1e9:6.2f} {t:9.3f} {h / t:9.3f} {diff:10.3e}")
        if h > t:
            slower.append(f"{name} forward")
        h, t = medians([lambda: grads(y_hip), lambda: grads(y_torch)], reps)
        g_hip = [g.float().clone() if g is not None else None for g in grads(y_hip)]
        g_torch = [g.float().clone() if g is not None else None for g in grads(y_torch)]
        diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(g_hip, g_torch)
                   if a is not None)
        say(f"{name:28s} {'backward':9s} {h:8.3f} {BWD_PASSES * array / h / 1e9:6.2f} {t:9.3f} {h / t:9.3f} {diff:10.3e}"
            "  (gradients: max norm-relative)")
        if h > t:
            slower.append(f"{name} backward")
    say("every pass is no slower than its torch composition" if not slower else
        "SLOWER than the torch composition: " + ", ".join(slower))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
