"""The fused point lift and point head (pcs_amd.pointhead) at BASELINE configs[2]'s scale: a 256^3
grid, 4 scenes of jittered clouds occupying ~2 % of it (per_voxel = 2), w0 = 64, Cin = 4, K = 2, bf16
voxel features.

Each pass is timed against the torch composition it replaces, on the same tensors and maps:
    lift forward      point_lift_mean            | voxel_mean(relu(F.linear(points, W, b)))
    lift backward     its autograd backward      | the composition's (dW, db)
    head + loss fwd   point_head_loss            | F.cross_entropy(F.linear(devoxelize(x), W, b))
    head + loss bwd   its autograd backward      | the composition's (dX, dW, db)
    model step        model.loss(rb).backward()  | F.cross_entropy(model(rb), labels).backward()
A figure is the median of `reps` single calls timed with device events after a warm-up, the fused
pass and the composition alternating in one process (a backward's forward runs untimed before each
timed call); the line gives min .. max of `rounds` such medians.  A fused pass counts as faster only
when its slowest median is below the composition's fastest.  Bytes are algorithmic (every array
once); peak memory is torch.cuda.max_memory_allocated above the step's start.
    timeout 900 python tools/bench_point_head.py [reps >= 10] [occupancy] [grid] [out file]"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcs_amd.data import jittered_clouds, ragged_collate  # noqa: E402
from pcs_amd.pointhead import point_head_loss, point_lift_mean  # noqa: E402
from pcs_amd.pointvoxel import devoxelize, point_voxel_map, voxel_mean  # noqa: E402
from pcs_amd.sparse import sparse_voxels  # noqa: E402
from pcs_amd.sparse_unet import SparseUNetSegmentation  # noqa: E402
from pcs_amd.voxel import voxelize  # noqa: E402

BF = torch.bfloat16
ROUNDS = 5


def medians(items, reps, warmup=2):
    """Median ms of each (prepare, run) over reps single calls, the items alternating; prepare runs
    untimed before its run and hands it its result."""
    for _ in range(warmup):
        for prep, run in items:
            run(prep())
    torch.cuda.synchronize()
    times = [[] for _ in items]
    for _ in range(reps):
        for i, (prep, run) in enumerate(items):
            state = prep()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(state)
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [statistics.median(t) for t in times]


def spread(items, reps, rounds=ROUNDS):
    """(min, max) of `rounds` medians for each item."""
    ms = [medians(items, reps) for _ in range(rounds)]
    return [(min(m[i] for m in ms), max(m[i] for m in ms)) for i in range(len(items))]


def peak_of(step):
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    reps = max(10, int(sys.argv[1])) if len(sys.argv) > 1 else 30
    occ = float(sys.argv[2]) if len(sys.argv) > 2 else 0.02
    G = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    out_path = sys.argv[4] if len(sys.argv) > 4 else None
    B, C, CIN, K = 4, 64, 4, 2
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    clouds = jittered_clouds(5, B, grid=G, occupancy=occ, per_voxel=2)
    rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])
    sv = sparse_voxels(rb, voxelize(rb, G))
    pvm = point_voxel_map(rb, sv)
    pvm.points_by_voxel(), pvm.pairs_by_voxel()
    T, V = pvm.num_points, pvm.num_voxels
    NP = int(pvm.pairs_by_voxel()[2][-1])
    say(f"grid {G}^3 x {B} scenes, occupancy {occ}: T = {T} points, V = {V} voxels, {NP} (point, corner) pairs; w0 = {C}, "
        f"Cin = {CIN}, K = {K}, bf16 voxel features; median of {reps} calls, min .. max of {ROUNDS} medians")

    torch.manual_seed(0)
    pts = rb.points.to(dev, torch.float32)
    labels = rb.labels.to(dev)
    cw = torch.tensor([1.0, 2.0], device=dev)
    lw = (torch.randn(C, CIN, device=dev) / 2).requires_grad_()
    lb = (torch.randn(C, device=dev) / 2).requires_grad_()
    hw = (torch.randn(K, C, device=dev) / 8).requires_grad_()
    hb = torch.randn(K, device=dev).requires_grad_()
    x = torch.randn(V, C, device=dev).to(BF).requires_grad_()
    dv = torch.randn(V, C, device=dev).to(BF)

    def lift_fused():
        return point_lift_mean(pts, lw, lb, pvm)

    def lift_torch():
        return voxel_mean(torch.relu(F.linear(pts[:, :CIN], lw, lb)), pvm)

    def loss_fused():
        return point_head_loss(x, pvm, hw, hb, labels, cw)

    def loss_torch():
        return F.cross_entropy(F.linear(devoxelize(x, pvm), hw, hb), labels, weight=cw, ignore_index=-1)

    nothing = lambda: None                                            # noqa: E731
    passes = [
        ("lift forward", (nothing, lambda _: lift_fused()), (nothing, lambda _: lift_torch()),
         T * (4 * CIN + 4) + V * (8 + 4 + 2 * C)),
        ("lift backward", (lift_fused, lambda y: torch.autograd.grad(y, [lw, lb], dv)),
         (lift_torch, lambda y: torch.autograd.grad(y, [lw, lb], dv)),
         T * (4 * CIN + 4) + V * (8 + 4 + 2 * C)),
        ("head + loss forward", (nothing, lambda _: loss_fused()), (nothing, lambda _: loss_torch()),
         V * (2 * C + 8 * K) + T * (64 + 8 + 4 * K)),
        ("head + loss backward", (loss_fused, lambda l: torch.autograd.grad(l, [x, hw, hb])),
         (loss_torch, lambda l: torch.autograd.grad(l, [x, hw, hb])),
         T * 4 * K + NP * 8 + V * (8 + 8 * K + 4 * C)),
    ]
    say(f"{'pass':22s} {'fused ms':>20s} {'MB':>7s} {'TB/s':>6s} | {'torch ms':>20s} | fused / torch")
    not_faster = []
    for name, fused, comp, fbytes in passes:
        (f0, f1), (t0, t1) = spread([fused, comp], reps)
        say(f"{name:22s} {f0:8.3f} .. {f1:8.3f} {fbytes / 1e6:7.0f} {fbytes / f0 / 1e9:6.2f} | {t0:8.3f} .. {t1:8.3f} | "
            f"{f1 / t0:.3f} (worst over best)")
        if not f1 < t0:
            not_faster.append(name)
    with torch.no_grad():
        ya, yb = lift_fused().float(), lift_torch().float()
    la, lt = loss_fused(), loss_torch()
    ga, gt = torch.autograd.grad(la, [x, hw, hb]), torch.autograd.grad(lt, [x, hw, hb])
    say(f"outputs: lift max |diff| {float((ya - yb).abs().max()):.3e} (max |y| {float(yb.abs().max()):.3e}); loss "
        f"{la.item():.7f} against {lt.item():.7f}; dX max |diff| {float((ga[0].float() - gt[0].float()).abs().max()):.3e} "
        f"(max {float(gt[0].float().abs().max()):.3e}); dW max |diff| {float((ga[1] - gt[1]).abs().max()):.3e} "
        f"(max {float(gt[1].abs().max()):.3e})")
    del ya, yb, la, lt, ga, gt
    torch.cuda.empty_cache()

    # the whole model, at the largest grid that fits
    for g in (G, G // 2, G // 4):
        try:
            torch.manual_seed(0)
            model = SparseUNetSegmentation(CIN, K, grid=g).to(dev)
            rbm = rb if g == G else ragged_collate([(torch.from_numpy(p), torch.from_numpy(l))
                                                    for p, l in jittered_clouds(5, B, grid=g, occupancy=occ, per_voxel=2)])
            lab = rbm.labels.to(dev)

            def step_fused():
                model.zero_grad(set_to_none=True)
                model.loss(rbm, cw).backward()

            def step_torch():
                model.zero_grad(set_to_none=True)
                F.cross_entropy(model(rbm), lab, weight=cw, ignore_index=-1).backward()

            mreps = max(5, reps // 3)
            (f0, f1), (t0, t1) = spread([(nothing, lambda _: step_fused()), (nothing, lambda _: step_torch())], mreps, 3)
            pf, pt = peak_of(step_fused), peak_of(step_torch)
        except torch.cuda.OutOfMemoryError:
            say(f"model step: grid {g} does not fit")
            model = None
            torch.cuda.empty_cache()
            continue
        tm = rbm.points.shape[0]
        say(f"model step (grid {g}^3, T = {tm}, widths {model.unet.widths}, forward + backward, median of {mreps}, min .. max of "
            f"3): fused {f0:.3f} .. {f1:.3f} ms, default {t0:.3f} .. {t1:.3f} ms, {f1 / t0:.3f} (worst over best)")
        say(f"model step peak memory above its start: fused {pf / 1e6:.1f} MB, default {pt / 1e6:.1f} MB, saved "
            f"{(pt - pf) / 1e6:.1f} MB (T * w0 * 4 = {tm * C * 4 / 1e6:.1f} MB)")
        if not f1 < t0:
            not_faster.append("model step")
        break
    say("every fused pass beats its composition by more than the spread" if not not_faster else
        "NOT faster than the composition beyond the spread: " + ", ".join(not_faster))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
