"""The segmented max (pcs_amd.segmax) at BASELINE configs[2]'s scale: a 256^3 grid, 4 scenes of
jittered clouds occupying ~2 % of it (per_voxel = 2), C = w0 = 64, Cin = 4, bf16 in and out.

Each pass is timed against the torch composition it replaces, on the same tensors and index arrays,
and against the sum kernel that moves the same rows (its sibling), all alternating in one process:
    voxel_max        fwd / bwd | scatter_reduce_(amax) on fp32 [T, C] with autograd | voxel_mean
    sparse_max_pool  fwd / bwd | scatter_reduce_(amax) on fp32 [Vf, C] with autograd | -
    point_lift_max   fwd / bwd | voxel_max(relu(F.linear(points, W, b))) with autograd | point_lift_mean
A figure is the median of `reps` single calls timed with device events after a warm-up (a backward's
forward runs untimed before each timed call); the line gives min .. max of 5 such medians.  Bytes are
algorithmic (every source row, output row, index and picked-row entry once); peak memory is
torch.cuda.max_memory_allocated of one model.loss(rb).backward() above its start.
    timeout 900 python tools/bench_segmax.py [reps >= 10] [occupancy] [grid] [out file]"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcs_amd.data import jittered_clouds, ragged_collate  # noqa: E402
from pcs_amd.pointhead import point_lift_mean  # noqa: E402
from pcs_amd.pointvoxel import point_voxel_map, voxel_mean  # noqa: E402
from pcs_amd.segmax import point_lift_max, sparse_max_pool, voxel_max  # noqa: E402
from pcs_amd.sparse import coarsen, sparse_voxels  # noqa: E402
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
    pvm.points_by_voxel()
    svc, link = coarsen(sv)
    T, V, Vc = pvm.num_points, pvm.num_voxels, svc.num_voxels
    say(f"grid {G}^3 x {B} scenes, occupancy {occ}: T = {T} points, V = {V} voxels ({T / V:.2f} points per voxel), Vc = {Vc} "
        f"coarse voxels ({V / Vc:.2f} children per cell); C = {C}, Cin = {CIN}, bf16 -> bf16; median of {reps} calls, "
        f"min .. max of {ROUNDS} medians")

    torch.manual_seed(0)
    pts = rb.points.to(dev, torch.float32)
    lw = (torch.randn(C, CIN, device=dev) / 2).requires_grad_()
    lb = (torch.randn(C, device=dev) / 10).requires_grad_()
    xp = torch.randn(T, C, device=dev).to(BF).requires_grad_()
    xv = torch.randn(V, C, device=dev).to(BF).requires_grad_()
    dv = torch.randn(V, C, device=dev).to(BF)
    dc = torch.randn(Vc, C, device=dev).to(BF)
    own = pvm.own.long()[:, None].expand(T, C)          # (every point has its voxel: the level is built from them)
    par = link.parent.long()[:, None].expand(V, C)

    def amax(x, index, rows):
        return torch.zeros(rows, C, device=dev).scatter_reduce_(0, index, x.float(), "amax", include_self=False).to(BF)

    nothing = lambda: None                                            # noqa: E731
    row = 2 * C

    def fwd(fn):
        return (nothing, lambda _: fn())

    def bwd(fn, leaves, grad):
        return (fn, lambda y: torch.autograd.grad(y, leaves, grad))

    vmax, vtorch, vmean = (lambda: voxel_max(xp, pvm)), (lambda: amax(xp, own, V)), (lambda: voxel_mean(xp, pvm))
    pmax, ptorch = (lambda: sparse_max_pool(xv, link)), (lambda: amax(xv, par, Vc))
    lmax = lambda: point_lift_max(pts, lw, lb, pvm)                                   # noqa: E731
    ltorch = lambda: voxel_max(torch.relu(F.linear(pts[:, :CIN], lw, lb)), pvm)       # noqa: E731
    lmean = lambda: point_lift_mean(pts, lw, lb, pvm)                                 # noqa: E731
    passes = [
        ("voxel_max forward", [fwd(vmax), fwd(vtorch), fwd(vmean)], T * (row + 4) + V * (row + 8 + 4 * C)),
        ("voxel_max backward", [bwd(vmax, [xp], dv), bwd(vtorch, [xp], dv), bwd(vmean, [xp], dv)],
         V * (row + 4 * C) + T * (row + 4)),
        ("sparse_max_pool forward", [fwd(pmax), fwd(ptorch)], V * row + Vc * (row + 32 + 8 + 4 * C)),
        ("sparse_max_pool backward", [bwd(pmax, [xv], dc), bwd(ptorch, [xv], dc)], Vc * (row + 4 * C) + V * (row + 4)),
        ("point_lift_max forward", [fwd(lmax), fwd(ltorch), fwd(lmean)], T * (4 * CIN + 4) + V * (8 + row)),
        ("point_lift_max backward", [bwd(lmax, [lw, lb], dv), bwd(ltorch, [lw, lb], dv), bwd(lmean, [lw, lb], dv)],
         T * (4 * CIN + 4) + V * (8 + row)),
    ]
    say(f"{'pass':26s} {'HIP ms':>18s} {'MB':>6s} {'TB/s':>6s} | {'torch ms':>18s} {'HIP/torch':>9s} | {'sibling ms':>18s} "
        f"{'HIP/sibling':>11s}")
    not_faster = []
    for name, items, nbytes in passes:
        res = spread(items, reps)
        (h0, h1), (t0, t1) = res[0], res[1]
        sib = f"{res[2][0]:8.3f} ..{res[2][1]:8.3f} {h0 / res[2][0]:11.3f}" if len(res) > 2 else f"{'-':>18s} {'-':>11s}"
        say(f"{name:26s} {h0:8.3f} ..{h1:8.3f} {nbytes / 1e6:6.0f} {nbytes / h0 / 1e9:6.2f} | {t0:8.3f} ..{t1:8.3f} "
            f"{h1 / t0:9.3f} | {sib}")
        if not h1 < t0:
            not_faster.append(name)
    say("HIP/torch: the slowest HIP median over the fastest torch median; HIP/sibling: fastest over fastest")
    with torch.no_grad():
        d1 = float((vmax().float() - vtorch().float()).abs().max())
        d2 = float((pmax().float() - ptorch().float()).abs().max())
        d3 = float((lmax().float() - ltorch().float()).abs().max())
    say(f"outputs, max |HIP - torch|: voxel_max {d1:.3e}, sparse_max_pool {d2:.3e}, point_lift_max {d3:.3e}")
    del xp, xv, dv, dc, own, par
    torch.cuda.empty_cache()

    # the model's loss step with either lift, at the largest grid that fits
    cw = torch.tensor([1.0, 2.0], device=dev)
    for g in (G, G // 2, G // 4):
        try:
            rbm = rb if g == G else ragged_collate([(torch.from_numpy(p), torch.from_numpy(l))
                                                    for p, l in jittered_clouds(5, B, grid=g, occupancy=occ, per_voxel=2)])
            peaks = {}
            for lift in ("max", "mean"):
                torch.manual_seed(0)
                model = SparseUNetSegmentation(CIN, K, grid=g, lift=lift).to(dev)

                def step():
                    model.zero_grad(set_to_none=True)
                    model.loss(rbm, cw).backward()

                peaks[lift] = peak_of(step)
                del model
                torch.cuda.empty_cache()
        except torch.cuda.OutOfMemoryError:
            say(f"model step: grid {g} does not fit")
            torch.cuda.empty_cache()
            continue
        say(f"model loss step (grid {g}^3, T = {rbm.points.shape[0]}) peak memory above its start: lift='max' "
            f"{peaks['max'] / 1e6:.1f} MB, lift='mean' {peaks['mean'] / 1e6:.1f} MB")
        break
    say("every pass beats its torch composition by more than the spread" if not not_faster else
        "NOT faster than the torch composition beyond the spread: " + ", ".join(not_faster))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
