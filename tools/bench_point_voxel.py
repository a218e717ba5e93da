"""Point <-> voxel transfer at BASELINE configs[2]'s scale: a 256^3 grid, 4 scenes of jittered
clouds occupying ~2 % of it (per_voxel = 2), C = 64, bf16 in and out (pcs_amd.pointvoxel).

Each of the six uses of the two row kernels is timed against two yardsticks:
    bytes   its algorithmic bytes (every source row, output row, index and weight once) over time
    torch   the torch composition of the same operator on the same device and the same index
            arrays: index_select * weight .sum(1) for the gathers, index_add_ into fp32 for the
            grouped sums (an atomic scatter-add: neither ordered nor reproducible)
and both outputs are compared.  Every figure is the median of `reps` single launches timed with
device events after a warm-up, kernel and composition alternating.  The index build
(pcs_trilinear_index) and the two CSR builds (torch stable sort) are timed once each.
    timeout 900 python tools/bench_point_voxel.py [reps >= 10] [occupancy] [grid] [out file]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pcs_amd._lib as L  # noqa: E402
from pcs_amd.data import jittered_clouds, ragged_collate  # noqa: E402
from pcs_amd.pointvoxel import CORNERS, point_voxel_map  # noqa: E402
from pcs_amd.sparse import sparse_voxels  # noqa: E402
from pcs_amd.voxel import voxelize  # noqa: E402

BF = torch.bfloat16


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
    reps = max(10, int(sys.argv[1])) if len(sys.argv) > 1 else 20
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
    sv = sparse_voxels(rb, voxelize(rb, G))
    ms_index = medians([lambda: point_voxel_map(rb, sv)], 5, 1)[0]   # includes the host -> device copy of the points
    pvm = point_voxel_map(rb, sv)
    T, V = pvm.num_points, pvm.num_voxels
    ms_pts = medians([lambda: (setattr(pvm, "_points", None), pvm.points_by_voxel())], 5, 1)[0]
    ms_pairs = medians([lambda: (setattr(pvm, "_pairs", None), pvm.pairs_by_voxel())], 5, 1)[0]
    order, pt_off, counts, inv, inv_pt = pvm.points_by_voxel()
    pair_pt, pair_w, pair_off = pvm.pairs_by_voxel()
    NP = int(pair_off[-1])
    say(f"grid {G}^3 x {B} scenes, occupancy {occ}: {T} points, {V} voxels ({T / V:.2f} points per voxel, max "
        f"{int(counts.max())}), {NP} (point, corner) pairs ({NP / T:.2f} per point, {NP / V:.2f} per voxel, max "
        f"{int((pair_off[1:] - pair_off[:-1]).max())}), C = {C}, bf16 -> bf16, median of {reps} launches")
    say(f"point_voxel_map (copy + pcs_trilinear_index): {ms_index:.3f} ms | points-by-voxel CSR: {ms_pts:.3f} ms | "
        f"pairs-by-voxel CSR: {ms_pairs:.3f} ms (torch stable sort, once per map)")

    st = L.stream_ptr()
    xp = torch.randn(T, C, device=dev).to(BF)        # per-point rows (features or gradients)
    xv = torch.randn(V, C, device=dev).to(BF)        # per-voxel rows
    yp = torch.empty(T, C, device=dev, dtype=BF)
    yv = torch.empty(V, C, device=dev, dtype=BF)
    row = 2 * C

    def interp(x, idx, w, M, K, y):
        return lambda: L.call("pcs_rows_interp", L.ptr(x), L.BF16, L.ptr(idx), L.ptr(w), M, K, C, L.ptr(y), L.BF16, st)

    def segsum(x, src, w, off, scale, M, y):
        return lambda: L.call("pcs_rows_segsum", L.ptr(x), L.BF16, L.ptr(src), L.ptr(w), L.ptr(off), L.ptr(scale), M, C,
                              L.ptr(y), L.BF16, st)

    # the same index arrays in the form torch's ops take (int64, -1 clamped to row 0 under a zero weight)
    own = pvm.own.long()
    own_ok = (own >= 0)
    own0 = own.clamp_min(0)
    own_w = own_ok.float()[:, None]
    cor0 = pvm.corner.long().clamp_min(0).reshape(-1)
    wgt = pvm.weight[:, :, None]
    order64, pair_pt64 = order.long()[: int(pt_off[-1])], pair_pt.long()[:NP]
    own_sorted = own0[order64]
    pair_v = torch.repeat_interleave(torch.arange(V, device=dev), pair_off[1:] - pair_off[:-1])
    pair_w1 = pair_w[:NP, None]
    res = {}

    def t_mean_fwd():
        res["t"] = (torch.zeros(V, C, device=dev).index_add_(0, own_sorted, xp[order64].float()) * inv[:, None]).to(BF)

    def t_mean_bwd():
        res["t"] = (xv.index_select(0, own0).float() * inv_pt[:, None]).to(BF)

    def t_tri_fwd():
        res["t"] = (xv.index_select(0, cor0).view(T, CORNERS, C).float() * wgt).sum(1).to(BF)

    def t_tri_bwd():
        res["t"] = torch.zeros(V, C, device=dev).index_add_(0, pair_v, xp.index_select(0, pair_pt64).float() * pair_w1).to(BF)

    def t_near_fwd():
        res["t"] = (xv.index_select(0, own0).float() * own_w).to(BF)

    def t_near_bwd():
        res["t"] = torch.zeros(V, C, device=dev).index_add_(0, own_sorted, xp[order64].float()).to(BF)

    uses = [
        ("voxel_mean forward   (segsum, points CSR, scale)", segsum(xp, order, None, pt_off, inv, V, yv), t_mean_fwd, yv,
         T * row + V * row + 4 * T + 8 * V + 4 * V),
        ("voxel_mean backward  (interp K=1, w)", interp(xv, pvm.own, inv_pt, T, 1, yp), t_mean_bwd, yp,
         V * row + T * row + 8 * T),
        ("trilinear forward    (interp K=8, w)", interp(xv, pvm.corner, pvm.weight, T, CORNERS, yp), t_tri_fwd, yp,
         V * row + T * row + 64 * T),
        ("trilinear backward   (segsum, pairs CSR, w)", segsum(xp, pair_pt, pair_w, pair_off, None, V, yv), t_tri_bwd, yv,
         T * row + V * row + 8 * NP + 8 * V),
        ("nearest forward      (interp K=1)", interp(xv, pvm.own, None, T, 1, yp), t_near_fwd, yp,
         V * row + T * row + 4 * T),
        ("nearest backward     (segsum, points CSR)", segsum(xp, order, None, pt_off, None, V, yv), t_near_bwd, yv,
         T * row + V * row + 4 * T + 8 * V),
    ]
    say(f"{'use':52s} {'HIP ms':>8s} {'GB/s':>8s} {'MB':>7s} {'torch ms':>9s} {'HIP/torch':>9s} {'max |diff|':>10s}")
    slower = []
    for name, hip, comp, y, nbytes in uses:
        y.zero_()
        h, t = medians([hip, comp], reps)
        diff = float((y.float() - res["t"].float()).abs().max())
        if h > t:
            slower.append(name.split("(")[0].strip())
        say(f"{name:52s} {h:8.3f} {nbytes / h / 1e6:8.0f} {nbytes / 1e6:7.1f} {t:9.3f} {h / t:9.3f} {diff:10.3e}")
    say("every kernel is no slower than its torch composition" if not slower else
        "SLOWER than the torch composition: " + ", ".join(slower))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
