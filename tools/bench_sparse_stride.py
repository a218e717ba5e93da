"""Stride-2 sparse down / up convolutions at BASELINE configs[2]'s scale: a 256^3 grid, jittered
clouds occupying ~2 % of it, 4 scenes, 64 -> 64 channels, coarsened once (pcs_amd.sparse.coarsen).

The one-tap-per-row direction (the up forward, the down input gradient) is timed two ways on the
same maps in the same process, launches alternating:
    rows   pcs_sparse_conv_rows (Y written directly)
    pairs  pcs_sparse_conv_pairs on the one-hot up map (Z fp32 round trip + reduce): the baseline
and both outputs are compared.  The down forward / up input gradient (8-tap gather, both forms)
and the two weight gradients are timed for completeness.  Every figure is the median of `reps`
single launches timed with device events, after a warm-up.
    timeout 600 python tools/bench_sparse_stride.py [reps >= 20] [occupancy] [grid]"""
import ctypes as ct
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pcs_amd._lib as L  # noqa: E402
from pcs_amd.data import jittered_clouds, ragged_collate  # noqa: E402
from pcs_amd.sparse import K2_TAPS, coarsen, sparse_voxels  # noqa: E402
from pcs_amd.voxel import voxelize  # noqa: E402


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
    reps = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 30
    occ = float(sys.argv[2]) if len(sys.argv) > 2 else 0.02
    G = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    B, C, T = 4, 64, K2_TAPS
    dev = torch.device("cuda")
    clouds = jittered_clouds(5, B, grid=G, occupancy=occ, per_voxel=2)
    rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])
    sv = sparse_voxels(rb, voxelize(rb, G))
    ms_coarsen = medians([lambda: coarsen(sv)], 5, 1)[0]
    svc, link = coarsen(sv)
    Vf, Vc = link.fine, link.coarse
    st = L.stream_ptr()
    upin, upout, uppos, utap, UP = link.up_pairs()
    dpin, dpout, dppos, dtap, DP = link.down_pairs()
    uta, dta = ct.addressof(utap), ct.addressof(dtap)
    print(f"grid {G}^3 x {B} scenes, occupancy {occ}: {Vf} fine voxels, {Vc} coarse ({Vf / Vc:.2f} children per cell), "
          f"{C} -> {C} channels, median of {reps} launches", flush=True)
    print(f"up-map pairs per tap: {[utap[t + 1] - utap[t] for t in range(T)]}", flush=True)
    print(f"coarsen (keys, unique, coarse table + neighbours, maps): {ms_coarsen:.3f} ms", flush=True)

    xf = torch.randn(Vf, C, device=dev).to(torch.bfloat16)
    xc = torch.randn(Vc, C, device=dev).to(torch.bfloat16)
    w = (torch.randn(C, T * C, device=dev) * 0.05).to(torch.bfloat16)
    bias = torch.randn(C, device=dev)
    yr = torch.empty(Vf, C, device=dev, dtype=torch.bfloat16)
    yp = torch.empty(Vf, C, device=dev, dtype=torch.bfloat16)
    z = torch.empty(max(UP, DP, 1), C, device=dev)
    useful = 2.0 * Vf * C * C / 1e12

    def rows(b):
        return lambda: L.call("pcs_sparse_conv_rows", L.ptr(upin), L.ptr(upout), uta, T, Vf, L.ptr(xc), C, L.ptr(w), C,
                              L.ptr(b), L.ptr(yr), L.BF16, st)

    def pairs(b):
        return lambda: L.call("pcs_sparse_conv_pairs", L.ptr(upin), L.ptr(uppos), uta, T, Vf, L.ptr(xc), C, L.ptr(w), C,
                              L.ptr(b), L.ptr(z), L.ptr(yp), L.BF16, 0, st)

    verdict = []
    for name, b in (("up forward (bias)", bias), ("down input gradient (no bias)", None)):
        yr.zero_(), yp.fill_(1.0)
        r, p = medians([rows(b), pairs(b)], reps)
        same = torch.equal(yr, yp)
        verdict.append(r <= p)
        print(f"{name}: rows {r:.3f} ms ({useful / r * 1e3:.1f} TF/s) | pairs baseline {p:.3f} ms "
              f"({useful / p * 1e3:.1f} TF/s) | rows / pairs = {r / p:.3f} | outputs identical: {same}", flush=True)

    yc = torch.empty(Vc, C, device=dev, dtype=torch.bfloat16)
    gat = lambda: L.call("pcs_sparse_conv", L.ptr(link.child), Vc, T, L.ptr(xf), C, L.ptr(w), C, L.ptr(bias), L.ptr(yc), L.BF16, 0, st)  # noqa: E731
    gpr = lambda: L.call("pcs_sparse_conv_pairs", L.ptr(dpin), L.ptr(dppos), dta, T, Vc, L.ptr(xf), C, L.ptr(w), C, L.ptr(bias), L.ptr(z), L.ptr(yc), L.BF16, 0, st)  # noqa: E731
    g, p = medians([gat, gpr], reps)
    print(f"down forward / up input gradient (8-tap gather): tile gather {g:.3f} ms | pair lists {p:.3f} ms "
          f"(the layers take {'the pair lists' if link.use_pairs() else 'the tile gather'})", flush=True)

    dw = torch.empty(C, T * C, device=dev)
    db = torch.empty(C, device=dev)
    nbd = int(L.load().pcs_sparse_conv_wgrad_pairs_workspace(dta, T, Vc, C, C))
    nbu = int(L.load().pcs_sparse_conv_wgrad_pairs_workspace(uta, T, Vf, C, C))
    ws = torch.empty(max(nbd, nbu) // 4, device=dev)
    wd = lambda: L.call("pcs_sparse_conv_wgrad_pairs", L.ptr(dpin), L.ptr(dpout), dta, T, Vc, L.ptr(xf), C, L.ptr(yc), C, L.ptr(ws), nbd, L.ptr(dw), L.ptr(db), st)  # noqa: E731
    wu = lambda: L.call("pcs_sparse_conv_wgrad_pairs", L.ptr(upin), L.ptr(upout), uta, T, Vf, L.ptr(xc), C, L.ptr(yr), C, L.ptr(ws), nbu, L.ptr(dw), L.ptr(db), st)  # noqa: E731
    d, u = medians([wd, wu], reps)
    print(f"weight gradient (pair lists): down {d:.3f} ms | up {u:.3f} ms", flush=True)
    print("pcs_sparse_conv_rows is " + ("no slower than" if all(verdict) else "SLOWER than") + " the pair-list baseline",
          flush=True)


if __name__ == "__main__":
    main()
