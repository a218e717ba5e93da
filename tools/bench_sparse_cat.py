"""The two-source submanifold convolution (pcs_amd.sparse.submanifold_conv3d_cat) at BASELINE
configs[2]'s scale: the occupied voxels of a 256^3 grid, 4 scenes at ~2 % occupancy, CA = CB = 64
-> 64, bf16 in and out: a U-Net decoder's convolution of (up, skip).

Two forms of the same layer on the same tensors and maps, alternating in one process:
    cat-free   submanifold_conv3d_cat(xa, xb, w, sv)
    torch.cat  submanifold_conv3d(torch.cat([xa, xb], 1), w, sv) and, in the backward, the two
               .contiguous() slices of dx (what a decoder did before the two-source layer)
The forward, the backward (a fresh forward outside the timed region before each) and both are
timed; every figure is the median of `reps` single launches timed with device events after a
warm-up, with the min .. max of `rounds` such medians beside it (the run-to-run spread).  The
outputs and gradients of the two forms are compared bit for bit, and torch.cuda.max_memory_allocated
of one forward + backward of each form is printed above the memory held before it.
    timeout 900 python tools/bench_sparse_cat.py [reps >= 10] [occupancy] [grid] [out file]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcs_amd.data import jittered_clouds, ragged_collate  # noqa: E402
from pcs_amd.sparse import sparse_voxels, submanifold_conv3d, submanifold_conv3d_cat  # noqa: E402
from pcs_amd.voxel import voxelize  # noqa: E402

BF = torch.bfloat16
ROUNDS = 5


def medians(fns, reps, setups=None, warmup=3):
    """Median ms of each fn over reps single launches, the fns alternating; setups[i]() runs untimed
    before every launch of fns[i]."""
    setups = setups or [lambda: None] * len(fns)
    for _ in range(warmup):
        for su, fn in zip(setups, fns):
            su()
            fn()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for i, (su, fn) in enumerate(zip(setups, fns)):
            su()
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
    B, CA, CB, COUT = 4, 64, 64, 64
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    clouds = jittered_clouds(5, B, grid=G, occupancy=occ, per_voxel=2)
    rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])
    sv = sparse_voxels(rb, voxelize(rb, G))
    V = sv.num_voxels
    sv.pairs()
    say(f"grid {G}^3 x {B} scenes, occupancy {occ}: {V} voxels, {int((sv.nbr >= 0).sum()) / V:.2f} occupied taps per "
        f"voxel ({'pair lists' if sv.use_pairs() else 'tile gather'}), CA = {CA}, CB = {CB} -> {COUT}, bf16 -> bf16; "
        f"a [V, CA + CB] bf16 array is {2 * V * (CA + CB) / 1e6:.1f} MB; median of {reps} launches, "
        f"min .. max of {ROUNDS} medians")

    torch.manual_seed(0)
    xa = torch.randn(V, CA, device=dev).to(BF).requires_grad_()
    xb = torch.randn(V, CB, device=dev).to(BF).requires_grad_()
    w = (torch.randn(COUT, CA + CB, 3, 3, 3, device=dev) * 0.05).to(BF).float().requires_grad_()
    dy = torch.randn(V, COUT, device=dev).to(BF)
    leaves = (xa, xb, w)

    def f_cat():
        return submanifold_conv3d_cat(xa, xb, w, sv)

    def f_ref():
        return submanifold_conv3d(torch.cat([xa, xb], 1), w, sv)

    def backward(y):
        for t in leaves:
            t.grad = None
        y.backward(dy)
        # the decoder's two branches take contiguous gradients: torch.cat's backward returns them so
        return xa.grad, xb.grad, w.grad

    forms = (("cat-free", f_cat), ("torch.cat", f_ref))
    held = {}

    def fwd_only(f):
        return lambda: f()

    def setup(name, f):
        def su():
            held[name] = f()
        return su

    def bwd_only(name):
        return lambda: backward(held.pop(name))

    def both(f):
        return lambda: backward(f())

    rows = {}
    for label, fns, sus in (
            ("forward", [fwd_only(f) for _, f in forms], None),
            ("backward", [bwd_only(n) for n, _ in forms], [setup(n, f) for n, f in forms]),
            ("forward + backward", [both(f) for _, f in forms], None)):
        meds = [medians(fns, reps, sus) for _ in range(ROUNDS)]
        rows[label] = [[m[i] for m in meds] for i in range(len(forms))]
    say(f"{'pass':20s} {'cat-free ms':>12s} {'(min .. max)':>18s} {'torch.cat ms':>13s} {'(min .. max)':>18s} {'ratio':>6s}")
    for label, (a, b) in rows.items():
        ma, mb = statistics.median(a), statistics.median(b)
        say(f"{label:20s} {ma:12.3f} {f'({min(a):.3f} .. {max(a):.3f})':>18s} {mb:13.3f} "
            f"{f'({min(b):.3f} .. {max(b):.3f})':>18s} {ma / mb:6.3f}")
    tot = rows["forward + backward"]
    say("the two-source layer is " + ("faster" if statistics.median(tot[0]) < statistics.median(tot[1]) else "NOT faster")
        + " in total at this shape")

    # bit-equality of the two forms
    got = [f_cat().detach()] + [g.clone() for g in backward(f_cat())]
    ref = [f_ref().detach()] + [g.clone() for g in backward(f_ref())]
    same = all(torch.equal(a, b) for a, b in zip(got, ref))
    say("outputs and gradients (y, dxa, dxb, dW) of the two forms: " + ("bit-identical" if same else "DIFFERENT"))

    # peak memory of one forward + backward above what is held before it
    del got, ref
    held.clear()
    for name, f in forms:
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        y = f()
        after_fwd = torch.cuda.memory_allocated() - base
        backward(y)
        del y
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        say(f"{name:10s} max_memory_allocated {peak / 1e6:9.1f} MB = {base / 1e6:.1f} MB held before + "
            f"{(peak - base) / 1e6:.1f} MB; held by the forward for the backward (with y) {after_fwd / 1e6:.1f} MB")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
