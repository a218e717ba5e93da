"""The inference path of the voxel U-Nets (pcs_amd.fold) against the existing eval path, on one MI355X, one
section per call (each appends to the out file, default profiles/bench_unet_infer.txt):

    layers   one convolution -> BatchNorm (+ residual) + ReLU layer, folded (fold.conv_bn, one kernel) against
             the existing eval pair (the convolution, then SparseBatchNorm / VoxelBatchNorm in eval mode, under
             torch.no_grad()) on the same tensors, with and without a residual, bf16 in and out:
               sparse  SubMConv3d 64 -> 64 at 256^3 x 4 scenes, 2 % occupied
               dense   Conv3d 64 -> 64 at 4 x 64^3, and Conv3dCat 32 + 32 -> 32 at 4 x 128^3
    sparse   SparseUNetSegmentation(widths=(64, 128, 256), grid=256).predict(rb) against model.eval() +
             torch.no_grad() + model(rb, fused=True) + argmax on the 256^3 x 4, 2 % batch: ms per call and
             torch.cuda.max_memory_allocated of each.
    dense    the same for VoxelUNetSegmentation(widths=(32, 64, 128), grid=128) on a fully occupied 4 x 128^3
             batch.

The baseline is always the existing path in the same process, the two forms alternating.  Every time is the
median of `reps` single calls timed with device events after a warm-up, with the min .. max of ROUNDS such
medians beside it (the run-to-run spread).
    timeout 900 python tools/bench_unet_infer.py SECTION [--reps N] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pcs_amd.data import jittered_clouds, ragged_collate, synthetic_clouds  # noqa: E402
from pcs_amd.fold import conv_bn  # noqa: E402

BF = torch.bfloat16
ROUNDS = 5
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def medians(fns, reps, warmup=3):
    """Median ms of each fn over reps single calls, the fns alternating."""
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


def compare(label, folded, existing, reps, note=""):
    """One line: the folded form against the existing one, medians of ROUNDS rounds and their spread."""
    meds = [medians([folded, existing], reps) for _ in range(ROUNDS)]
    a, b = [m[0] for m in meds], [m[1] for m in meds]
    ma, mb = statistics.median(a), statistics.median(b)
    say(f"{label:34s} folded {ma:8.3f} ms ({min(a):.3f} .. {max(a):.3f})   existing {mb:8.3f} ms ({min(b):.3f} .. {max(b):.3f})"
        f"   folded / existing {ma / mb:5.3f}, saves {mb - ma:7.3f} ms{note}")
    return ma, mb


def _randomise(bn, g):
    with torch.no_grad():
        c = bn.num_features
        bn.weight.copy_((0.5 + torch.rand(c, generator=g)) * (torch.randint(0, 2, (c,), generator=g) * 2 - 1))
        bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.5)
        bn.running_var.copy_(0.5 + 1.5 * torch.rand(c, generator=g))
    return bn.eval()


def _layer(title, conv, bn, xs, tail, res, reps):
    """Times conv_bn against bn(conv(.)) without and with the residual res; checks the outputs first."""
    say(f"-- {title}; median of {reps} calls, min .. max of {ROUNDS} medians")
    with torch.no_grad():
        for r in (None, res):
            got, ref32 = conv_bn(conv, bn, *xs, *tail, residual=r), bn(conv(*xs, *tail, out_dtype=torch.float32), residual=r,
                                                                       out_dtype=BF)
            ref = bn(conv(*xs, *tail), residual=r)
            same = torch.equal(got.view(torch.int16), ref32.view(torch.int16))
            d = float((got.float() - ref.float()).abs().max())
            say(f"   residual {'yes' if r is not None else 'no ':3s}: folded output " + ("bit-identical to" if same else "DIFFERENT from")
                + f" the pair with an fp32 intermediate; max |folded - existing bf16 pair| = {d:.3e} (one bf16 rounding less)")
            del got, ref32, ref

        def pair(r):
            return lambda: bn(conv(*xs, *tail), residual=r)

        for r, name in ((None, "conv + BN + ReLU"), (res, "conv + BN + residual + ReLU")):
            compare(name, lambda r=r: conv_bn(conv, bn, *xs, *tail, residual=r), pair(r), reps)
        conv_ms = statistics.median(medians([lambda: conv(*xs, *tail)], reps)[0] for _ in range(ROUNDS))
        say(f"   (the convolution alone, bf16 out: {conv_ms:.3f} ms)")


def section_layers(reps, dev):
    from pcs_amd.sparse import SubMConv3d, sparse_voxels
    from pcs_amd.sparse_norm import SparseBatchNorm
    from pcs_amd.voxel import Conv3d, Conv3dCat, voxelize
    from pcs_amd.voxel_unet import VoxelBatchNorm
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    B, G, occ, C = 4, 256, 0.02, 64
    clouds = jittered_clouds(5, B, grid=G, occupancy=occ, per_voxel=2)
    rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])
    sv = sparse_voxels(rb, voxelize(rb, G))
    V = sv.num_voxels
    x = torch.randn(V, C, device=dev).to(BF)
    res = torch.randn(V, C, device=dev).to(BF)
    conv, bn = SubMConv3d(C, C, bias=False).to(dev), _randomise(SparseBatchNorm(C, relu=True).to(dev), g)
    _layer(f"sparse SubMConv3d {C} -> {C} + SparseBatchNorm at {G}^3 x {B}, {occ:.0%} ({V} voxels, "
           f"{'pair lists' if sv.use_pairs() else 'tile gather'}; a [V, {C}] bf16 array is {2 * V * C / 1e6:.1f} MB)",
           conv, bn, [x], (sv,), res, reps)
    del x, res, sv, rb, clouds
    torch.cuda.empty_cache()
    B, G, C = 4, 64, 64
    x = torch.randn(B, G, G, G, C, device=dev).to(BF)
    res = torch.randn(B, G, G, G, C, device=dev).to(BF)
    conv, bn = Conv3d(C, C, bias=False).to(dev), _randomise(VoxelBatchNorm(C, relu=True).to(dev), g)
    _layer(f"dense Conv3d {C} -> {C} stencil + VoxelBatchNorm at {B} x {G}^3 (a [.., {C}] bf16 grid is "
           f"{2 * B * G ** 3 * C / 1e6:.1f} MB)", conv, bn, [x], (), res, reps)
    del x, res
    torch.cuda.empty_cache()
    B, G, C = 4, 128, 32
    xa = torch.randn(B, G, G, G, C, device=dev).to(BF)
    xb = torch.randn(B, G, G, G, C, device=dev).to(BF)
    res = torch.randn(B, G, G, G, C, device=dev).to(BF)
    conv, bn = Conv3dCat(C, C, C, bias=False).to(dev), _randomise(VoxelBatchNorm(C, relu=True).to(dev), g)
    _layer(f"dense Conv3dCat {C} + {C} -> {C} two-source stencil + VoxelBatchNorm at {B} x {G}^3 (a [.., {C}] bf16 grid "
           f"is {2 * B * G ** 3 * C / 1e6:.1f} MB)", conv, bn, [xa, xb], (), res, reps)


def section_model(reps, dev, sparse):
    from pcs_amd.sparse_norm import SparseBatchNorm
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    if sparse:
        from pcs_amd.sparse_unet import SparseUNetSegmentation as Model
        B, G, widths = 4, 256, (64, 128, 256)
        clouds = jittered_clouds(5, B, grid=G, occupancy=0.02, per_voxel=2)
        what = f"the {G}^3 x {B}, 2 % batch"
    else:
        from pcs_amd.voxel_unet import VoxelUNetSegmentation as Model
        B, G, widths = 4, 128, (32, 64, 128)
        clouds = synthetic_clouds(3, [0] * B, num_classes=2, grid=G, dense=True)
        what = f"a fully occupied {B} x {G}^3 batch"
    rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds])
    rb = rb._replace(points=rb.points.to(dev), labels=rb.labels.to(dev))
    model = Model(4, 2, widths, G).to(dev)
    for m in model.modules():
        if isinstance(m, SparseBatchNorm):
            _randomise(m, g)
    model.eval()
    say(f"-- {Model.__name__}(widths={widths}, grid={G}) inference on {what} ({rb.points.shape[0]} points): predict(rb) "
        f"against eval() + no_grad + model(rb, fused=True) + argmax (both rebuild the point <-> voxel maps every call); "
        f"median of {reps} calls, min .. max of {ROUNDS} medians")

    def existing():
        with torch.no_grad():
            return torch.argmax(model(rb, fused=True), 1)

    def folded():
        return model.predict(rb)

    la, lb = folded(), existing()
    say(f"   labels of the two forms agree on {float((la == lb).float().mean()):.6f} of the points "
        "(they differ by one bf16 rounding per layer)")
    del la, lb
    compare("whole model, one batch", folded, existing, reps)
    for name, fn in (("predict", folded), ("existing eval forward", existing)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        say(f"   {name:22s} max_memory_allocated {peak / 1e9:7.3f} GB = {base / 1e9:.3f} GB held before + {(peak - base) / 1e9:.3f} GB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("section", choices=["layers", "sparse", "dense"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "bench_unet_infer.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    if a.section == "layers":
        section_layers(max(10, a.reps), dev)
    else:
        section_model(max(3, a.reps), dev, a.section == "sparse")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
