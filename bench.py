"""Benchmark: PointNetSegmentation training step (forward + weighted CE + backward + Adam)
on MI355X, points/s on a dense 128^3 grid, batch 4 scenes per GPU (BASELINE.json configs[1];
SURVEY.md §8(d) cfg2).  One process per GPU; for N>1 launch with torch.distributed.run.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dtype bf16|fp8|fp32] [--grid 128]
                    [--full] [--dump-outputs DIR]

--dtype fp8 is BASELINE.json configs[4] (cfg5): the bf16 step with the 1024-wide layer's
activation a5 and global_feat's GEMMs in e4m3 on MX-scaled MFMA.

Prints ONE JSON line (rank 0).  value = points processed by all ranks / max-over-ranks
wall time of K steps (bracketed by barrier + synchronize); ``ms_per_step`` is that wall time
over K.  A plain run does nothing else: it sets up, warms up, times the K steps and prints
the line (``roofline``, ``northstar_64x64`` and ``cpu_baseline`` are null).

``--full`` adds everything else the benchmark measures: ``roofline`` describes the dominant
kernel from HIP events recorded on its launch stream inside the timed region, two extra steps
after it give the per-kernel table (stderr) and ``northstar_64x64``, and ``cpu_baseline`` times
the pure-PyTorch CPU restatement of the reference step (and the numpy oracle) on the host
cores.  ``--no-kernel-timing`` / ``--no-cpu-baseline`` switch single legs of ``--full`` off.

``--dump-outputs DIR`` writes, after the timed steps, what the last timed step handed its
caller as float32 ``DIR/<name>.npy`` (rank 0): ``loss``, every parameter's gradient
(``grad.<param>``), the Adam-updated parameters (``param.<param>``) and the BatchNorm running
statistics (``buffer.<name>``), about 15 MB in all.  Inputs, initial weights and dropout
seeds are fixed by the arguments, so two builds can be compared array for array.

``--gpus N`` with N > 1 and no torch.distributed environment starts N ranks itself (a
torch.distributed.run child, one process per GPU, RCCL); under a launcher WORLD_SIZE must equal
N, and an RCCL run refuses to start with fewer than N visible GPUs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

import pcs_amd  # noqa: E402
from pcs_amd.data import class_weights_from_counts, label_counts, synthetic_batch  # noqa: E402
from pcs_amd.model import PointNetSegmentation  # noqa: E402
from pcs_amd.optim import FusedAdam  # noqa: E402
from pcs_amd.train import FusedTrainStep  # noqa: E402

PEAK = {"bf16": {"mfma": 2516.6, "hbm": 8000.0}, "fp32": {"mfma": 157.3, "hbm": 8000.0},
        "fp8": {"mfma": 5033.2, "hbm": 8000.0}}   # fp8: dense e4m3 (block-scaled MFMA), no sparsity


def act_bytes(dtype):
    """Bytes per stored activation element (fp8: the bf16 path outside the wide layer)."""
    return 4 if dtype == "fp32" else 2


def kernel_peak(tag, dtype):
    """MFMA / HBM peaks the kernel behind ``tag`` is priced against: under fp8 the
    global_feat kernels run e4m3 MFMA, everything else bf16."""
    if dtype == "fp8":
        return PEAK["fp8"] if tag.endswith(":global_feat") else PEAK["bf16"]
    return PEAK[dtype]
LAYER_DIMS = {"conv1": (4, 64), "conv2": (64, 64), "conv3": (64, 64), "conv4": (64, 128),
              "conv5": (128, 1024), "global_feat": (1024, 1024), "seg_conv1": (64, 512),
              "seg_conv2": (512, 256), "seg_conv3": (256, 128)}


# bench tag -> HIP kernel symbol (as summarised from rocprofv3 in profiles/pmc_<round>.json)
# (the template's bool is the fp8 form)
TAG_KERNEL = {
    "wgrad:global_feat": "gram_glds_kernel<{f}>",              # LDS-DMA Gram a5^T a5 (upper tiles)
    "fwd:global_feat": "gemm_glds_kernel<0, {f}>",             # LDS-DMA: BN stats + max-pool epilogue
    "dgrad:global_feat": "gemm_glds_kernel<1, {f}>",           # LDS-DMA: folded a5 H, ReLU mask
}
GRAM_TILE_FRACTION = 10.0 / 16.0   # upper 256-tiles of the symmetric 1024 x 1024 Gram


def lib_sha16():
    """First 16 hex digits of the SHA-256 of the HIP library this process runs (the build a
    PMC summary must describe for its counters to be quoted against this run)."""
    import hashlib
    path = os.path.join(REPO, "point-cloud-cnn-segmentation_amd", "csrc", "libpcs.so")
    try:
        with open(path, "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()[:16]
    except OSError:
        return None


def pmc_traffic(tag, dtype, workload, points):
    """HBM bytes per launch of the kernel behind ``tag``, from a committed PMC summary
    (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, tools/profile_round.sh) whose
    recorded workload, dtype, points per step AND libpcs.so hash match this run; None when no
    such profile exists (the number would describe a different launch or another build)."""
    import glob
    sym = TAG_KERNEL.get(tag)
    if sym is None:
        return None
    sym = sym.format(f="true" if dtype == "fp8" else "false")
    lib = lib_sha16()
    for path in sorted(glob.glob(os.path.join(REPO, "profiles", "pmc_*.json")), reverse=True):
        with open(path) as f:
            rec = json.load(f)
        meta = rec.get("meta") if isinstance(rec, dict) else None
        if not meta or (meta.get("workload"), meta.get("dtype"), meta.get("points_per_step"),
                        meta.get("lib_sha16")) != (workload, dtype, points, lib) or lib is None:
            continue
        ent = rec.get("kernels", {}).get(sym, {})
        if "hbm_bytes_per_launch" in ent:
            return {"bytes": ent["hbm_bytes_per_launch"], "source": os.path.relpath(path, REPO)}
    return None


def kernel_model(tag, M, dtype):
    """Algorithmic FLOPs and HBM bytes of one launch (SURVEY.md §8(d) accounting).  fp8:
    a5 (global_feat's input, conv5's stored output) is 1 byte, dz5 and the rest bf16."""
    kind, conv = tag.split(":", 1)
    if conv not in LAYER_DIMS or kind not in ("fwd", "dgrad", "wgrad", "dgrad+wgrad"):
        return None
    ab = act_bytes(dtype)
    a5b = 1 if dtype == "fp8" else ab
    cin, cout = LAYER_DIMS[conv]
    flops = 2.0 * M * cin * cout
    if kind == "dgrad+wgrad" and conv == "seg_conv1":   # folded: dz and y2 in, dA2 out (Y' not read)
        return 2 * flops, M * (cout + 2 * cin) * ab
    if kind == "dgrad+wgrad":   # fused: dZ, Y in once, Y_{l-1} (+ addend) in, dZ_{l-1} out
        extra = cin if conv == "conv3" else 0
        return 2 * flops, M * (2 * cout + 2 * cin + extra) * ab
    if kind == "wgrad" and conv == "global_feat":   # Gram of a5: upper tiles, reads a5 once
        return flops * GRAM_TILE_FRACTION, M * cin * a5b
    if conv == "global_feat" and kind == "fwd":     # reads a5; statistics + pool only, no store
        return flops, M * cin * a5b
    if conv == "global_feat" and kind == "dgrad":   # a5 (also the ReLU mask) in, dz5 out
        return flops, M * (cin * a5b + cout * ab)
    if conv == "conv5" and kind == "fwd":           # a4 in, a5 out
        return flops, M * (cin * ab + cout * a5b)
    if conv == "conv5" and kind == "dgrad":   # folded, one pass: dz5, y4 in, dz4 out (+ a4 H4 FLOPs)
        return flops + 2.0 * M * cin * cin, M * (cout + 2 * cin) * ab
    if conv == "conv5" and kind == "wgrad":   # R = dz5^T a4: dz5, y4 in
        return flops, M * (cout + cin) * ab
    if kind == "fwd":
        nbytes = M * (cin + cout) * ab
    elif kind == "dgrad":
        extra = 0 if conv == "global_feat" else cout      # pool path reads no dZ
        nbytes = M * (cout + extra + 2 * cin) * ab        # A (+dZ), Y_{l-1} in, dZ_{l-1} out
        if conv == "seg_conv1":
            nbytes = M * (2 * cout + cin) * ab
    else:  # wgrad
        extra = 0 if conv == "global_feat" else cout
        nbytes = M * (cout + extra + cin) * ab
    return flops, nbytes


def step_roofline(M, C, dtype, measured_ms):
    """t_roof = sum over layers of max(F_l / P_mfma, Bytes_l / 8 TB/s) for
    the whole fwd+bwd step (decomposed seg_conv1: local 64->512 GEMM; conv1 has no dgrad;
    every activation read or written once per pass).  fp8: global_feat at the e4m3 peak with
    a 1-byte input, conv5's output 1 byte."""
    layers = [(4, 64, 2), (64, 64, 3), (64, 64, 3), (64, 128, 3), (128, 1024, 3), (1024, 1024, 3),
              (64, 512, 3), (512, 256, 3), (256, 128, 3), (128, C, 3)]
    ab = act_bytes(dtype)
    t = 0.0
    for cin, cout, passes in layers:
        wide = (cin, cout) == (1024, 1024)
        peak = PEAK["fp8"] if dtype == "fp8" and wide else PEAK["bf16" if ab == 2 else "fp32"]
        f = 2.0 * M * cin * cout * passes
        ib = 1 if dtype == "fp8" and wide else ab
        ob = 1 if dtype == "fp8" and cout == 1024 and cin == 128 else ab
        b = 3.0 * M * (cin * ib + cout * ob)
        t += max(f / (peak["mfma"] * 1e12), b / (peak["hbm"] * 1e9))
    return {"t_roof_ms": round(t * 1e3, 3), "frac": round(t * 1e3 / measured_ms, 4),
            "model": "sum_l max(F_l/P_mfma, B_l/8TB/s), SURVEY 8(d)"}


def northstar_64(kernels, M, dtype):
    """HBM-only fraction of the 64->64 conv fwd+bwd (conv2: fwd, dgrad, wgrad)
    against t_HBM = 6 x 64 ch x M x bytes / 8 TB/s."""
    tags = ("fwd:conv2", "dgrad:conv2", "wgrad:conv2")
    if "dgrad+wgrad:conv2" in kernels:   # fused backward (csrc/fused_bwd.hip)
        tags = ("fwd:conv2", "dgrad+wgrad:conv2")
    if not all(t in kernels for t in tags):
        return None
    ms = sum(kernels[t][0] / kernels[t][1] for t in tags)
    t_hbm = 6 * 64 * M * act_bytes(dtype) / (PEAK["bf16"]["hbm"] * 1e9) * 1e3
    return {"layer": "conv2 (64->64) fwd+dgrad+wgrad", "ms": round(ms, 4), "t_hbm_ms": round(t_hbm, 4),
            "hbm_frac": round(t_hbm / ms, 4)}


def _cpu_threads():
    """(threads used, cores in this process's affinity mask, BLAS pool size)."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        omp = int(os.environ.get("OMP_NUM_THREADS", "0"))
    except ValueError:
        omp = 0
    threads = min(aff, omp) if omp > 0 else aff
    blas = None
    try:
        from threadpoolctl import threadpool_info
        blas = max([i.get("num_threads", 1) for i in threadpool_info() if i.get("user_api") == "blas"] or [0]) or None
    except Exception:  # pragma: no cover
        pass
    return threads, aff, blas


def cpu_baseline(max_seconds=10.0):
    """the pure-PyTorch CPU restatement of the reference step (oracle/torch_cpu.py,
    pinned to the reference goldens) in fp32, train mode, dropout on, fwd + weighted CE + bwd, on
    the reference's CPU-runnable case (B=4, N=4096, C=2), torch threads = the cores this process
    may use.  Also times the numpy oracle (``numpy`` field) for continuity with earlier rounds."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import pointnet_oracle as orc
    import torch_cpu as tc
    threads, aff, blas = _cpu_threads()
    B, N = 4, 4096
    sd = orc.init_params(2, 7)
    pts, lab, _ = synthetic_batch(1234, [N] * B, 2, grid=32)
    w = np.array([0.5, 1.5], np.float32)

    def timed(fn):
        fn()   # warm-up
        t0 = time.perf_counter()
        steps = 0
        while True:
            fn()
            steps += 1
            el = time.perf_counter() - t0
            if el >= max_seconds or steps >= 20:
                return steps, el

    prev = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        T = tc.to_tensors(sd)
        xt, yt, wt = torch.from_numpy(pts), torch.from_numpy(lab), torch.from_numpy(w)
        steps, el = timed(lambda: tc.train_step(T, xt, yt, wt))
    finally:
        torch.set_num_threads(prev)
    masks = orc.dropout_masks(3, B * N)
    nsteps, nel = timed(lambda: orc.train_step(sd, pts, lab, w, masks=masks, dtype=np.float32))
    note = ("torch threads = the affinity count" if threads == aff else
            f"torch threads capped at OMP_NUM_THREADS={threads}: the GPU box sets it to its CPU share "
            f"per GPU; the affinity mask lists all {aff} host cores, which the other GPUs' jobs share")
    return {"value": B * N * steps / el / 1e6, "unit": "M points/s", "cores": int(threads),
            "kind": "port", "affinity_cores": int(aff), "torch_threads": int(threads), "threads_note": note,
            "sample": f"pure-PyTorch CPU restatement of the reference step (oracle/torch_cpu.py: "
                      f"ATen conv1d / batch_norm / dropout / cross_entropy + autograd, fp32, train "
                      f"mode, dropout on), B=4 x N=4096 (32^3 lattice), C=2, {steps} steps in "
                      f"{el:.1f}s after 1 warm-up, {threads} torch threads",
            "numpy": {"value": B * N * nsteps / nel / 1e6, "unit": "M points/s",
                      "blas_threads": blas,
                      "sample": f"numpy fp32 oracle fwd+CE+bwd, same batch, {nsteps} steps in {nel:.1f}s"}}


def shared_class_weights(label_arrays, num_classes, world):
    """One class-weight vector for every rank (P:168-189, P:216: the reference builds a single
    weight tensor from the labels it scans): the per-class counts of this rank's scenes are
    summed over the process group, so every rank derives the weights of the global batch (the
    concatenation of all ranks' scenes), not of its own shard.  ``label_arrays`` are the scenes'
    own labels: the reference scans dataset events (P:148-166), which never hold collate pads, so
    pad labels (-1) are skipped here and must not reach ``class_weights`` either (its Counter
    would count them)."""
    counts = label_counts(label_arrays, num_classes)
    if world > 1:
        t = torch.from_numpy(counts)
        if dist.get_backend() == "nccl":
            t = t.cuda()
        dist.all_reduce(t)
        counts = t.cpu().numpy()
    return class_weights_from_counts(counts, num_classes)


def dump_outputs(out_dir, model, loss):
    """``--dump-outputs``: what the last timed step handed its caller, as float32
    ``<out_dir>/<name>.npy``: the loss, p.grad and the Adam-updated p of every parameter, and the
    BatchNorm running statistics (about 15 MB at C=2; everything is written whole)."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss": loss.detach().reshape(1)}
    for n, p in model.named_parameters():
        arrays[f"grad.{n}"] = p.grad
        arrays[f"param.{n}"] = p.detach()
    for n, b in model.named_buffers():
        if n.endswith(("running_mean", "running_var")):
            arrays[f"buffer.{n}"] = b
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.to(torch.float32).cpu().numpy())


def launch_ranks(n):
    """``--gpus N`` (N > 1) without a torch.distributed environment: start N ranks, one process
    per GPU, with torch.distributed.run as a CHILD process and return its exit code.  This
    process never initialises the GPU (device_count() does not, on this image) and never execs."""
    import socket
    import subprocess
    backend = os.environ.get("PCS_DIST_BACKEND", "nccl")
    have = torch.cuda.device_count()
    if backend == "nccl" and have < n:
        print(f"bench.py: --gpus {n} needs {n} visible GPUs for one RCCL rank per GPU, found {have}",
              file=sys.stderr)
        return 2
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8", "fp32"])
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: per-kernel HIP events "
                         "(roofline, northstar_64x64, the stderr table) and the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the last step's loss, gradients, updated "
                         "parameters and BatchNorm running statistics as float32 DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-kernel-timing", action="store_true", help="with --full: record no HIP events")
    ap.add_argument("--draw-at-start", action="store_true",
                    help="draw the dropout bits at the start of the forward instead of beside the Gram of a5 (A/B)")
    ap.add_argument("--no-fused-seg12", action="store_true",
                    help="A/B: seg_conv1 and seg_conv2 forward as two passes instead of pcs_fwd_seg12")
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "cfg3"],
                    help="cfg2: dense G^3 grid (the bench line); cfg3: occupied-only ragged "
                         "clouds on a 256^3 lattice (~2%% occupancy), CSR batch resident in HBM, "
                         "padded on the device inside every timed step")
    ap.add_argument("--occupancy", type=float, default=0.02)
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a "
              f"{world}-rank run as {args.gpus} GPUs", file=sys.stderr)
        sys.exit(2)
    # RCCL ("nccl") is the data-parallel backend; PCS_DIST_BACKEND=gloo rehearses the N>1
    # code path with several ranks sharing the GPUs a box has (device = local rank mod count)
    backend = os.environ.get("PCS_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "gloo":
        local %= max(1, ndev)
    elif local >= ndev:
        print(f"bench.py: rank {rank} (local {local}) has no GPU of its own: {ndev} visible",
              file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    B, G, C = args.scenes, args.grid, args.classes
    rb = None
    if args.workload == "cfg3":
        # occupied-only ragged scenes: CSR in HBM, device-side collate
        # (pcs_pad_scatter) to the DP-global max length inside the step, like collate_fn + H2D
        from pcs_amd.data import occupied_clouds, ragged_collate
        from pcs_amd.loader import global_max_points, pad_on_device
        G = 256 if args.grid == 128 else args.grid
        clouds = occupied_clouds(1234 + rank, B, grid=G, occupancy=args.occupancy, num_classes=C)
        w = shared_class_weights([l for _, l in clouds], C, world)
        rb = ragged_collate([(torch.from_numpy(p), torch.from_numpy(l)) for p, l in clouds], torch.int32)
        N = global_max_points(rb.max_points, None, dev)
        real_points = int(rb.offsets[-1])
        rb = type(rb)(*(t.to(dev) for t in rb))
        del clouds
    else:
        N = G ** 3
        pts, lab, _ = synthetic_batch(1234 + rank, [N] * B, C, grid=G, dense=True)
        w = shared_class_weights([lab[b][lab[b] >= 0] for b in range(B)], C, world)
        x = torch.from_numpy(pts).to(dev)
        y = torch.from_numpy(lab).to(dev)
        real_points = B * N
        del pts, lab

    def run_step():
        if rb is not None:
            xs, ys, _ = pad_on_device(rb, dev, scene_rows=N)
            return step(xs, ys)
        return step(x, y)

    torch.manual_seed(0)
    model = PointNetSegmentation(C, compute_dtype=args.dtype).to(dev)
    if args.draw_at_start:
        model._engine().draw_beside_gram = False
    if args.no_fused_seg12:
        model._engine().fused_seg12 = False
    if world > 1:   # identical initial weights on every rank (DataParallel replicates them)
        for p in model.parameters():
            dist.broadcast(p.data, 0)
    opt = FusedAdam(model, lr=1e-3, weight_decay=1e-4)
    step = FusedTrainStep(model, opt, class_weight=w)

    for i in range(args.warmup):
        loss = run_step()
    torch.cuda.synchronize()
    # --full: inside the timed region only the dominant-kernel candidates (the global_feat GEMMs
    # and Gram) are bracketed by HIP events, so the measurement barely perturbs the step; the
    # full per-kernel breakdown comes from two extra steps after it
    timing = {} if args.full and not args.no_kernel_timing else None
    step.timing = timing
    step.timing_tags = set(TAG_KERNEL)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = run_step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    el = time.perf_counter() - t0
    step.timing = None
    if args.dump_outputs and rank == 0:   # before --full's extra steps move the weights on
        dump_outputs(args.dump_outputs, model, loss)
    breakdown = {}
    if timing is not None:
        step.timing, step.timing_tags = breakdown, None
        for i in range(2):
            run_step()
        torch.cuda.synchronize()
        step.timing = None
    if world > 1:
        t = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    loss_v = float(loss.item())

    M = B * N
    devices = [local]
    if world > 1:
        t = torch.tensor([real_points], device=dev, dtype=torch.int64)
        dist.all_reduce(t)
        real_points = int(t.item())
        d = torch.zeros(world, dtype=torch.int64, device=dev)
        d[rank] = local
        dist.all_reduce(d)
        devices = [int(v) for v in d.tolist()]
        world = dist.get_world_size()
    total_points = real_points * args.steps
    roof = None
    kernels, full = {}, {}
    if timing:
        for tag, evs in timing.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            kernels[tag] = (sum(ms), len(ms))
        for tag, evs in breakdown.items():
            ms = [a.elapsed_time(b) for a, b in evs]
            full[tag] = (sum(ms), len(ms))
        dom = max(kernels, key=lambda k: kernels[k][0])
        tot, cnt = kernels[dom]
        avg_s = tot / cnt / 1e3
        mdl = kernel_model(dom, M, args.dtype)
        if mdl:
            flops, nbytes = mdl
            ai = flops / nbytes
            tr = pmc_traffic(dom, args.dtype, args.workload, M)
            pk = kernel_peak(dom, args.dtype)
            ridge = pk["mfma"] * 1e12 / (pk["hbm"] * 1e9)
            if ai >= ridge:
                ach = flops / avg_s / 1e12
                roof = {"bound": "mfma", "kernel": dom, "achieved": round(ach, 2),
                        "peak": pk["mfma"], "unit": "TFLOP/s",
                        "frac": round(ach / pk["mfma"], 4),
                        "traffic": tr and tr["bytes"], "traffic_source": tr and tr["source"],
                        "algorithmic_bytes": nbytes,
                        "algorithmic_flops": flops, "avg_ms": round(avg_s * 1e3, 4)}
            else:
                ach = nbytes / avg_s / 1e9
                roof = {"bound": "hbm", "kernel": dom, "achieved": round(ach, 1),
                        "peak": pk["hbm"], "unit": "GB/s",
                        "frac": round(ach / pk["hbm"], 4),
                        "traffic": tr and tr["bytes"], "traffic_source": tr and tr["source"],
                        "algorithmic_bytes": nbytes, "avg_ms": round(avg_s * 1e3, 4)}
        if rank == 0:
            step_ms = el / args.steps * 1e3
            print(f"# per-kernel (avg ms over 2 steps after the timed region, share of the {step_ms:.2f} ms "
                  f"step):", file=sys.stderr)
            for tag, (tot, cnt) in sorted(full.items(), key=lambda kv: -kv[1][0]):
                mdl = kernel_model(tag, M, args.dtype)
                extra = ""
                if mdl:
                    a = tot / cnt / 1e3
                    extra = f"  {mdl[0] / a / 1e12:8.1f} TF/s  {mdl[1] / a / 1e9:8.1f} GB/s"
                print(f"#  {tag:22s} {tot / cnt:9.3f} ms  {100 * tot / cnt / step_ms:5.1f}%{extra}",
                      file=sys.stderr)

    cpu = None
    if rank == 0 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline()

    if rank == 0:
        rec = {
            "metric": "M voxels/sec fwd+bwd, 128^3 grid batch=4 (points/s of the PointNet "
                      "training step: forward + weighted CE + backward + Adam)",
            "value": round(total_points / el / 1e6, 3),
            "unit": "M points/s",
            "n_gpus": world, "world_size": world, "rank_devices": devices,
            "dist_backend": backend if world > 1 else None,
            "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(el / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "fp8 e4m3 (global_feat, a5) + bf16" if args.dtype == "fp8" else args.dtype,
            "data": ("synthetic (dense voxel-centre clouds, seeded)" if rb is None else
                     "synthetic (occupied-only voxel-centre clouds, ragged, seeded)"),
            "config": ({"workload": ("cfg5: " if args.dtype == "fp8" else "") +
                                    f"PointNetSegmentation train step, {B} scenes x {G}^3 points "
                                    f"per GPU, C={C}" + (", a5 + global_feat in fp8 e4m3 (MX-scaled "
                                                         "MFMA)" if args.dtype == "fp8" else ""),
                        "global_batch": B * world,
                        "points_per_scene": N, "parallelism": f"dp{world}"} if rb is None else
                       {"workload": f"cfg3: PointNetSegmentation train step, {B} occupied-only "
                                    f"ragged scenes per GPU on a {G}^3 lattice ({args.occupancy:g} "
                                    f"occupancy), device-side collate in the step, C={C}",
                        "global_batch": B * world, "padded_points_per_scene": N,
                        "real_points_per_step": real_points, "parallelism": f"dp{world}"}),
            "loss": round(loss_v, 6),
            "roofline": roof,
            "step_roofline": step_roofline(M, C, args.dtype, el / args.steps * 1e3),
            "northstar_64x64": northstar_64(full, M, args.dtype) if kernels else None,
            "cpu_baseline": cpu,
            "lib_sha16": lib_sha16(),
        }
        print(json.dumps(rec))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
