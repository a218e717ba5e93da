"""The forward pcs_gemm (BN+ReLU prologue, store) at the cfg2 global_feat shape, for rocprofv3
counter passes:
    python tools/prof_big.py [reps]"""
import ctypes as ct
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pcs_amd._lib as L  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    B, N, K, Nc = 4, 128 ** 3, 1024, 1024
    M = B * N
    dev = torch.device("cuda")
    lib = L.load()
    A = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
    W = (torch.randn(Nc, K, device=dev) * 0.03).to(torch.bfloat16)
    C = torch.empty(M, Nc, device=dev, dtype=torch.bfloat16)
    s, t = torch.rand(K, device=dev) + 0.5, torch.randn(K, device=dev) * 0.1
    a = L.GemmArgs(num_scenes=B, scene_rows=N, K=K, Ncols=Nc, dtype=L.BF16, prologue=L.PRO_BNRELU,
                   epilogue=L.EPI_FWD, chunks_per_scene=0)
    lib.pcs_gemm_geometry(ct.byref(a))
    a.A, a.W, a.C = A.data_ptr(), W.data_ptr(), C.data_ptr()
    a.pa, a.pb = L.ptr(s), L.ptr(t)
    for _ in range(reps):
        L.call("pcs_gemm", ct.byref(a), L.stream_ptr())
    torch.cuda.synchronize()
    print("done fwd", reps)


if __name__ == "__main__":
    main()
