"""numpy restatements of the coarse index and of the two k = 2, s = 2 sparse convolutions, from
their descriptions in include/pcs.h (not a test module).  tests/test_sparse_stride_refs.py proves
them against torch's dense conv3d / conv_transpose3d in fp64 on the CPU; the GPU tests
(test_gpu_sparse_stride.py) compare the kernels and pcs_amd.sparse.coarsen with them.

Build-defined, like the rest of the voxel vocabulary: the reference has no voxel grid.  Plain
dict lookups and np.unique, no hashing scheme restated.
"""
import numpy as np


def decode(keys, G):
    k = np.asarray(keys, dtype=np.uint64).astype(np.int64)
    G3 = G * G * G
    scene, loc = k // G3, k % G3
    return scene, loc // (G * G), (loc // G) % G, loc % G


def parent_keys(keys, G):
    """(parent_key int64 [Vf], tap int32 [Vf]) of the fine keys on an even grid G."""
    assert G % 2 == 0
    Gc = G // 2
    s, ix, iy, iz = decode(keys, G)
    pk = s * Gc ** 3 + ((ix >> 1) * Gc + (iy >> 1)) * Gc + (iz >> 1)
    tap = ((ix & 1) * 2 + (iy & 1)) * 2 + (iz & 1)
    return pk.astype(np.int64), tap.astype(np.int32)


def coarse_maps(keys, G):
    """coarse_keys (ascending, unique), tap [Vf], child [Vc, 8], parent [Vf], up [Vf, 8]."""
    pk, tap = parent_keys(keys, G)
    ckeys = np.unique(pk)
    row = {int(k): i for i, k in enumerate(ckeys)}
    parent = np.array([row[int(k)] for k in pk], dtype=np.int32).reshape(-1)
    child = np.full((len(ckeys), 8), -1, dtype=np.int32)
    up = np.full((len(pk), 8), -1, dtype=np.int32)
    for f in range(len(pk)):
        assert child[parent[f], tap[f]] == -1      # one fine voxel per (cell, corner)
        child[parent[f], tap[f]] = f
        up[f, tap[f]] = parent[f]
    return ckeys, tap, child, parent, up


def down_conv(x, w, b, child):
    """Y_c[m] = b + sum_t W[:, :, t] X[child[m, t]] in fp64; x [Vf, Cin], w [Cout, Cin, 2, 2, 2]."""
    x = np.asarray(x, np.float64)
    wt = np.asarray(w, np.float64).reshape(w.shape[0], w.shape[1], 8)
    y = np.zeros((child.shape[0], w.shape[0]), np.float64) + (0 if b is None else np.asarray(b, np.float64))
    for t in range(8):
        rows = child[:, t]
        ok = rows >= 0
        y[ok] += x[rows[ok]] @ wt[:, :, t].T
    return y


def up_conv(x, w, b, parent, tap):
    """Y_f[f] = b + U[:, :, tap[f]]^T X_c[parent[f]] in fp64; x [Vc, Cin], w [Cin, Cout, 2, 2, 2]
    (the ConvTranspose3d layout)."""
    x = np.asarray(x, np.float64)
    wt = np.asarray(w, np.float64).reshape(w.shape[0], w.shape[1], 8)
    y = np.zeros((len(parent), w.shape[1]), np.float64) + (0 if b is None else np.asarray(b, np.float64))
    for t in range(8):
        ok = tap == t
        y[ok] += x[parent[ok]] @ wt[:, :, t]
    return y
