"""The numpy restatements of tests/sparse_stride_refs.py against torch in fp64 on the CPU: the two
k = 2, s = 2 convolutions on the coarse maps equal F.conv3d(stride=2) / F.conv_transpose3d(stride=2)
on the zero-filled dense grid, read at the represented sites; and the invariants of the maps."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_stride_refs as sr

import pcs_amd.sparse  # noqa: F401  (the layers these restate: coarsen, sparse_conv3d_down, ..._up)
from pcs_amd.sparse import K2_TAPS

CASES = [(8, 0.4, 2), (12, 0.1, 3), (16, 0.03, 2)]


def _keys(seed, G, occ, B):
    rng = np.random.default_rng(seed)
    occd = rng.random((B, G, G, G)) < occ
    occd[0, G - 1, G - 1, G - 1] = occd[1, 0, 0, 0] = True    # neighbouring keys of two scenes
    return np.nonzero(occd.reshape(-1))[0].astype(np.int64)


@pytest.mark.parametrize("G,occ,B", CASES)
def test_map_invariants(G, occ, B):
    keys = _keys(G, G, occ, B)
    ckeys, tap, child, parent, up = sr.coarse_maps(keys, G)
    assert K2_TAPS == 8 and child.shape == (len(ckeys), 8) and up.shape == (len(keys), 8)
    f = np.arange(len(keys))
    assert np.array_equal(child[parent, tap], f)
    assert ((child >= 0).sum(1) >= 1).all()
    assert int((child >= 0).sum()) == len(keys)
    assert (np.diff(ckeys) > 0).all()
    assert np.array_equal(up[f, tap], parent) and int((up >= 0).sum()) == len(keys)
    # the parent is the cell the fine voxel lies in, the tap its corner
    s, ix, iy, iz = sr.decode(keys, G)
    cs, cx, cy, cz = sr.decode(ckeys[parent], G // 2)
    assert np.array_equal(cs, s)
    assert np.array_equal(2 * cx + (tap >> 2), ix)
    assert np.array_equal(2 * cy + ((tap >> 1) & 1), iy)
    assert np.array_equal(2 * cz + (tap & 1), iz)
    assert ckeys.max() < B * (G // 2) ** 3


@pytest.mark.parametrize("G,occ,B", CASES)
def test_convolutions_equal_torch_dense(G, occ, B):
    keys = _keys(100 + G, G, occ, B)
    ckeys, tap, child, parent, up = sr.coarse_maps(keys, G)
    s, ix, iy, iz = sr.decode(keys, G)
    cs, cx, cy, cz = sr.decode(ckeys, G // 2)
    g = torch.Generator().manual_seed(G)
    cin, cout = 5, 7
    rel = lambda a, r: float(np.abs(a - r).max() / np.abs(r).max())  # noqa: E731
    # down
    x = torch.randn(len(keys), cin, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 2, 2, 2, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    xd = torch.zeros(B, cin, G, G, G, dtype=torch.float64)
    xd[s, :, ix, iy, iz] = x
    ref = F.conv3d(xd, w, b, stride=2)[cs, :, cx, cy, cz].numpy()
    assert rel(sr.down_conv(x.numpy(), w.numpy(), b.numpy(), child), ref) < 1e-12
    # up
    xc = torch.randn(len(ckeys), cin, generator=g, dtype=torch.float64)
    u = torch.randn(cin, cout, 2, 2, 2, generator=g, dtype=torch.float64)
    xcd = torch.zeros(B, cin, G // 2, G // 2, G // 2, dtype=torch.float64)
    xcd[cs, :, cx, cy, cz] = xc
    ref = F.conv_transpose3d(xcd, u, b, stride=2)[s, :, ix, iy, iz].numpy()
    assert rel(sr.up_conv(xc.numpy(), u.numpy(), b.numpy(), parent, tap), ref) < 1e-12
