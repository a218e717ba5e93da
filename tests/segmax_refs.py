"""Numpy fp64 statement of the segmented max (pcs_amd.segmax; csrc/segmax.hip and the max lift of
csrc/pointhead.hip), and the inputs the CPU and GPU tests of it share.

TEST INFRASTRUCTURE ONLY.  Build-defined, like the rest of the voxel vocabulary:

  segment_max     over j in [seg_off[m], seg_off[m + 1]) ascending, s = src[j] (src None: s = j), s < 0
                  skipped: the running pick of torch.max over a dim.  A later row replaces the pick only
                  when it is strictly greater or the first NaN, and the first present row always makes
                  one.  Y[m][c] = the picked value, arg[m][c] = the picked s; no present row: 0, -1
  argselect       dX[r][c] = dY[seg_of[r]][c] if seg_of[r] >= 0 and arg[seg_of[r]][c] == r else 0
  voxel_max       segment_max over PointVoxelMap.points_by_voxel()'s CSR, seg_of = own
  sparse_max_pool segment_max over src = child.reshape(-1), seg_off = 8 * arange(Vc + 1), seg_of = parent
  lift_max        z[j][c] = b[c] + sum_i W[c][i] P[order[j]][i] (point_head_refs._lift_z);
                  Y[v][c] = relu(z[j*][c]), j* the first j of the largest z of v's segment (0 without
                  points);  g[v][c] = z[j*][c] > 0 ? dV[v][c] : 0;  dW[c][i] = sum_v g[v][c] P[order[j*]][i];
                  db[c] = sum_v g[v][c]

The device recomputes z in fp32, so an element (voxel, channel) is *undecided* when another z of the
voxel lies within GATE_BAND * (|b| + sum_i |W_i p_i|) of the largest (the larger of the two entries'
sums), or the largest within that band of the gate at 0: point_head_refs' rule for the gate.  A
correct evaluation may then pick another point or gate the other way; lift_max_bwd reports the sum of
|dV| * 2 max_j |p_j| (dW) and of |dV| (db) over those elements, which widens the bound of dW and db.
"""
import numpy as np

import point_head_refs as ph

GATE_BAND = ph.GATE_BAND
UNDECIDED_CAP = 5e-4


def segment_max(X, src, seg_off):
    """pcs_rows_segmax: (Y float64 [M, C], arg int32 [M, C])."""
    X = np.asarray(X, np.float64)
    seg_off = np.asarray(seg_off, np.int64)
    M, C = len(seg_off) - 1, X.shape[1]
    best, arg = np.zeros((M, C)), np.full((M, C), -1, np.int32)
    length = np.diff(seg_off)
    for k in range(int(length.max()) if M else 0):
        seg = np.nonzero(length > k)[0]
        j = seg_off[seg] + k
        s = j.astype(np.int64) if src is None else np.asarray(src, np.int64)[j]
        seg, s = seg[s >= 0], s[s >= 0]
        v, cur, ca = X[s], best[seg], arg[seg]
        with np.errstate(invalid="ignore"):
            wins = (ca < 0) | (v > cur) | (np.isnan(v) & ~np.isnan(cur))
        best[seg] = np.where(wins, v, cur)
        arg[seg] = np.where(wins, s[:, None].astype(np.int32), ca)
    return best, arg


def argselect(dY, arg, seg_of, R):
    """pcs_rows_argselect: float64 [R, C]."""
    dY, seg_of = np.asarray(dY, np.float64), np.asarray(seg_of, np.int64)
    out = np.zeros((R, dY.shape[1]))
    ok = np.nonzero(seg_of >= 0)[0]
    m = seg_of[ok]
    out[ok] = np.where(np.asarray(arg)[m] == ok[:, None], dY[m], 0.0)
    return out


def voxel_max(P, own, V):
    """pcs_amd.segmax.voxel_max: (Y [V, C], arg [V, C])."""
    order, seg_off, _ = ph.points_by_voxel(own, V)
    return segment_max(P, order, seg_off)


def pool_segments(child):
    """(src int32 [8 Vc], seg_off int64 [Vc + 1]) of sparse_max_pool."""
    child = np.asarray(child, np.int32)
    return child.reshape(-1), 8 * np.arange(child.shape[0] + 1, dtype=np.int64)


def sparse_max_pool(X, child):
    """pcs_amd.segmax.sparse_max_pool: (Y [Vc, C], arg [Vc, C])."""
    return segment_max(X, *pool_segments(child))


def lift_max(P, Cin, W, b, order, seg_off):
    """pcs_point_lift_max: dict of Y float64 [V, C], zmax [V, C] (0 without points), entry int32 [V, C]
    (the picked CSR entry j*, -1 without points) and undecided bool [V, C]."""
    z, scale, _, vox = ph._lift_z(P, Cin, W, b, order, seg_off)
    V = len(seg_off) - 1
    zmax, entry = segment_max(z, None, seg_off)
    top = np.where(entry >= 0, np.take_along_axis(scale, np.maximum(entry, 0).astype(np.int64), 0) if len(scale) else 0.0, 0.0)
    near = z >= zmax[vox] - GATE_BAND * np.maximum(scale, top[vox])
    count = np.zeros((V, z.shape[1]))
    np.add.at(count, vox, near)
    undecided = (count >= 2) | ((entry >= 0) & (np.abs(zmax) <= GATE_BAND * top))
    return {"Y": np.maximum(zmax, 0.0), "zmax": zmax, "entry": entry, "undecided": undecided}


def lift_max_bwd(dV, P, Cin, W, b, order, seg_off):
    """pcs_point_lift_max_bwd: dict of dW [C, Cin], db [C], the sums of |term| (abs_dW, abs_db) and the
    widening over the undecided elements (amb_dW, amb_db)."""
    f = lift_max(P, Cin, W, b, order, seg_off)
    _, _, pts, vox = ph._lift_z(P, Cin, W, b, order, seg_off)
    dV = np.asarray(dV, np.float64)
    V, C = dV.shape
    g = np.where(f["zmax"] > 0, dV, 0.0)                          # (zmax is 0 without points)
    picked = pts[np.maximum(f["entry"], 0).astype(np.int64)] if len(pts) else np.zeros((V, C, Cin))   # [V, C, Cin]
    pmax = np.zeros((V, Cin))
    np.maximum.at(pmax, vox, np.abs(pts))
    amb = np.where(f["undecided"], np.abs(dV), 0.0)
    return {"dW": np.einsum("vc,vci->ci", g, picked), "db": g.sum(0),
            "abs_dW": np.einsum("vc,vci->ci", np.abs(g), np.abs(picked)), "abs_db": np.abs(g).sum(0),
            "amb_dW": 2.0 * amb.T @ pmax, "amb_db": amb.sum(0), "undecided": f["undecided"]}


def point_lift_max(points, W, b, own, V):
    """pcs_amd.segmax.point_lift_max: float64 [V, C]."""
    order, seg_off, _ = ph.points_by_voxel(own, V)
    return lift_max(points, np.shape(W)[1], W, b, order, seg_off)["Y"]


def point_lift_max_grad(dV, points, W, b, own, V):
    order, seg_off, _ = ph.points_by_voxel(own, V)
    return lift_max_bwd(dV, points, np.shape(W)[1], W, b, order, seg_off)


# ---- inputs shared by the CPU and the GPU tests
SEG_LENGTHS = [0, 1, 3, 4, 5, 37]            # around the kernel's SEG_UNROLL = 4
SEG_M = 45
NAN_SEG, NAN_COL = 7, 3                      # one NaN, in this column of one row of this segment
TIE_SEG, INF_SEG, GONE_SEG = 9, 11, 13       # exact ties; all -inf; every entry of src is -1


def segments(seed=0, M=SEG_M, shuffled=True):
    """(src int32 [n] or None, seg_off int64 [M + 1], seg_of int32 [R], R): M segments of the lengths
    above mixed over R source rows, each row in at most one segment; shuffled: src is a permutation
    with a share of -1 entries and one segment (GONE_SEG) whose entries are all -1, else src is None
    (the rows themselves)."""
    rng = np.random.default_rng(100 + seed)
    length = np.array([SEG_LENGTHS[i % len(SEG_LENGTHS)] for i in rng.permutation(M)], np.int64)
    for s, n in ((NAN_SEG, 5), (TIE_SEG, 37), (INF_SEG, 3), (GONE_SEG, 4)):
        length[s] = n
    seg_off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    n = int(seg_off[-1])
    seg = np.repeat(np.arange(M), length)
    if not shuffled:
        return None, seg_off, seg.astype(np.int32), n
    R = n + 9                                                     # rows no segment reads
    src = rng.permutation(R)[:n].astype(np.int32)
    drop = rng.random(n) < 0.1
    drop[seg_off[GONE_SEG]:seg_off[GONE_SEG + 1]] = True
    for s in (NAN_SEG, TIE_SEG, INF_SEG):
        drop[seg_off[s]:seg_off[s + 1]] = False
    src[drop] = -1
    seg_of = np.full(R, -1, np.int32)
    seg_of[src[~drop]] = seg[~drop]
    return src, seg_off, seg_of, R


def segment_rows(seed, R, C, src, seg_off):
    """bf16-exact float32 [R, C] with the single-column NaN, the ties and the all -inf segment."""
    x = ph.rows(seed, R, C)
    row = (lambda j: j) if src is None else (lambda j: int(src[j]))
    j0 = int(seg_off[TIE_SEG])
    for k in (3, 4, 20, 36):                                      # equal maxima at four places of the segment
        x[row(j0 + k)] = 9.0
    x[row(j0 + 20), 1] = 10.0                                     # ... and a column with a later strict maximum
    for j in range(int(seg_off[INF_SEG]), int(seg_off[INF_SEG + 1])):
        x[row(j)] = -np.inf
    x[row(int(seg_off[NAN_SEG]) + 2), NAN_COL] = np.nan
    return x


def clouds(grid, occupancy, per_voxel=3, seed=5, scenes=3):
    from pcs_amd.data import jittered_clouds
    return [(p.astype(np.float32), l.astype(np.int64)) for p, l in
            jittered_clouds(seed, scenes, grid=grid, occupancy=occupancy, per_voxel=per_voxel)]


def cpu_level(grid, occupancy, per_voxel=3):
    """(points [T, 4], own int32 [T], keys int64 [V]) of clouds(...) from tests/point_voxel_refs.py."""
    import point_voxel_refs as pv
    pts, _, off = ph.flat(clouds(grid, occupancy, per_voxel))
    keys = pv.level_keys(pts, off, grid, ph.LO, ph.HI)
    own, _, _ = pv.trilinear_index(pts, off, keys, grid, ph.LO, ph.HI)
    return pts, own, keys


# the two inputs of the fused lift's GPU test: (grid, occupancy, per_voxel)
LIFT_INPUTS = [(16, 0.3, 3), (16, 0.3, 6)]
LIFT_CIN = 4


def lift_max_params(C, seed=0):
    """(W [C, 4] ~ 0.5 N(0, 1), b [C] ~ 0.1 N(0, 1)) float32."""
    rng = np.random.default_rng(7000 + seed)
    return (0.5 * rng.standard_normal((C, LIFT_CIN))).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
