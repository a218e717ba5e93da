"""Numpy fp64 statement of the fused point lift and point head (pcs_amd.pointhead,
csrc/pointhead.hip), and the inputs the CPU and GPU tests of it share.

TEST INFRASTRUCTURE ONLY.  Build-defined, like the rest of the voxel vocabulary.  The maps (a
PointVoxelMap's arrays, or tests/point_voxel_refs.py's) are passed in as numpy arrays:

  lift     z[j][c] = b[c] + sum_{i < Cin} W[c][i] P[order[j]][i];
           Y[v][c] = inv_count[v] * sum_{j in seg v} relu(z[j][c])
           g[j][c] = z[j][c] > 0 ? dV[v][c] inv_count[v] : 0;  dW[c][i] = sum g P_i;  db[c] = sum g
  project  Z[v][k] = sum_c X[v][c] W[k][c]
  logits   l[p][k] = b[k] + sum_{j < 8} weight[p][j] Z[corner[p][j]][k] (corner -1 skipped); for
           y = labels[p] in [0, K): nll = logsumexp(l) - l[y], loss = inv_wsum sum cw[y] nll,
           dlogits = cw[y] inv_wsum (softmax(l) - onehot(y)), db = sum_p dlogits; other labels: nothing
  bwd      dZ[v][k] = g sum_{j in seg v} pair_weight[j] dlogits[pair_point[j]][k];
           dX = dZ W;  dW = dZ^T X

The gate z > 0 of the lift's backward is recomputed on the device in fp32.  An element with
|z| <= GATE_BAND * (|b| + sum_i |W_i p_i|) may gate either way (the fp32 evaluation error of a 9-term
fma chain is below 6e-7 of that sum); lift_bwd reports the sum of |term| over those elements, which
widens the bound of dW and db.
"""
import numpy as np

import point_voxel_refs as pv

GATE_BAND = 1e-5
LO, HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


# ---- the CSRs of a map (pcs_amd.pointvoxel.PointVoxelMap.points_by_voxel / pairs_by_voxel)
def _csr(rows, n):
    key = np.where(rows < 0, n, rows).astype(np.int64)
    order = np.argsort(key, kind="stable")
    return order.astype(np.int32), np.searchsorted(key[order], np.arange(n + 1)).astype(np.int64)


def points_by_voxel(own, V):
    """(order int32 [T], seg_off int64 [V + 1], inv_count float64 [V])."""
    order, seg_off = _csr(np.asarray(own), V)
    cnt = (seg_off[1:] - seg_off[:-1]).astype(np.float64)
    return order, seg_off, np.where(cnt > 0, 1.0 / np.maximum(cnt, 1.0), 0.0)


def pairs_by_voxel(corner, weight, V):
    """(pair_point int32 [8 T], pair_weight float64 [8 T], seg_off int64 [V + 1])."""
    order, seg_off = _csr(np.asarray(corner).reshape(-1), V)
    return (order // 8).astype(np.int32), np.asarray(weight, np.float64).reshape(-1)[order], seg_off


def _segment_of(seg_off, n):
    """Row of each of the first seg_off[-1] entries of a CSR."""
    return np.repeat(np.arange(len(seg_off) - 1), np.diff(seg_off))


# ---- the five entry points
def _lift_z(P, Cin, W, b, order, seg_off):
    """(z float64 [n, C], scale |b| + sum |W_i p_i| [n, C], pts [n, Cin], voxel [n]) of the n = seg_off[-1]
    (voxel, point) entries in CSR order."""
    n = int(seg_off[-1])
    ids = np.asarray(order[:n], np.int64)
    assert (ids >= 0).all()
    pts = np.asarray(P, np.float64)[ids][:, :Cin]
    W = np.asarray(W, np.float64)
    bb = np.zeros(W.shape[0]) if b is None else np.asarray(b, np.float64)
    z = pts @ W.T + bb
    scale = np.abs(pts) @ np.abs(W).T + np.abs(bb)
    return z, scale, pts, _segment_of(seg_off, n)


def lift_mean(P, Cin, W, b, order, seg_off, inv_count):
    """pcs_point_lift_mean: float64 [V, C]."""
    z, _, _, vox = _lift_z(P, Cin, W, b, order, seg_off)
    V = len(seg_off) - 1
    out = np.zeros((V, np.shape(W)[0]))
    np.add.at(out, vox, np.maximum(z, 0.0))
    return out * np.asarray(inv_count, np.float64)[:, None]


def gate_ambiguous(P, Cin, W, b, order, seg_off):
    """bool [n, C]: the elements whose gate a correct fp32 evaluation may take either way."""
    z, scale, _, _ = _lift_z(P, Cin, W, b, order, seg_off)
    return np.abs(z) <= GATE_BAND * scale


def lift_mean_bwd(dV, P, Cin, W, b, order, seg_off, inv_count):
    """pcs_point_lift_mean_bwd: dict of dW [C, Cin], db [C], the sums of |term| (abs_dW, abs_db) and
    the sums of |dV inv_count P_i| over the ambiguous-gate elements (amb_dW, amb_db)."""
    z, scale, pts, vox = _lift_z(P, Cin, W, b, order, seg_off)
    up = (np.asarray(dV, np.float64) * np.asarray(inv_count, np.float64)[:, None])[vox]     # [n, C]
    g = np.where(z > 0, up, 0.0)
    amb = np.where(np.abs(z) <= GATE_BAND * scale, np.abs(up), 0.0)
    return {"dW": g.T @ pts, "db": g.sum(0), "abs_dW": np.abs(g).T @ np.abs(pts), "abs_db": np.abs(g).sum(0),
            "amb_dW": amb.T @ np.abs(pts), "amb_db": amb.sum(0)}


def head_project(X, W):
    """pcs_point_head_project: float64 [V, K]."""
    return np.asarray(X, np.float64) @ np.asarray(W, np.float64).T


def head_logits(Z, corner, weight, bias, labels=None, class_weight=None):
    """pcs_point_head_logits with inv_wsum = 1 / the sum of class_weight[label] over the valid labels:
    dict of logits [T, K] and, with labels, loss, abs_loss (the sum of |term|), dlogits [T, K], db [K],
    abs_db, valid [T]."""
    Z = np.asarray(Z, np.float64)
    K = Z.shape[1]
    l = pv.devoxelize(Z, corner, weight) if Z.shape[0] else np.zeros((len(corner), K))
    if bias is not None:
        l = l + np.asarray(bias, np.float64)
    out = {"logits": l}
    if labels is None:
        return out
    y = np.asarray(labels, np.int64)
    valid = (y >= 0) & (y < K)
    cw = np.ones(K) if class_weight is None else np.asarray(class_weight, np.float64)
    yc = np.where(valid, y, 0)
    cwy = np.where(valid, cw[yc], 0.0)
    wsum = cwy.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.float64(1.0) / wsum
        m = l.max(axis=1, keepdims=True)
        ex = np.exp(l - m)
        se = ex.sum(axis=1, keepdims=True)
        nll = (np.log(se) + m)[:, 0] - l[np.arange(len(l)), yc]
        terms = cwy * nll
        onehot = np.zeros_like(l)
        onehot[np.arange(len(l)), yc] = 1.0
        dl = np.where(valid[:, None], (cwy * inv)[:, None] * (ex / se - onehot), 0.0)
        out.update(loss=inv * terms.sum(), abs_loss=inv * np.abs(terms).sum(), dlogits=dl, db=dl.sum(0),
                   abs_db=np.abs(dl).sum(0), valid=valid)
    return out


def head_bwd(dlogits, pair_point, pair_weight, seg_off, X, W, g=1.0):
    """pcs_point_head_bwd: dict of dZ [V, K], dX [V, C], dW [K, C] and abs_dW (the sum of |term|)."""
    dl = np.asarray(dlogits, np.float64)
    V, n = len(seg_off) - 1, int(seg_off[-1])
    dZ = np.zeros((V, dl.shape[1]))
    np.add.at(dZ, _segment_of(seg_off, n), np.asarray(pair_weight, np.float64)[:n, None] * dl[np.asarray(pair_point[:n], np.int64)])
    dZ *= g
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    return {"dZ": dZ, "dX": dZ @ W, "dW": dZ.T @ X, "abs_dW": np.abs(dZ).T @ np.abs(X)}


# ---- the three Python functions
def point_lift_mean(points, W, b, own, V):
    """pcs_amd.pointhead.point_lift_mean: float64 [V, C]."""
    order, seg_off, inv = points_by_voxel(own, V)
    return lift_mean(points, np.shape(W)[1], W, b, order, seg_off, inv)


def point_lift_mean_grad(dV, points, W, b, own, V):
    order, seg_off, inv = points_by_voxel(own, V)
    return lift_mean_bwd(dV, points, np.shape(W)[1], W, b, order, seg_off, inv)


def point_head(X, corner, weight, W, b):
    """pcs_amd.pointhead.point_head: float64 logits [T, K]."""
    return head_logits(head_project(X, W), corner, weight, b)["logits"]


def point_head_grad(dlogits, X, corner, weight, W):
    """Gradients of point_head for an upstream dlogits: head_bwd's dict plus db, abs_db."""
    out = head_bwd(dlogits, *pairs_by_voxel(corner, weight, np.shape(X)[0]), X, W)
    dl = np.asarray(dlogits, np.float64)
    out.update(db=dl.sum(0), abs_db=np.abs(dl).sum(0))
    return out


def point_head_loss(X, corner, weight, W, b, labels, class_weight=None, upstream=1.0):
    """pcs_amd.pointhead.point_head_loss and its gradients for an upstream gradient of the loss: a
    dict of loss, abs_loss, logits, dlogits, dX, dW, abs_dW, db, abs_db."""
    out = head_logits(head_project(X, W), corner, weight, b, labels, class_weight)
    out.update(head_bwd(out["dlogits"], *pairs_by_voxel(corner, weight, np.shape(X)[0]), X, W, g=upstream))
    out["db"], out["abs_db"] = out["db"] * upstream, out["abs_db"] * abs(upstream)
    return out


# ---- inputs shared by the CPU and the GPU tests
def bf16_exact(a):
    """float32 values rounded to bf16 (round to nearest even), as float32: exact in every dtype."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _jittered(seed, scenes, grid, occupancy, edges):
    from pcs_amd.data import jittered_clouds
    out = []
    for p, l in jittered_clouds(seed, scenes, grid=grid, occupancy=occupancy, per_voxel=3):
        if edges:
            e = pv.edge_points(grid)
            p, l = np.concatenate([p, e]), np.concatenate([l, np.zeros(len(e), np.int64)])
        out.append((p.astype(np.float32), l.astype(np.int64)))
    return out


def _crowded_cloud(grid=8, seed=3, crowd=40):
    """One scene: one cell holding `crowd` points beside a handful of ordinary ones."""
    rng = np.random.default_rng(seed)
    h = 2.0 / grid
    cells = [(3, 3, 3)] * crowd + [(3, 3, 4), (3, 4, 3), (2, 3, 3), (6, 1, 5), (6, 1, 5), (0, 7, 2), (5, 5, 5)]
    xyz = -1.0 + (np.asarray(cells, np.float64) + rng.uniform(0.05, 0.95, size=(len(cells), 3))) * h
    p = np.zeros((len(cells), 4), np.float32)
    p[:, :3] = rng.permutation(xyz)
    p[:, 3] = rng.exponential(size=len(p))
    return [(p, rng.integers(-1, 2, size=len(p)).astype(np.int64))]


# name -> (grid, the clouds that make the level, the clouds whose points are mapped into it)
def case_clouds(name):
    """(grid, level clouds, query clouds) of a test map; query is level for A, B and D."""
    if name == "A":      # points outside the box, missing corners, renormalised weights
        c = _jittered(31, 3, 8, 0.4, True)
        return 8, c, c
    if name == "B":      # ~2.4 k voxels: several row blocks, V no multiple of the rows per block
        c = _jittered(32, 2, 16, 0.3, False)
        return 16, c, c
    if name == "C":      # A's level queried with other clouds: own = -1, points without a corner, empty voxels
        return 8, _jittered(31, 3, 8, 0.4, True), _jittered(57, 3, 8, 0.25, True)
    if name == "D":      # a segment much longer than the unroll
        c = _crowded_cloud()
        return 8, c, c
    raise KeyError(name)


def flat(clouds):
    """(points float32 [T, 4], labels int64 [T], offsets int64 [B + 1])."""
    pts = np.concatenate([p for p, _ in clouds]).astype(np.float32)
    lab = np.concatenate([l for _, l in clouds]).astype(np.int64)
    return pts, lab, np.concatenate([[0], np.cumsum([len(p) for p, _ in clouds])]).astype(np.int64)


def cpu_map(name):
    """The map of a case from tests/point_voxel_refs.py: (points [T, 4], own, corner, weight float64, V)."""
    grid, level, query = case_clouds(name)
    lp, _, loff = flat(level)
    keys = pv.level_keys(lp, loff, grid, LO, HI)
    qp, _, qoff = flat(query)
    own, corner, weight = pv.trilinear_index(qp, qoff, keys, grid, LO, HI)
    return qp, own, corner, weight, len(keys)


def lift_points(points4, cin, seed):
    """The point array of a lift case: the cloud's [T, 4], widened to 8 seeded columns when Cin > 4
    (so that ldp > Cin for the others)."""
    if cin <= 4:
        return np.ascontiguousarray(points4, np.float32)
    rng = np.random.default_rng(1000 + seed)
    return np.concatenate([points4, rng.standard_normal((len(points4), 4))], axis=1).astype(np.float32)


def lift_params(seed, C, cin, bias):
    """(W [C, Cin], b [C] or None) float32."""
    rng = np.random.default_rng(2000 + seed)
    W = (rng.standard_normal((C, cin)) / np.sqrt(cin)).astype(np.float32)
    return W, ((0.5 * rng.standard_normal(C)).astype(np.float32) if bias else None)


def head_params(seed, C, K, bias):
    """(W [K, C], b [K] or None) float32."""
    rng = np.random.default_rng(3000 + seed)
    W = (rng.standard_normal((K, C)) / np.sqrt(C)).astype(np.float32)
    return W, ((0.5 * rng.standard_normal(K)).astype(np.float32) if bias else None)


def rows(seed, n, C):
    """bf16-exact float32 [n, C] features or gradients."""
    return bf16_exact(np.random.default_rng(4000 + seed).standard_normal((n, C)).astype(np.float32))


def labels_for(seed, T, K, ignored=0.25):
    """int64 [T] in [0, K) with a share of -1."""
    rng = np.random.default_rng(5000 + seed)
    y = rng.integers(0, K, size=T).astype(np.int64)
    y[rng.random(T) < ignored] = -1
    return y


def class_weights(seed, K):
    return np.random.default_rng(6000 + seed).uniform(0.5, 2.0, size=K).astype(np.float32)


# (map, Cin, C, bf16 output, bias): the lift cases of tests/test_gpu_point_head.py; the seed of a
# case is its position
LIFT_CASES = [
    ("A", 4, 64, True, True), ("A", 1, 8, False, False), ("A", 8, 96, True, True), ("A", 4, 256, False, True),
    ("A", 4, 20, False, True),
    ("B", 4, 64, True, True), ("B", 8, 96, False, False), ("B", 1, 256, True, True),
    ("C", 4, 64, False, True), ("C", 1, 96, True, False),
    ("D", 4, 64, True, True), ("D", 8, 8, False, True),
]

# (map, C, K, bf16 features, bias, class weights): the head cases
HEAD_CASES = [
    ("A", 64, 2, True, True, True), ("A", 8, 1, False, False, False), ("A", 96, 5, True, True, False),
    ("A", 256, 16, False, True, True), ("A", 20, 3, False, True, True),
    ("B", 64, 2, True, True, True), ("B", 96, 16, True, False, True), ("B", 8, 5, False, True, False),
    ("C", 64, 2, False, True, True), ("C", 96, 1, True, True, False),
    ("D", 64, 5, True, True, True), ("D", 256, 2, True, False, False),
]
