"""fp64 numpy statement of the two-source sparse convolution (pcs_sparse_conv_cat*; sparse.py's
submanifold_conv3d_cat), with x = [xa | xb] along channels and W in the kernel layout
[Cout, taps, CA + CB]:

    y[m]     = b + sum_t ( W[:, tw(t), :CA] xa[nbr[m][t]] + W[:, tw(t), CA:] xb[nbr[m][t]] ),
               tw(t) = flip ? taps - 1 - t : t
    dxa, dxb = the column blocks [:CA], [CA:] of the gather of dy with W^T (Wt[ci][t][co] = W[co][t][ci])
    dW[co][t][ci] = sum_m dy[m][co] x[nbr[m][t]][ci],  db[co] = sum_m dy[m][co]

Every function takes numpy arrays (any float dtype, converted to fp64) and an int map with -1 for
an empty entry."""
import numpy as np


def _tw(t, taps, flip):
    return taps - 1 - t if flip else t


def conv_cat(nbr, xa, xb, w, b=None, flip=0):
    """y [M, Cout] of the forward; the two sources are never concatenated here either."""
    xa, xb, w = np.asarray(xa, np.float64), np.asarray(xb, np.float64), np.asarray(w, np.float64)
    (M, taps), ca, cout = nbr.shape, xa.shape[1], w.shape[0]
    y = np.zeros((M, cout)) if b is None else np.tile(np.asarray(b, np.float64), (M, 1))
    for t in range(taps):
        rows = np.nonzero(nbr[:, t] >= 0)[0]
        src = nbr[rows, t]
        wt = w[:, _tw(t, taps, flip), :]
        y[rows] += xa[src] @ wt[:, :ca].T + xb[src] @ wt[:, ca:].T
    return y


def weight_t(w):
    """Wt [Cin, taps, Cout] of W [Cout, taps, Cin] (pcs_conv3d_weight_t)."""
    return np.ascontiguousarray(np.transpose(np.asarray(w, np.float64), (2, 1, 0)))


def dgrad_cat(nbr, dy, w, ca, flip=1):
    """(dxa [M, CA], dxb [M, CB]) of pcs_sparse_conv_cat_dgrad: the gather of dy through nbr with
    Wt and the tap order of flip, cut into the two column blocks."""
    dy, wt = np.asarray(dy, np.float64), weight_t(w)
    M, taps = nbr.shape
    dx = np.zeros((M, wt.shape[0]))
    for t in range(taps):
        rows = np.nonzero(nbr[:, t] >= 0)[0]
        dx[rows] += dy[nbr[rows, t]] @ wt[:, _tw(t, taps, flip), :].T
    return dx[:, :ca], dx[:, ca:]


def wgrad_cat(nbr, xa, xb, dy):
    """(dW [Cout, taps, CA + CB], db [Cout]) with X's columns taken from xa, then xb."""
    xa, xb, dy = np.asarray(xa, np.float64), np.asarray(xb, np.float64), np.asarray(dy, np.float64)
    (M, taps), ca, cb, cout = nbr.shape, xa.shape[1], xb.shape[1], dy.shape[1]
    dw = np.zeros((cout, taps, ca + cb))
    for t in range(taps):
        rows = np.nonzero(nbr[:, t] >= 0)[0]
        src = nbr[rows, t]
        dw[:, t, :ca] = dy[rows].T @ xa[src]
        dw[:, t, ca:] = dy[rows].T @ xb[src]
    return dw, dy.sum(0)
