"""The numpy float64 statement of pcs_amd.sparse_norm: BatchNorm over the V rows of x [V, C], then
+ residual, then ReLU, forward and backward, in training and in eval mode.  Build-defined (the
reference has no voxel grid); tests/test_sparse_norm_refs.py proves it against
torch.nn.functional.batch_norm in float64 with autograd."""
import numpy as np


def forward(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5, relu=False, residual=None):
    """A dict: y, pre (before the ReLU), mean / var (what normalised: the batch's, biased, or the
    running buffers), rstd, xhat, and running_mean / running_var after the step (unchanged in eval)."""
    x = np.asarray(x, np.float64)
    V = x.shape[0]
    rm, rv = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
    if training:
        if V < 2:
            raise ValueError("training needs at least 2 rows")
        mean, var = x.mean(0), x.var(0)
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * V / (V - 1)
    else:
        mean, var = rm, rv
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * rstd
    pre = xhat * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    if residual is not None:
        pre = pre + np.asarray(residual, np.float64)
    y = np.maximum(pre, 0.0) if relu else pre
    return {"y": y, "pre": pre, "mean": mean, "var": var, "rstd": rstd, "xhat": xhat, "running_mean": rm,
            "running_var": rv}


def backward(dy, gate, x, gamma, mean, rstd, training):
    """(dx, dgamma, dbeta, dresidual, terms) from the output gradient dy and the ReLU gate (a boolean
    [V, C] array, True where the gradient passes; None without a ReLU).  mean / rstd are forward()'s.
    terms = (|dz|, |dz * xhat|) summed over the rows: the scale of the two column sums."""
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    gamma = np.asarray(gamma, np.float64)
    V = x.shape[0]
    dz = dy if gate is None else np.where(gate, dy, 0.0)
    xhat = (x - mean) * rstd
    s1, s2 = dz.sum(0), (dz * xhat).sum(0)
    if training:
        dx = gamma * rstd * (dz - s1 / V - xhat * s2 / V)
    else:
        dx = gamma * rstd * dz
    return dx, s2, s1, dz, (np.abs(dz).sum(0), np.abs(dz * xhat).sum(0))
