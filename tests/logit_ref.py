"""Plain numpy restatement of trk_assoc_scan_logistic's definition (include/trk.h), in float64 or np.longdouble:
the same start, Newton steps, stopping rule, 30-step cap, rank rule and statuses."""
import math

import numpy as np

OK, COLLINEAR, CONSTANT_OUTCOME, NOT_CONVERGED = 0, 6, 7, 8
MAX_STEPS = 30


def _factor(H, grad, kept):
    """Cholesky of H with the right-hand side carried along (z = L^-1 grad).  kept None: the first factorisation decides
    the columns (d > 1e-11 a_jj); else a kept column failing the rule returns None."""
    P = len(grad)
    Lm, z = np.zeros_like(H), np.zeros_like(grad)
    use = np.zeros(P, dtype=bool)
    for j in range(P):
        d = H[j, j] - Lm[j, :j] @ Lm[j, :j]
        ok = bool(d > H.dtype.type(1e-11) * H[j, j])
        if kept is not None and kept[j] and not ok:
            return None
        use[j] = ok if kept is None else kept[j]
        if not use[j]:
            continue
        Lm[j, j] = np.sqrt(d)
        for i in range(j + 1, P):
            Lm[i, j] = (H[i, j] - Lm[i, :j] @ Lm[j, :j]) / Lm[j, j]
        z[j] = (grad[j] - Lm[j, :j] @ z[:j]) / Lm[j, j]
    return Lm, z, use


def fit(X, y, dtype=np.longdouble):
    """X [n, P] = [1, c_1..c_K, g] over the tested samples, y [n] of 0 / 1.  Returns dict(status, rank, n_iter, coef, se,
    z, pval, loglik); the floats are nan unless status is OK."""
    X, y = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype)
    n, P = X.shape
    out = dict(status=OK, rank=0, n_iter=0, coef=math.nan, se=math.nan, z=math.nan, pval=math.nan, loglik=math.nan)

    def stop(status):
        out['status'] = status
        return out
    if y.sum() == 0 or y.sum() == n:
        return stop(CONSTANT_OUTCOME)
    b = np.zeros(P, dtype=dtype)
    ybar = y.sum() / dtype(n)
    b[0] = np.log(ybar / (1 - ybar))
    kept = None

    def moments(b):
        eta = X @ b
        mu = 1 / (1 + np.exp(-eta))
        return eta, (X * (mu * (1 - mu))[:, None]).T @ X, X.T @ (y - mu)

    while True:
        eta, H, grad = moments(b)
        f = _factor(H, grad, kept)
        if f is None:
            return stop(NOT_CONVERGED)
        Lm, z, use = f
        if kept is None:
            kept, out['rank'] = use, int(use.sum())
            if not kept[P - 1]:
                return stop(COLLINEAR)
        delta = np.zeros(P, dtype=dtype)
        for j in range(P - 1, -1, -1):
            if kept[j]:
                delta[j] = (z[j] - Lm[j + 1:, j] @ delta[j + 1:]) / Lm[j, j]
        b = b + delta
        out['n_iter'] += 1
        if not np.all(np.isfinite(b)):
            return stop(NOT_CONVERGED)
        if np.max(np.abs(delta)) <= dtype(1e-9) * max(dtype(1), np.max(np.abs(b))):
            break
        if out['n_iter'] == MAX_STEPS:
            return stop(NOT_CONVERGED)
    eta, H, grad = moments(b)
    f = _factor(H, grad, kept)
    if f is None:
        return stop(NOT_CONVERGED)
    se = 1 / f[0][P - 1, P - 1]
    zval = b[P - 1] / se
    out.update(coef=float(b[P - 1]), se=float(se), z=float(zval), pval=math.erfc(abs(float(zval)) / math.sqrt(2.0)),
               loglik=float(np.sum(y * eta - (np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta)))))))
    return out
