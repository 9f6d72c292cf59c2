"""A plain restatement of trk_mosaic_fit's definition (include/trk.h) in numpy and Python loops, in float64 or any wider
numpy float type (``dt``).  The f step is a bisection on the derivative of each branch run to a fixed 200 halvings."""
import numpy as np

ZERO = 10e-200
FIT, NOCALL, UNSUPPORTED, SINGLE = 0, 1, 2, 3


def stutter_table(u, d, rho, dt=np.float64):
    """P[delta + 100] for delta = -100 .. 100 (StutterProb)."""
    u, d, rho = dt(u), dt(d), dt(rho)
    tab = np.empty(201, dtype=dt)
    tab[100] = 1 - u - d
    for k in range(1, 101):
        tab[100 + k] = (u * rho) * (1 - rho) ** (k - 1)
        tab[100 - k] = (d * rho) * (1 - rho) ** (k - 1)
    return tab


def status(A, B, vals, output_all=False):
    if A is None or B is None or len(vals) == 0:
        return NOCALL
    if A not in vals or (B not in vals and not output_all):
        return UNSUPPORTED
    if len(set(vals)) == 1 and not output_all:
        return SINGLE
    return FIT


def _p(tab, delta):
    return tab[100 + np.clip(delta, -100, 100)]


def _ll(vals, cnts, tab, A, B, C, f):
    """(LL_1, LL_2) at (C, f), the reads added in ascending order."""
    dt = tab.dtype.type
    half, f = dt(0.5), dt(f)
    if C == A or C == B:
        v1 = v2 = np.full(len(vals), dt(ZERO))
    else:
        pa, pb, pc = _p(tab, vals - A), _p(tab, vals - B), _p(tab, vals - C)
        v1 = (half * pa + (half - f) * pb) + f * pc
        v2 = ((half - f) * pa + half * pb) + f * pc
    l1 = l2 = dt(0)
    for t1, t2 in zip(cnts.astype(dt) * np.log(v1), cnts.astype(dt) * np.log(v2)):
        l1 = l1 + t1
        l2 = l2 + t2
    return l1, l2


def LL(vals, cnts, tab, A, B, C, f):
    l1, l2 = _ll(vals, cnts, tab, A, B, C, f)
    return l2 if l2 > l1 else l1


def c_step(vals, cnts, tab, A, B, f):
    best, c_final = -np.inf, 0
    for c in range(int(vals[0]) - 3, int(vals[-1]) + 4):
        ll = LL(vals, cnts, tab, A, B, c, f)
        if ll > best:
            best, c_final = ll, c
    return c_final


def f_step(vals, cnts, tab, A, B, C):
    dt = tab.dtype.type
    n = cnts.astype(dt)
    pa, pb, pc = _p(tab, vals - A), _p(tab, vals - B), _p(tab, vals - C)
    half, zero = dt(0.5), np.zeros(len(vals), dtype=dt)
    fs = []
    for k, b in enumerate((pc - pb, pc - pa) if C != A and C != B else (zero, zero)):
        def g(f):   # d LL_k / d f = sum n b_k / L_k(f)
            v = (half * pa + (half - f) * pb) + f * pc if k == 0 else ((half - f) * pa + half * pb) + f * pc
            return np.sum(n * b / v)
        if g(dt(0)) <= 0:
            fs.append(dt(0))
        elif g(dt(0.5)) >= 0:
            fs.append(dt(0.5))
        else:
            lo, hi = dt(0), dt(0.5)
            for _ in range(200):
                mid = (lo + hi) / 2
                if g(mid) > 0:
                    lo = mid
                else:
                    hi = mid
            fs.append((lo + hi) / 2)
    l1 = _ll(vals, cnts, tab, A, B, C, fs[0])[0]
    l2 = _ll(vals, cnts, tab, A, B, C, fs[1])[1]
    return fs[1] if l2 > l1 else fs[0]


def fit(vals, cnts, A, B, tab):
    """The fitted values of one call: dict(C (None: absent), f, pval, ll_fit, ll_null, support, nonconv)."""
    vals, cnts = np.asarray(vals, dtype=np.int64), np.asarray(cnts, dtype=np.int64)
    dt = tab.dtype.type
    f = dt(0.01)
    C = c_step(vals, cnts, tab, A, B, f)
    f = f_step(vals, cnts, tab, A, B, C)
    it, nonconv = 1, False
    while True:
        c_prev, f_prev = C, f
        C = c_step(vals, cnts, tab, A, B, f)
        f = f_step(vals, cnts, tab, A, B, C)
        it += 1
        if it > 100:
            nonconv = True
            break
        if abs(f - f_prev) < 0.01 and (f < 0.000001 or C == c_prev):
            break
    ll_null = LL(vals, cnts, tab, A, B, C, 0)
    if f == 0:
        return dict(C=None, f=f, pval=dt(1), ll_fit=ll_null, ll_null=ll_null, support=0, nonconv=nonconv)
    ll_fit = LL(vals, cnts, tab, A, B, C, f)
    t = -2 * (ll_null - ll_fit)
    pval = dt(0.5) * (t <= 0) + dt(0.5) * np.exp(-t / 2)
    return dict(C=C, f=f, pval=pval, ll_fit=ll_fit, ll_null=ll_null, support=int(cnts[vals == C].sum()), nonconv=nonconv)
