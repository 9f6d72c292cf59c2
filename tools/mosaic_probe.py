#!/usr/bin/env python
"""Times trk_mosaic_fit (prancSTR's per-call model) with the engine's event timers on a synthetic dense grid of calls of
which about a fifth are fitted (four distinct read values each; the others are no-calls or show one read value), and,
for scale, tests/mosaic_ref.py on one core over a few thousand of the same calls.  Default 2000 loci x 5000 samples.
    python tools/mosaic_probe.py [--loci L] [--samples S] [--fitted 0.2] [--reps R] [--ref-calls N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--loci', type=int, default=2000)
    ap.add_argument('--samples', type=int, default=5000)
    ap.add_argument('--fitted', type=float, default=0.2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--ref-calls', type=int, default=2000)
    a = ap.parse_args()
    from trtools_amd import _lib as L
    from trtools_amd.engine import Engine
    import mosaic_ref as ref
    rng = np.random.default_rng(0)
    n = a.loci * a.samples
    x = rng.random(n)
    fit = x < a.fitted
    nocall = x > 0.5 + a.fitted / 2
    A = rng.integers(-20, 20, n).astype(np.int32)
    B = A + rng.integers(1, 5, n).astype(np.int32)
    R = np.where(fit, 4, np.where(nocall, 0, 1)).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(R)]).astype(np.int32)
    val = np.empty(off[-1], np.int32)
    cnt = np.empty(off[-1], np.int32)
    o = off[:-1][fit]
    for k, (v, c) in enumerate(((A - 1, rng.integers(1, 3, n)), (A, rng.integers(10, 30, n)), (B, rng.integers(10, 30, n)),
                                (B + 2, rng.integers(1, 9, n)))):
        val[o + k], cnt[o + k] = v[fit], c[fit]
    single = ~fit & ~nocall
    val[off[:-1][single]], cnt[off[:-1][single]] = A[single], 20
    ab = np.stack([A, B], axis=1)
    ab[nocall] = L.MOSAIC_NOCALL_AB
    stutter = np.column_stack([rng.uniform(0.01, 0.3, a.loci), rng.uniform(0.01, 0.3, a.loci), rng.uniform(0.5, 0.95, a.loci)])
    eng = Engine(0, reserve_pair_gb=0)
    dev = [eng.upload(np.ascontiguousarray(v)) for v in (ab.reshape(a.loci, a.samples, 2), off, val, cnt, stutter)]
    ms = []
    for rep in range(a.reps + 1):
        eng.timer_start(0)
        res = eng.mosaic_fit(*dev)
        eng.timer_stop(0)
        if rep:
            ms.append(eng.timer_ms(0))
        if rep == a.reps:
            status = res['status'].get().reshape(-1)
        for v in res.values():
            v.free()
    n_fit = int(np.count_nonzero((status & 0xf) == L.MOSAIC_FIT))
    eng.close()
    idx = np.flatnonzero(fit)[:a.ref_calls]
    t0 = time.perf_counter()
    for c in idx:
        ref.fit(val[off[c]:off[c + 1]], cnt[off[c]:off[c + 1]], int(A[c]), int(B[c]), ref.stutter_table(*stutter[c // a.samples]))
    ref_us = (time.perf_counter() - t0) / max(len(idx), 1) * 1e6
    med = float(np.median(ms))
    print(json.dumps(dict(loci=a.loci, samples=a.samples, calls=n, fitted=n_fit, pass_ms=round(med, 3),
                          pass_all=[round(v, 3) for v in ms], ns_per_fitted_call=round(med * 1e6 / max(n_fit, 1), 2),
                          ref_calls=len(idx), ref_us_per_call_one_core=round(ref_us, 1))))


if __name__ == '__main__':
    main()
