#!/usr/bin/env python3
"""Timing of the multi-outcome associaTR scan against the single-outcome scans it replaces (not the bench contract):
100k loci x 10k samples, T outcomes + K shared covariates.

  A  one Engine.assoc_scan_multi call on the [T + K, S] block
  B  T Engine.assoc_scan calls, each on [y_t, covariates]

in ONE process, alternating A and B over --rounds rounds after a warm-up of both, timed by the engine's event timers
(k_assoc_scan: vector block + scan + Gram correction; k_assoc_finalize: filters + regression) and by a host clock around
work that ends in a device synchronise.  The split of the scan bracket into scan / Gram correction and of the finalise
bracket into filters / regression is per kernel: run this tool under `rocprofv3 --kernel-trace --stats` in a run of its
own (kernel names: k_assoc_scan_mfma, k_assoc_gram_miss, k_assoc_finalize, k_assoc_regress_multi, k_assoc_regress_wave).
Also checks that A's [L, T, 5] agrees with B's columns on the timed inputs."""
import os as _os; _os.environ.setdefault('TRK_LAB', '1')   # a tool: lab knobs are honoured (trtools_amd/_knobs.py)
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from trtools_amd import _lib as TL
from trtools_amd.engine import Engine
from trtools_amd.synth import SynthBatch, pack_assoc_tables

ap = argparse.ArgumentParser()
ap.add_argument('--loci', type=int, default=100000)
ap.add_argument('--samples', type=int, default=10000)
ap.add_argument('--outcomes', type=int, default=16)
ap.add_argument('--covars', type=int, default=15)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--subset', action='store_true')
a = ap.parse_args()
T, K = a.outcomes, a.covars
eng = Engine(0)
sb = SynthBatch(eng, a.loci, a.samples, seed=20260928 + 5, planes=())
alen, rcls = pack_assoc_tables(sb.loci.allele_lens, 2)
alen_d, rcls_d = eng.upload(alen, np.float64), eng.upload(rcls, np.uint16)
rng = np.random.default_rng(5)
sin = (rng.random(a.samples) < 0.9).astype(np.uint8) if a.subset else None
sin_d = eng.upload(sin, np.uint8) if sin is not None else None
vec = rng.normal(size=(T + K, a.samples))
vec -= vec.mean(axis=1, keepdims=True)
vec /= vec.std(axis=1, keepdims=True)
multi_d = eng.upload(vec, np.float64)
single_d = [eng.upload(np.ascontiguousarray(vec[[t] + list(range(T, T + K))]), np.float64) for t in range(T)]
singles = [None] * T


def run_multi():
    return eng.assoc_scan_multi(sb.batch, multi_d, T, alen_d, rcls_d, sample_in=sin_d, non_major_cutoff=20.0)


def run_singles():
    for t in range(T):
        singles[t] = eng.assoc_scan(sb.batch, single_d[t], alen_d, rcls_d, sample_in=sin_d, non_major_cutoff=20.0,
                                    out=singles[t])


def timed(fn):
    eng.profile_reset()
    eng.sync(); t0 = time.time()
    out = fn()
    eng.sync(); wall = (time.time() - t0) * 1e3
    pg = eng.profile_get()
    return out, wall, pg['k_assoc_scan'][1], pg['k_assoc_finalize'][1]


eng.profile(True)
for _ in range(2):                       # warm-up of both: code objects, the workspace at both sizes
    res, per = run_multi()
    for x in (res.locus_int, res.locus_f64, res.allele_count, per):
        x.free()
    run_singles()
rows = {'multi': [], 'singles': []}
for r in range(a.rounds):
    (res, per), *m = timed(run_multi)
    _, *s = timed(run_singles)
    rows['multi'].append(m)
    rows['singles'].append(s)
    if r < a.rounds - 1:
        for x in (res.locus_int, res.locus_f64, res.allele_count, per):
            x.free()
for name, rr in rows.items():
    rr = np.array(rr)
    print("%-8s wall %8.3f ms (min %.3f max %.3f)   scan bracket %8.3f ms   finalise bracket %8.3f ms   [median of %d]" % (
        name, np.median(rr[:, 0]), rr[:, 0].min(), rr[:, 0].max(), np.median(rr[:, 1]), np.median(rr[:, 2]), a.rounds), flush=True)
print("T=%d K=%d  %d x %d%s: multi / singles wall = %.3f" % (T, K, a.loci, a.samples, ' subset' if a.subset else '',
      np.median(np.array(rows['multi'])[:, 0]) / np.median(np.array(rows['singles'])[:, 0])))
# the same numbers?  (float columns of the tested loci, relative)
per_h, li = per.get(), res.locus_int.get()
ok = li[:, TL.AI_STATUS] == TL.AS_OK
assert np.isfinite(per_h[ok]).all() and np.isnan(per_h[~ok]).all()
worst = 0.0
for t in range(T):
    lf = singles[t].locus_f64.get()
    assert np.array_equal(singles[t].locus_int.get(), li), t
    one = lf[ok][:, [TL.AF_PVAL, TL.AF_COEF, TL.AF_SE, TL.AF_RSQUARED, TL.AF_TVALUE]]
    worst = max(worst, float(np.max(np.abs(per_h[ok, t] - one) / np.maximum(np.abs(one), 1e-300))))
print("tested %d / %d loci; largest relative difference multi vs singles over p, coef, se, R^2, t: %.3e" % (ok.sum(), a.loci, worst))
