#!/usr/bin/env python3
"""Timing of the logistic associaTR scan (trk_assoc_scan_logistic) with the linear scan on the same batch as the
yardstick (not the bench contract): 100k loci x 10k samples, K covariates, a 0/1 outcome of the given prevalence.

  A  Engine.assoc_scan_logistic on [y, covariates]        (scan + filters + k_assoc_logit)
  B  Engine.assoc_scan on the same block                  (scan + filters + Cholesky regression)

in ONE process, alternating A and B over --rounds rounds after a warm-up of both, timed by a host clock around work that
ends in a device synchronise and by the engine's event timers (k_assoc_scan: the scan bracket; k_assoc_finalize: filters +
regression, which for A holds k_assoc_vect and k_assoc_logit).  The split between the scan and k_assoc_logit per kernel:
run this tool under `rocprofv3 --kernel-trace --stats` in a run of its own.  Also prints the mean and the largest
TRK_AI_N_ITER and the status counts."""
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
ap.add_argument('--covars', type=int, default=12)
ap.add_argument('--prevalence', type=float, default=0.4)
ap.add_argument('--rounds', type=int, default=5)
a = ap.parse_args()
K = a.covars
eng = Engine(0)
sb = SynthBatch(eng, a.loci, a.samples, seed=20260928 + 5, planes=())
alen, rcls = pack_assoc_tables(sb.loci.allele_lens, 2)
alen_d, rcls_d = eng.upload(alen, np.float64), eng.upload(rcls, np.uint16)
rng = np.random.default_rng(5)
vec = rng.normal(size=(1 + K, a.samples))
vec -= vec.mean(axis=1, keepdims=True)
vec /= vec.std(axis=1, keepdims=True)
eta = np.log(a.prevalence / (1 - a.prevalence)) + 0.1 * vec[1:].sum(axis=0)
vec[0] = rng.random(a.samples) < 1 / (1 + np.exp(-eta))
vec_d = eng.upload(vec, np.float64)
outs = {'logistic': None, 'linear': None}


def run(name):
    fn = eng.assoc_scan_logistic if name == 'logistic' else eng.assoc_scan
    kw = dict(outcome_checked=True) if name == 'logistic' else dict(out=outs[name])
    if name == 'logistic' and outs[name] is not None:
        for x in (outs[name].locus_int, outs[name].locus_f64, outs[name].allele_count):
            x.free()
    outs[name] = fn(sb.batch, vec_d, alen_d, rcls_d, non_major_cutoff=20.0, **kw)


def timed(name):
    eng.profile_reset()
    eng.sync(); t0 = time.time()
    run(name)
    eng.sync(); wall = (time.time() - t0) * 1e3
    pg = eng.profile_get()
    return wall, pg['k_assoc_scan'][1], pg['k_assoc_finalize'][1]


eng.profile(True)
for _ in range(2):                       # warm-up of both: code objects, the workspace at both sizes
    run('logistic'); run('linear')
rows = {'logistic': [], 'linear': []}
for r in range(a.rounds):
    for name in rows:
        rows[name].append(timed(name))
for name, rr in rows.items():
    rr = np.array(rr)
    print("%-8s wall %8.3f ms (min %.3f max %.3f)   scan bracket %8.3f ms   finalise bracket %8.3f ms   [median of %d]" % (
        name, np.median(rr[:, 0]), rr[:, 0].min(), rr[:, 0].max(), np.median(rr[:, 1]), np.median(rr[:, 2]), a.rounds), flush=True)
li = outs['logistic'].locus_int.get()
st = li[:, TL.AI_STATUS]
ok = st == TL.AS_OK
print("K=%d prevalence %.2f  %d x %d: statuses %s; N_ITER over the %d fitted loci: mean %.2f max %d" % (
    K, a.prevalence, a.loci, a.samples, dict(zip(*[x.tolist() for x in np.unique(st, return_counts=True)])), ok.sum(),
    li[ok, TL.AI_N_ITER].mean() if ok.any() else float('nan'), li[ok, TL.AI_N_ITER].max() if ok.any() else 0))
