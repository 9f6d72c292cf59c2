#!/usr/bin/env python
"""Record what the REAL reference's prancSTR computes for a few hundred seeded calls (build container only).

Imports the reference (cyvcf2 through tools/refshim) and runs its MaximizeMosaicLikelihoodBoth, ComputePvalue,
Likelihood_mosaic, ExtractReadVector and StutterProb; writes tests/golden/prancstr/cases.json: the inputs, the
reference's C, f, pval and its log likelihood at its own (C, f), and two margins measured between the reference and
tests/mosaic_ref.py (never the device): f_margin, the largest |f_reference - f_mosaic_ref|, which is SLSQP's own
stopping error, and pval_margin, the same for the p-value.  A case on whose C the two disagree is dropped; more than
2 % dropped is an error.
    python tools/gen_golden_prancstr.py [--reference /root/reference] [--cases 300] [--seed 7]"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, 'refshim'))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))


def draw_call(rng):
    """A call drawn from the model itself: a genotype, sometimes a mosaic allele at fraction f, stutter on every read."""
    u, d, rho = rng.uniform(0.01, 0.3), rng.uniform(0.01, 0.3), 0.95 - rng.uniform(0.0, 0.45)
    period = int(rng.integers(1, 7))
    A = int(rng.integers(-15, 15))
    B = A + int(rng.integers(0, 6))
    f = rng.uniform(0.05, 0.35) if rng.random() < 0.85 else 0.0
    C = A + int(rng.integers(-6, 10))
    reads = []
    for _ in range(int(rng.integers(20, 80))):
        x = rng.random()
        al = C if x < f else (A if x < f + (1 - f) / 2 else B)
        x = rng.random()
        if x < u:
            al += int(rng.geometric(rho))
        elif x < u + d:
            al -= int(rng.geometric(rho))
        reads.append(al)
    vals, cnts = np.unique(reads, return_counts=True)
    text = ';'.join('%d|%d' % (v * period + int(rng.integers(0, period)), n) for v, n in zip(vals, cnts))
    return dict(A=A, B=B, u=u, d=d, rho=rho, period=period, mallreads=text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    ap.add_argument('--cases', type=int, default=300)
    ap.add_argument('--seed', type=int, default=7)
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    import trtools.prancSTR.prancSTR as rp     # the reference
    import mosaic_ref as ref
    rng = np.random.default_rng(a.seed)
    kept, dropped, f_margin, pval_margin = [], 0, 0.0, 0.0
    while len(kept) + dropped < a.cases:
        c = draw_call(rng)
        reads = rp.ExtractReadVector(c['mallreads'], c['period'])
        if c['A'] not in reads or c['B'] not in reads or len(set(reads)) == 1:
            continue                               # the reference would not test this call
        probs = [rp.StutterProb(k, c['u'], c['d'], c['rho']) for k in range(-rp.MAXSTUTTEROFFSET, rp.MAXSTUTTEROFFSET)]
        C, f = rp.MaximizeMosaicLikelihoodBoth(reads, c['A'], c['B'], probs, quiet=True)
        pval = rp.ComputePvalue(reads, c['A'], c['B'], C, f, probs)
        # the likelihood at the reference's own point; without C the f term is zero: any allele outside {A, B} stands in
        c_ll = C if C is not None else next(x for x in range(min(reads) - 3, max(reads) + 4) if x not in (c['A'], c['B']))
        ll = rp.Likelihood_mosaic(c['A'], c['B'], c_ll, f, reads, probs)
        vals, cnts = np.unique(reads, return_counts=True)
        mine = ref.fit(vals, cnts, c['A'], c['B'], ref.stutter_table(c['u'], c['d'], c['rho']))
        if mine['C'] != C:
            dropped += 1
            continue
        f_margin = max(f_margin, abs(float(mine['f']) - float(f)))
        pval_margin = max(pval_margin, abs(float(mine['pval']) - float(pval)))
        c.update(reads=[int(r) for r in reads], stutter_probs=[probs[rp.MAXSTUTTEROFFSET + k] for k in range(-3, 4)],
                 C=C, f=float(f), pval=float(pval), ll=float(ll))
        kept.append(c)
    if dropped > 0.02 * a.cases:
        raise SystemExit("%d of %d cases dropped: the reference's C differs from mosaic_ref's" % (dropped, a.cases))
    out = os.path.join(REPO, 'tests', 'golden', 'prancstr')
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'cases.json'), 'w') as fh:
        json.dump(dict(seed=a.seed, dropped=dropped, f_margin=f_margin, pval_margin=pval_margin, cases=kept), fh, indent=0)
    print("kept %d, dropped %d, f_margin %.3e, pval_margin %.3e" % (len(kept), dropped, f_margin, pval_margin))


if __name__ == '__main__':
    main()
