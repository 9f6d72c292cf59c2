#!/usr/bin/env python
"""Times trk_compare (compareSTR's concordance pass) and, in the same process, trk_qc_reduce with a quality plane --
both move 8 B per call -- with the engine's event timers.  Default 100 000 loci x 10 000 samples.
    python tools/compare_probe.py [--loci L] [--samples S] [--reps R]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--loci', type=int, default=100000)
    ap.add_argument('--samples', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    from trtools_amd.engine import Engine
    from trtools_amd.synth import SynthBatch
    eng = Engine(0, reserve_pair_gb=0)
    sb1 = SynthBatch(eng, a.loci, a.samples, seed=1)
    sb2 = SynthBatch(eng, a.loci, a.samples, seed=2)
    off = sb1.tables[0]
    nA = int(off[-1])
    ids = eng.upload((np.arange(nA) - np.repeat(off[:-1], np.diff(off))).astype(np.uint16))   # the allele's index: the same on both sides
    dlen = eng.upload(np.arange(nA, dtype=np.float64) % 7 - 3)
    offd = eng.upload(np.asarray(off, dtype=np.int32))
    sides = [dict(gt=sb.batch.arrays['gt'], allele_off=offd, seq_id=ids, len_id=ids, dlen=dlen) for sb in (sb1, sb2)]
    dabs = eng.upload(np.full(a.loci, -5.0))
    acc = eng.compare_accumulators(a.samples)
    q = eng.upload(np.random.default_rng(0).random((a.loci, a.samples), dtype=np.float32))

    held = list(acc.values())

    def timed(fn):
        fn()
        best = []
        for _ in range(a.reps):
            eng.timer_start(0)
            r = fn()
            eng.timer_stop(0)
            best.append(eng.timer_ms(0))
            for v in r.values():
                if hasattr(v, 'free') and not any(v is x for x in held):
                    v.free()
        return round(float(np.median(best)), 4), [round(x, 4) for x in best]
    cmp_ms = timed(lambda: eng.compare_calls(sides, dabs, acc=acc))
    ph = [eng.upload(np.zeros((a.loci, a.samples), np.uint8)) for _ in range(2)]
    phased = [dict(sd, phased=p) for sd, p in zip(sides, ph)]
    cmp_ph_ms = timed(lambda: eng.compare_calls(phased, dabs, acc=acc))
    dp = [sb.dev['dp'] for sb in (sb1, sb2)]
    acc_s = eng.compare_accumulators(a.samples, 1, 10)
    held.extend(acc_s.values())
    cmp_st_ms = timed(lambda: eng.compare_calls(sides, dabs, acc=acc_s, fields=[dict(planes=dp, edges=np.arange(0, 51, 5.0), stratify_file=0)]))
    qc_ms = timed(lambda: {k: v for k, v in eng.qc_reduce(sb1.batch, q).items() if k != '_keep'})
    print(json.dumps(dict(loci=a.loci, samples=a.samples, compare_ms=cmp_ms[0], compare_all=cmp_ms[1],
                          qc_reduce_ms=qc_ms[0], qc_all=qc_ms[1],
                          compare_phased_ms=cmp_ph_ms[0], compare_strat_dp10_ms=cmp_st_ms[0],
                          compare_tb_s=round(8.0 * a.loci * a.samples / cmp_ms[0] / 1e9, 3))))
    eng.close()


if __name__ == '__main__':
    main()
