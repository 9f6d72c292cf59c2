"""The mosaic fit against the real reference's prancSTR (cases.json of tools/gen_golden_prancstr.py, which also measured
f_margin and pval_margin, SLSQP's stopping error, on the CPU) and mosaic_fit_records on a small HipSTR-format VCF."""
import json
import os

import numpy as np
import pytest

import mosaic_ref as ref
from test_gpu_mosaic import eng   # noqa: F401 (the module's engine fixture)
from trtools_amd import _lib as L
from trtools_amd import prancSTR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, 'golden', 'prancstr', 'cases.json')))
CASES = GOLD['cases']
VCF = os.path.join(HERE, 'golden', 'data', 'statSTR', 'test_longtr.vcf')   # one sample, 67 loci, HipSTR's FORMAT fields


def test_host_functions_match_recorded():
    for c in CASES:
        assert prancSTR.ExtractReadVector(c['mallreads'], c['period']) == c['reads']
        assert [prancSTR.StutterProb(k, c['u'], c['d'], c['rho']) for k in range(-3, 4)] == c['stutter_probs']
    assert prancSTR.ExtractReadVector(None, 2) == [] and prancSTR.ExtractReadVector('.', 2) == []
    assert [prancSTR.ConfineRange(x, -100, 100) for x in (-101, 5, 300)] + [prancSTR.SF(x) for x in (-1, 0, 0.5)] == [-100, 5, 100, 1, 1, 0]


def test_restatement_matches_reference():
    assert GOLD['dropped'] <= 0.02 * (len(CASES) + GOLD['dropped'])
    for c in CASES:
        vals, cnts = prancSTR.read_counts(c['reads'])
        w = ref.fit(vals, cnts, c['A'], c['B'], ref.stutter_table(c['u'], c['d'], c['rho']))
        assert w['C'] == c['C'] and abs(w['f'] - c['f']) <= GOLD['f_margin'] and abs(w['pval'] - c['pval']) <= GOLD['pval_margin']
        assert w['ll_fit'] >= c['ll'] - 1e-9 * abs(c['ll'])


@pytest.mark.gpu
def test_device_matches_reference(eng):
    """Every case a locus of its own (its own stutter table), one call each."""
    parts = [prancSTR.read_counts(c['reads']) for c in CASES]
    off = np.concatenate([[0], np.cumsum([v.size for v, _ in parts])]).astype(np.int32)
    res = eng.mosaic_fit(np.array([[[c['A'], c['B']]] for c in CASES], dtype=np.int32), off,
                         np.concatenate([v for v, _ in parts]), np.concatenate([n for _, n in parts]),
                         np.array([[c['u'], c['d'], c['rho']] for c in CASES]))
    got = {k: v.get().reshape(-1) for k, v in res.items()}
    for i, c in enumerate(CASES):
        assert (got['status'][i] & 0xf) == L.MOSAIC_FIT
        assert (None if got['status'][i] & L.MOSAIC_NO_C else got['C'][i]) == c['C'], (i, c)
        assert got['ll_fit'][i] >= c['ll'] - 1e-9 * abs(c['ll']), (i, got['ll_fit'][i], c['ll'])
        assert abs(got['f'][i] - c['f']) <= 2 * GOLD['f_margin'], (i, got['f'][i], c['f'])
        assert abs(got['pval'][i] - c['pval']) <= 2 * GOLD['pval_margin'], (i, got['pval'][i], c['pval'])


@pytest.mark.gpu
def test_reference_names_are_batches_of_one(eng):
    for c in CASES[:3]:
        probs = [prancSTR.StutterProb(k, c['u'], c['d'], c['rho']) for k in range(-200, 200)]
        C, f = prancSTR.MaximizeMosaicLikelihoodBoth(c['reads'], c['A'], c['B'], probs, engine=eng)
        assert C == c['C'] and abs(f - c['f']) <= 2 * GOLD['f_margin']
        pval = prancSTR.ComputePvalue(c['reads'], c['A'], c['B'], C, f, probs, engine=eng)
        assert abs(pval - c['pval']) <= 2 * GOLD['pval_margin']


@pytest.mark.gpu
@pytest.mark.parametrize('readfield,output_all', [('MALLREADS', False), ('ALLREADS', True)])
def test_mosaic_fit_records(eng, readfield, output_all):
    import trtools_amd.utils.tr_harmonizer as trh
    from trtools_amd import vcfio
    recs = [trh.HarmonizeRecord(trh.VcfTypes.hipstr, v) for v in vcfio.VCFReader(VCF)]
    out = prancSTR.mosaic_fit_records(recs, readfield=readfield, output_all=output_all, engine=eng)
    n_fit = 0
    for l, rec in enumerate(recs):
        period = len(rec.motif)
        text = rec.format[readfield][0]
        reads = prancSTR.ExtractReadVector(text, period)
        A, B = prancSTR.ExtractAB(rec)[0]
        A, B = (None, None) if A is None else (A // period, B // period)
        lo, hi = out['read_off'][l], out['read_off'][l + 1]
        assert np.repeat(out['read_val'][lo:hi], out['read_cnt'][lo:hi]).tolist() == sorted(reads)
        assert out['reads'][l][0] == text and out['dp'][l, 0] == max(int(rec.format['DP'][0][0]), 0)
        assert tuple(out['stutter'][l]) == (0.05, 0.05, 0.90)        # the file has no INFRAME_* fields
        st = ref.status(A, B, reads, output_all)
        assert (out['status'][l, 0] & 0xf) == st
        if st != ref.FIT:
            continue
        n_fit += 1
        w = ref.fit(out['read_val'][lo:hi], out['read_cnt'][lo:hi], A, B, ref.stutter_table(0.05, 0.05, 0.90))
        assert (None if out['status'][l, 0] & L.MOSAIC_NO_C else out['C'][l, 0]) == w['C']
        assert out['support'][l, 0] == w['support'] and abs(out['f'][l, 0] - w['f']) <= 1e-9
        for k in ('ll_fit', 'll_null', 'pval'):
            assert abs(out[k][l, 0] - w[k]) <= 1e-9 * abs(w[k]), (l, k)
    assert n_fit >= 10
