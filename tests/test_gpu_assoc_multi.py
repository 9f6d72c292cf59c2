"""GPU parity of trk_assoc_scan_multi: T outcomes against the same K covariates in one pass over the genotype tensor and
one factorisation per locus (k_assoc_regress_multi), against the associaTR oracle run one outcome at a time, against T
single-outcome scans, and through the command line.  Integers exact; floats by test_gpu_assoc.py's rule (1e-9), which
DESIGN.md section 4 documents for at least 6 tested samples per design column -- every float-checked case keeps that."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from trtools_amd import _lib as TL                      # noqa: E402
from test_gpu_assoc import eng, make_case               # noqa: E402,F401

pytestmark = pytest.mark.gpu
FLOATS = ((TL.AO_COEF, 'coef_std'), (TL.AO_SE, 'se_std'), (TL.AO_RSQUARED, 'rsquared'), (TL.AO_TVALUE, 'tvalue'),
          (TL.AO_PVAL, 'pval'))
AF_OF_AO = [TL.AF_PVAL, TL.AF_COEF, TL.AF_SE, TL.AF_RSQUARED, TL.AF_TVALUE]


def close(a, b, key):
    return abs(a - b) <= 1e-9 * max(abs(b), 1e-300) + (1e-12 if key in ('coef_std', 'tvalue', 'rsquared') else 0)


def build(e, seed, T, K, S, P=2, subset=False, cutoff=3.0, miss=0.04, dup=False, collinear=None, n_loci=40):
    """A seeded batch (test_gpu_assoc.make_case: missing calls, an all-missing and a one-allele locus) plus a locus
    below the non-major cutoff; the designs [y_t, C] of the oracle, the [T + K, S] block of the device and its result."""
    from oracle import associatr_oracle as ao
    from trtools_amd import synth
    lens, gt, lp, traits, keep = make_case(seed, n_loci, S, P, T + K, subset, miss=miss)
    lens[4], gt[4] = [10.0, 12.0], 0
    gt[4, 0, 0] = 1                                            # non-major allele count 1
    if dup:
        traits[:, T + 1] = traits[:, T]
    if collinear is not None:                                  # a covariate that IS a (fully called) locus's summed length
        lens[collinear] = [10.0, 11.0, 13.0]
        gt[collinear] = (np.arange(S * P).reshape(S, P) * 7 // 3) % 3
        traits[:, T] = np.take(np.array(lens[collinear]), gt[collinear]).sum(axis=1)
    names = ['s%d' % i for i in range(S)]
    ok = (keep if keep is not None else np.ones(S, bool)) & ~np.isnan(traits).any(axis=1)
    sub = [n for n, k in zip(names, ok) if k]
    designs = [ao.prepare_design(names, [traits[:, [t] + list(range(T, T + K))]], True, sub) for t in range(T)]
    sf, covars = designs[0][0], designs[0][1]
    vec = np.zeros((T + K, S))
    for t in range(T):
        vec[t, sf] = designs[t][2]
    vec[T:, sf] = covars[:, 2:].T
    off, lc, sc, cv = synth.pack_alleles(lens, None)
    alen, rcls = synth.pack_assoc_tables(lens, 2)
    batch = e.make_batch(gt, off, lc, sc, cv, locus_ploidy=lp)
    sin = None if sf.all() else sf.astype(np.uint8)
    res, per = e.assoc_scan_multi(batch, vec, T, alen, rcls, sample_in=sin, non_major_cutoff=cutoff)
    return dict(lens=lens, gt=gt, sf=sf, designs=designs, vec=vec, off=off, tables=(alen, rcls), batch=batch, sin=sin,
                cutoff=cutoff, li=res.locus_int.get(), lf=res.locus_f64.get(), cnt=res.allele_count.get(), per=per.get())


def check_against_oracle(c, T, K, floats=True, skip=()):
    """Every locus of case ``c`` against oracle/associatr_oracle.py; returns the statuses seen."""
    from oracle import associatr_oracle as ao
    status_of = {None: TL.AS_OK, 'No called samples': TL.AS_NO_CALLED, 'Only one called allele': TL.AS_ONE_ALLELE,
                 'n covars >= n samples': TL.AS_N_COVARS}
    sf, covars = c['sf'], c['designs'][0][1]
    li, lf, per, off = c['li'], c['lf'], c['per'], c['off']
    assert per.shape == (len(c['lens']), T, TL.AO_COLS) and covars.shape[1] == K + 2
    for l, lens in enumerate(c['lens']):
        g = c['gt'][l]
        gi = ao.locus_genotypes(g, lens, sf, c['cutoff'], 2)
        n_tested = int(np.sum(gi['called_samples_filter']))
        reason = gi['locus_filtered'] or ('n covars >= n samples' if covars.shape[1] >= n_tested else None)
        sel = g[sf & ~np.any(g == -1, axis=1)]
        assert li[l, TL.AI_N_TESTED] == n_tested, l
        assert np.array_equal(c['cnt'][off[l]:off[l + 1]], np.bincount(sel[sel >= 0].astype(int), minlength=len(lens))), l
        assert li[l, TL.AI_N_RALLELES] == len(gi['allele_frequency']), l
        if l in skip:
            continue
        if not reason and np.std(np.sum(gi['gts'], axis=1)) <= 1e-9:
            assert li[l, TL.AI_STATUS] == TL.AS_ZERO_VARIANCE and np.isnan(per[l]).all(), (l, li[l])
            continue
        assert li[l, TL.AI_STATUS] == status_of.get(reason, TL.AS_NON_MAJOR), (l, li[l], reason)
        if reason:
            assert np.isnan(per[l]).all() and np.isnan(lf[l, AF_OF_AO]).all(), l
            continue
        for t in range(T if floats else 0):
            r = ao.locus_regression(gi['gts'], gi['called_samples_filter'], covars, c['designs'][t][2], 1.0)
            assert li[l, TL.AI_RANK] == n_tested - r['df_resid'] and lf[l, TL.AF_DF_RESID] == r['df_resid'], (l, li[l])
            for col, key in FLOATS:
                assert close(per[l, t, col], r[key], key), (l, t, key, per[l, t, col], r[key])
        assert np.array_equal(lf[l, AF_OF_AO], per[l, 0]), l                     # outcome 0 in the locus columns
    return set(li[:, TL.AI_STATUS].tolist())


@pytest.mark.parametrize('T,K,S,P,subset,mfma_min', [
    (2, 0, 64, 2, False, None),       # few-row scan, no covariates
    (3, 4, 256, 2, True, '99'),       # k_assoc_scan<8> (the matrix-pipe scan switched off for this size)
    (16, 15, 512, 2, True, None),     # 31 rows: two 16-row tiles
    (52, 10, 512, 2, False, None),    # 62 rows, all 64 lanes, four tiles, three of them outcomes only
    (40, 8, 509, 2, True, None),      # unaligned rows, more than 31 of them: pairs of row groups through the generic scan
    (3, 4, 250, 3, False, None),      # triploid: k_assoc_scan_any
])
def test_multi_outcome_scan_against_oracle(eng, T, K, S, P, subset, mfma_min):
    TL.set_option('TRK_AS_MFMA_MIN', mfma_min)
    try:
        c = build(eng, 100 + T, T, K, S, P, subset)
    finally:
        TL.set_option('TRK_AS_MFMA_MIN', None)
    seen = check_against_oracle(c, T, K)
    assert {TL.AS_OK, TL.AS_NO_CALLED, TL.AS_ONE_ALLELE, TL.AS_NON_MAJOR} <= seen
    assert np.sum(c['li'][:, TL.AI_STATUS] == TL.AS_OK) > 15


def test_duplicated_covariate_is_dropped(eng):
    c = build(eng, 7, 5, 6, 256, dup=True)
    check_against_oracle(c, 5, 6)
    tested = c['li'][:, TL.AI_STATUS] == TL.AS_OK
    assert tested.sum() > 15 and np.all(c['li'][tested, TL.AI_RANK] == 6 + 1)


def test_genotype_collinear_with_a_covariate(eng):
    c = build(eng, 8, 4, 3, 256, collinear=9, cutoff=0.0)
    check_against_oracle(c, 4, 3, skip=(9,))
    assert c['li'][9, TL.AI_STATUS] == TL.AS_COLLINEAR and np.isnan(c['per'][9]).all() and np.isnan(c['lf'][9, TL.AF_PVAL])


def test_n_covars_rule_counts_design_columns_not_outcomes(eng):
    """1 + K + 1 = 6 columns against 16 samples with many missing calls, T + K + 1 = 15 scanned rows: the rule fires where
    a single-outcome run's fires (statuses only: so few samples per column are outside the 1e-9 regime)."""
    c = build(eng, 9, 10, 4, 16, cutoff=0.0, miss=0.35)
    seen = check_against_oracle(c, 10, 4, floats=False)
    assert {TL.AS_OK, TL.AS_N_COVARS} <= seen
    ok = c['li'][:, TL.AI_STATUS] == TL.AS_OK
    assert np.any(ok & (c['li'][:, TL.AI_N_TESTED] <= 15))       # tested although n <= T + K + 1


def test_same_results_as_single_outcome_scans(eng):
    T, K = 16, 15
    c = build(eng, 11, T, K, 512, subset=True)
    for t in range(T):
        one = eng.assoc_scan(c['batch'], c['vec'][[t] + list(range(T, T + K))], *c['tables'], sample_in=c['sin'],
                             non_major_cutoff=c['cutoff'])
        li, lf = one.locus_int.get(), one.locus_f64.get()
        assert np.array_equal(li, c['li']) and np.array_equal(one.allele_count.get(), c['cnt'])
        for l in np.flatnonzero(li[:, TL.AI_STATUS] == TL.AS_OK):
            for col, key in FLOATS:
                assert close(c['per'][l, t, col], lf[l, AF_OF_AO[col]], key), (l, t, key)
        assert np.isnan(c['per'][li[:, TL.AI_STATUS] != TL.AS_OK, t]).all()
    v1 = c['vec'][[0] + list(range(T, T + K))]
    one = eng.assoc_scan(c['batch'], v1, *c['tables'], sample_in=c['sin'], non_major_cutoff=c['cutoff'])
    res, per = eng.assoc_scan_multi(c['batch'], v1, 1, *c['tables'], sample_in=c['sin'], non_major_cutoff=c['cutoff'])
    assert np.array_equal(res.locus_int.get(), one.locus_int.get())
    assert np.array_equal(res.locus_f64.get(), one.locus_f64.get(), equal_nan=True)
    assert np.array_equal(per.get()[:, 0], one.locus_f64.get()[:, AF_OF_AO], equal_nan=True)
    with pytest.raises(TL.TrkError):
        eng.assoc_scan_multi(c['batch'], np.zeros((63, 512)), 2, *c['tables'])


def test_command_line_writes_one_table_per_outcome(tmp_path):
    import assoc_cases
    from assoc_compare import compare_tables
    from test_assoc_cli import run_cli
    from trtools_amd import runtime
    runtime.set_compute(None)
    traits = np.random.default_rng(5).normal(size=(50, 5))
    names = ['ya', 'yb', 'yc']
    kw = dict(same_samples=True, tr_vcf=assoc_cases.HIPSTR, non_major_cutoff=3)
    np.save(str(tmp_path / 'all.npy'), traits)
    out = str(tmp_path / 'multi.tsv')
    run_cli(out, dict(kw, traits=[str(tmp_path / 'all.npy')], phenotype_name=','.join(names), n_outcomes=3), 10, 15)
    for t, name in enumerate(names):
        np.save(str(tmp_path / (name + '.npy')), traits[:, [t, 3, 4]])
        one = str(tmp_path / (name + '.tsv'))
        run_cli(one, dict(kw, traits=[str(tmp_path / (name + '.npy'))], phenotype_name=name), 10, 15)
        assert compare_tables(out + '.' + name, one, rtol=1e-9) > 50
    with pytest.raises(ValueError):
        run_cli(out, dict(kw, traits=[str(tmp_path / 'all.npy')], phenotype_name='ya,yb', n_outcomes=2,
                          beagle_dosages=True), 10, 15)
