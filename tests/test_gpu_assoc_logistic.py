"""GPU parity: trk_assoc_scan_logistic (k_assoc_logit) against the np.longdouble restatement of its definition
(tests/logit_ref.py) at every locus of seeded batches.  Integers, statuses, step counts and the allele histogram exact;
floats by test_gpu_assoc.py's rule (1e-9 relative, + 1e-12 absolute on COEF / TVALUE).  Every design keeps at least six
tested samples per column."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logit_ref                                        # noqa: E402
from test_gpu_assoc import eng, make_case               # noqa: E402,F401
from trtools_amd import _lib as TL                      # noqa: E402

pytestmark = pytest.mark.gpu
FLOATS = ((TL.AF_COEF, 'coef', 1e-12), (TL.AF_SE, 'se', 0.0), (TL.AF_TVALUE, 'z', 1e-12), (TL.AF_PVAL, 'pval', 0.0),
          (TL.AF_LOGLIK, 'loglik', 0.0))
FIT_COLS = [TL.AF_PVAL, TL.AF_COEF, TL.AF_SE, TL.AF_RSQUARED, TL.AF_TVALUE, TL.AF_DF_RESID, TL.AF_LOGLIK]


def summed(gt_l, lens_l):
    lut = np.array([*lens_l, -2.0, -1.0])
    return lut[gt_l.astype(int)].sum(axis=1)


def run_case(eng, S, K, P=2, Lc=24, subset=False, locus_ploidy=False, special=False, seed=11):
    """Device against restatement on a make_case batch.  special: locus 4 fully called with covariate 1 equal to its
    summed length (collinear) and covariate K a copy of covariate 2 (dropped: rank K + 1 elsewhere); locus 5 separated
    completely by the outcome; locus 6 with every case's call missing."""
    from trtools_amd import synth
    lens, gt, lp, traits, keep = make_case(seed, Lc, S, P, K + 1, subset, locus_ploidy=locus_ploidy)
    rng = np.random.default_rng(seed + 1)
    sf = np.ones(S, dtype=bool) if keep is None else keep
    C = traits[:, 1:].copy()
    if special:
        lens[4], lens[5], lens[6] = [10.0, 12.0, 15.0], [10.0, 11.0], [10.0, 11.0, 13.0]
        gt[4] = rng.integers(0, 3, size=(S, P))
        gt[6] = rng.integers(0, 3, size=(S, P))
        C[:, 0] = summed(gt[4], lens[4])
        C[:, K - 1] = C[:, 1]
    C = (C - C[sf].mean(axis=0)) / C[sf].std(axis=0)
    g0 = summed(np.maximum(gt[0], 0), lens[0])
    eta = -0.5 + 0.3 * (g0 - g0.mean()) / g0.std() + C @ np.full(K, 0.1)
    y = (rng.random(S) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    if special:
        gt[5, :, 0], gt[5, :, 1:] = y.astype(np.int16), 0            # y == (g > median), exactly
        gt[6][y == 1] = -1                                           # only controls remain
    off, lc, sc, cv = synth.pack_alleles(lens, None)
    tables = synth.pack_assoc_tables(lens, 2)
    vec = np.vstack([y[None, :], C.T])
    batch = eng.make_batch(gt, off, lc, sc, cv, locus_ploidy=lp)
    mask = None if sf.all() else sf.astype(np.uint8)

    def device(scan=None):
        r = (scan or eng.assoc_scan_logistic)(batch, vec, *tables, sample_in=mask, non_major_cutoff=3.0)
        return r.locus_int.get(), r.locus_f64.get(), r.allele_count.get()
    lin, (li, lf, cnt), again = device(eng.assoc_scan), device(), device()
    assert li.tobytes() == again[0].tobytes() and lf.tobytes() == again[1].tobytes()      # a rerun: identical bytes
    # everything the scan decides is the linear scan's, to the bit
    same_i, same_f = [TL.AI_N_TESTED, TL.AI_N_RALLELES, TL.AI_N_BAD, TL.AI_N_HAPS], [TL.AF_GT_MEAN, TL.AF_GT_STD, TL.AF_NONMAJOR]
    assert np.array_equal(cnt, lin[2]) and np.array_equal(li[:, same_i], lin[0][:, same_i])
    assert lf[:, same_f].tobytes() == lin[1][:, same_f].tobytes()
    assert np.all(np.isnan(lf[:, TL.AF_RSQUARED]))
    statuses = {}
    for l in range(Lc):
        if lin[0][l, TL.AI_STATUS] not in (TL.AS_OK, TL.AS_COLLINEAR):                   # filtered by the scan
            assert li[l, TL.AI_STATUS] == lin[0][l, TL.AI_STATUS] and np.all(np.isnan(lf[l, FIT_COLS])), l
            continue
        g = gt[l] if lp is None else gt[l][:, :lp[l]]
        curr = sf & ~np.any(g == -1, axis=1)
        gs = summed(g[curr], lens[l])
        X = np.column_stack([np.ones(curr.sum()), C[curr], (gs - gs.mean()) / gs.std()])
        assert X.shape[0] >= 6 * X.shape[1]
        ref = logit_ref.fit(X, y[curr])
        statuses[l] = ref['status']
        assert (li[l, TL.AI_STATUS], li[l, TL.AI_RANK], li[l, TL.AI_N_ITER]) == (ref['status'], ref['rank'], ref['n_iter']), l
        assert li[l, TL.AI_N_ITER] <= 30
        if ref['status'] != logit_ref.OK:
            assert np.all(np.isnan(lf[l, FIT_COLS])), l
            continue
        assert lf[l, TL.AF_DF_RESID] == curr.sum() - ref['rank']
        for col, key, atol in FLOATS:
            assert abs(lf[l, col] - ref[key]) <= 1e-9 * abs(ref[key]) + atol, (l, key, lf[l, col], ref[key])
    return dict(statuses=statuses, rank=li[:, TL.AI_RANK], device=device, li=li, lf=lf, batch=batch, tables=tables, vec=vec)


@pytest.mark.parametrize('S,K,P,kw', [
    (48, 0, 2, {}),                                     # less than one wave step
    (257, 1, 2, dict(subset=True)),                     # ragged tail, a sample_in subset
    (1000, 5, 2, dict(special=True)),                   # several waves' shares; the constructed loci
    (1000, 13, 2, {}),                                  # the widest design
    (257, 5, 1, {}),                                    # haploid rows
    (257, 1, 3, dict(locus_ploidy=True)),               # mixed ploidy
    (20000, 5, 2, dict(Lc=6)),                          # beyond the LDS-resident rows: decoded again in every pass
])
def test_logistic_scan_against_restatement(eng, S, K, P, kw):
    r = run_case(eng, S, K, P, **kw)
    assert sum(s == logit_ref.OK for s in r['statuses'].values()) >= 2
    if kw.get('special'):
        st = r['statuses']
        assert (st[4], st[5], st[6]) == (logit_ref.COLLINEAR, logit_ref.NOT_CONVERGED, logit_ref.CONSTANT_OUTCOME)
        ok = [l for l, s in st.items() if s == logit_ref.OK]
        assert np.all(r['rank'][ok] == K + 1)           # the duplicated covariate is dropped, once
    if S == 1000 and K == 5:
        # the streaming instantiation on rows that also fit in LDS: the same bits
        from helpers import lab_env
        with lab_env(TRK_AS_LOGIT_STREAM='1'):
            li2, lf2, _ = r['device']()
        assert li2.tobytes() == r['li'].tobytes() and lf2.tobytes() == r['lf'].tobytes()


def test_limits(eng):
    r = run_case(eng, 257, 1, Lc=6)
    with pytest.raises(TL.TrkError):                    # K = 14: TRK_ERR_ARG
        eng.assoc_scan_logistic(r['batch'], np.zeros((15, 257)), *r['tables'])
    with pytest.raises(ValueError):                     # an outcome that is not 0 / 1
        eng.assoc_scan_logistic(r['batch'], r['vec'] + 0.5, *r['tables'])


def test_command_line_binary_logistic(tmp_path):
    import assoc_cases
    from test_assoc_cli import run_cli
    from trtools_amd import runtime
    from trtools_amd.utils import tr_harmonizer as trh, utils
    runtime.set_compute(None)
    traits = np.random.default_rng(5).normal(size=(50, 3))
    traits[:, 0] = traits[:, 0] > 0.2                   # the trait is a thresholded column
    np.save(str(tmp_path / 't.npy'), traits)
    kw = dict(same_samples=True, tr_vcf=assoc_cases.HIPSTR, non_major_cutoff=3, traits=[str(tmp_path / 't.npy')],
              phenotype_name='cc', binary='logistic')
    out = str(tmp_path / 'b.tsv')
    run_cli(out, kw, 10, 15)
    rows = [line.rstrip('\n').split('\t') for line in open(out)]
    assert rows.pop(0)[5:9] == ['p_cc', 'coeff_cc', 'se_cc', 'regression_R^2']
    C = (traits[:, 1:] - traits[:, 1:].mean(axis=0)) / traits[:, 1:].std(axis=0)
    reader = utils.LoadSingleReader(assoc_cases.HIPSTR, checkgz=False)
    vt, n_ok = trh.InferVCFType(reader, 'auto'), 0
    for row, rec in zip(rows, reader):
        if row[4] != 'False':
            continue
        tr = trh.HarmonizeRecord(vt, rec)
        curr = tr.GetCalledSamples()
        gs = tr.GetLengthGenotypes()[curr, :-1].sum(axis=1)
        ref = logit_ref.fit(np.column_stack([np.ones(curr.sum()), C[curr], (gs - gs.mean()) / gs.std()]), traits[curr, 0])
        want = ('%.15e' % ref['pval'], ref['coef'] / gs.std(), ref['se'] / gs.std())
        assert row[8] == 'nan' and abs(float(row[5]) - ref['pval']) <= 1e-9 * ref['pval'], (row, want)
        assert abs(float(row[6]) - want[1]) <= 1e-9 * abs(want[1]) + 1e-12 and abs(float(row[7]) - want[2]) <= 1e-9 * want[2]
        n_ok += 1
    assert n_ok > 50
    for refused in (dict(beagle_dosages=True), dict(n_outcomes=2, phenotype_name='a,b')):
        with pytest.raises(ValueError):
            run_cli(out, dict(kw, **refused), 10, 15)
