"""trk_compare (compareSTR's concordance pass, include/trk.h) on the device against a plain numpy restatement of
trtools/compareSTR/compareSTR.py:550-693, one locus at a time, float64 sums by math.fsum."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGES = {'DP': np.arange(0, 51, 5).astype(np.float64), 'Q': np.arange(0, 1.05, 0.1)}
BIG = 5     # the locus of a 'big' batch whose alleles do not fit the LDS table


def random_pair(rng, L, S, P, thirds=False, big=False):
    """Two call sets over shared samples: joint ids with duplicates across the two tables, missing and half-missing
    calls, haploid samples inside the records (equal on both sides), swapped haplotypes."""
    sides = []
    step = 1.0 / 3.0 if thirds else 0.25
    for k in range(2):
        nA = rng.integers(1, 7, size=L)
        if big:
            nA[BIG] = 1500
        off = np.concatenate([[0], np.cumsum(nA)]).astype(np.int32)
        val = np.concatenate([(np.arange(n) + rng.integers(0, 2)) % max(n, 3) if n < 100 else rng.permutation(n) for n in nA])
        sides.append(dict(allele_off=off, seq_id=val.astype(np.uint16), len_id=(val // 2).astype(np.uint16),
                          dlen=((val // 2) % 200 - 100) * step, nA=nA))
    g1 = rng.integers(0, 6, size=(L, S, P)) % sides[0]['nA'][:, None, None]
    g2 = np.where(rng.random((L, S, P)) < 0.8, g1, rng.integers(0, 6, size=(L, S, P))) % sides[1]['nA'][:, None, None]
    if big:
        g1[BIG] = rng.integers(0, 1500, size=(S, P))
        g2[BIG] = np.where(rng.random((S, P)) < 0.5, g1[BIG], rng.integers(0, 1500, size=(S, P)))
    swap = rng.random((L, S)) < 0.3
    g2[swap] = g2[swap][:, ::-1]
    for g in (g1, g2):
        g[rng.random((L, S, P)) < 0.05] = -1
        g[rng.random((L, S)) < 0.05] = -1
    if P > 1:
        hap = rng.random((L, S)) < 0.04
        g1[hap, -1] = -2
        g2[hap, -1] = -2
    sides[0]['gt'], sides[1]['gt'] = g1.astype(np.int16), g2.astype(np.int16)
    ordered = rng.random(L) < 0.5        # ordered loci: every sample phased on one side at least
    for k in range(2):
        ph = (rng.random((L, S)) < 0.5) & ordered[:, None]
        sides[k]['phased'] = (ph | (ordered[:, None] & (k == 1))).astype(np.uint8)
    dp = [rng.integers(-3, 56, size=(L, S)).astype(np.int32) for _ in range(2)]
    q = [rng.choice(np.concatenate([EDGES['Q'].astype(np.float32), rng.random(20).astype(np.float32), [np.nan]]),
                    size=(L, S)).astype(np.float32) for _ in range(2)]
    for p in dp:
        p[rng.random((L, S)) < 0.05] = -2 ** 31
    return sides, -2.0 - rng.integers(4, 40, size=L) * step, dp, q, rng.integers(0, 3, size=L).astype(np.uint8)


def in_bin(v, e, i):
    return (v >= e[i]) & ((v <= e[i + 1]) if i + 2 == len(e) else (v < e[i + 1]))


def restate(sides, dabs, phase, fields, slot, n_slots):
    g = [sd['gt'].astype(np.int64) for sd in sides]
    L, S, P = g[0].shape
    nb = 1 + sum(len(f['edges']) - 1 for f in fields)
    li, terms = np.zeros((L, 4), np.int64), [[[] for _ in range(5)] for _ in range(L)]
    si, bi = np.zeros((3, S), np.int64), np.zeros((n_slots, nb, 3), np.int64)
    bterms = {}
    for l in range(L):
        called = ~np.any(g[0][l] == -1, axis=1) & ~np.any(g[1][l] == -1, axis=1)
        if not called.any():
            continue
        if np.any(np.sum(g[0][l] == -2, axis=1)[called] != np.sum(g[1][l] == -2, axis=1)[called]):
            li[l, 3] |= 1
        all_un = True
        if phase:
            un = ((sides[0]['phased'][l] == 0) & (sides[1]['phased'][l] == 0))[called]
            all_un = bool(np.all(un))
            if not (all_un or np.all(~un)):
                li[l, 3] |= 2
                all_un = True
        ids, xs = [], []
        for k, sd in enumerate(sides):
            o, gl = sd['allele_off'][l], g[k][l]
            if np.any((gl >= sd['nA'][l])[called]):
                li[l, 3] |= 4
            at = o + np.clip(gl, 0, sd['nA'][l] - 1)
            ids.append([np.where(gl == -2, 0xffff, sd[n][at]) for n in ('seq_id', 'len_id')])
            xs.append(np.where(gl == -2, dabs[l], sd['dlen'][at]).sum(axis=1))
        if all_un:
            ids = [[np.sort(a, axis=1) for a in pair] for pair in ids]
        conc = [np.all(ids[0][n] == ids[1][n], axis=1) & called for n in range(2)]
        li[l, :3] = called.sum(), conc[0].sum(), conc[1].sum()
        si += np.stack([called, conc[0], conc[1]])
        x, y = xs
        mom = [x, y, x * x, x * y, y * y]
        masks = [called]
        for f in fields:
            e = f['edges'].astype(np.float32) if f['planes'][0].dtype == np.float32 else f['edges']
            v = [p[l] if p.dtype == np.float32 else p[l].astype(np.float64) for p in f['planes']]
            for i in range(len(e) - 1):
                m = [in_bin(v[k], e, i) for k in range(2)]
                masks.append(called & (m[0] & m[1] if f['stratify_file'] == 0 else m[f['stratify_file'] - 1]))
        for b, m in enumerate(masks):
            bi[slot[l], b] += m.sum(), (conc[0] & m).sum(), (conc[1] & m).sum()
            for k in range(5):
                bterms.setdefault((slot[l], b, k), []).extend(mom[k][m])
        for k in range(5):
            terms[l][k] = list(mom[k][called])
    return li, terms, si, bi, bterms


def check_sums(got, terms, exact):
    """exact: every partial sum is representable (multiples of 1/16 far below 2^53), order cannot matter -- bit-equal;
    else the bound for reordering n float64 terms, n * 2^-52 * sum |t_i|."""
    want = math.fsum(terms)
    if exact:
        assert got == want
    else:
        assert abs(got - want) <= len(terms) * 2.0 ** -52 * math.fsum(abs(t) for t in terms)


def run_case(L, S, P, mode, thirds=False, big=False, pad=True):
    from trtools_amd.engine import Engine
    rng = np.random.default_rng(L * 1000 + S + 7 * len(mode))
    sides, dabs, dp, q, slot = random_pair(rng, L, S, P, thirds, big)
    phase = mode == 'phased'
    if mode not in ('phased', 'ignore'):
        for sd in sides:
            sd.pop('phased')
    fields = []
    if mode.startswith('strat'):
        sf = int(mode[-1])
        fields = [dict(planes=dp, edges=EDGES['DP'], stratify_file=sf), dict(planes=q, edges=EDGES['Q'], stratify_file=sf)]
    n_slots = 3 if mode in ('slots', 'strat0') else 1
    if n_slots == 1:
        slot = np.zeros(L, np.uint8)
    eng = Engine(0)
    res = eng.compare_calls(sides, dabs, slot=slot if n_slots > 1 else None, n_slots=n_slots, fields=fields,
                            ignore_phasing=mode == 'ignore', pad=pad)
    got = {k: v.get() for k, v in res.items()}
    eng.close()
    li, terms, si, bi, bterms = restate(sides, dabs, phase, fields, slot, n_slots)
    assert np.array_equal(got['locus_int'], li)
    assert np.array_equal(got['sample_int'], si)
    assert np.array_equal(got['bin_int'], bi)
    for l in range(L):
        for k in range(5):
            check_sums(got['locus_f64'][l, k], terms[l][k], not thirds)
    for s in range(n_slots):
        for b in range(bi.shape[1]):
            for k in range(5):
                check_sums(got['bin_f64'][s, b, k], bterms.get((s, b, k), []), not thirds)
    return got


@pytest.mark.parametrize('L,S,P', [(37, 64, 2), (300, 1030, 2), (129, 203, 2), (50, 77, 1), (40, 90, 3)])
@pytest.mark.parametrize('mode', ['plain', 'phased', 'ignore', 'strat0', 'strat1', 'strat2', 'slots'])
def test_device_equals_restatement(L, S, P, mode):
    run_case(L, S, P, mode)


@pytest.mark.parametrize('L,S,P,kw', [(37, 64, 2, dict(thirds=True)), (129, 203, 2, dict(pad=False)),
                                      (37, 64, 2, dict(big=True)), (40, 90, 3, dict(thirds=True))])
def test_thirds_unpadded_rows_and_oversized_allele_table(L, S, P, kw):
    run_case(L, S, P, 'strat0', **kw)


@pytest.fixture(scope='module')
def flagged():
    """One batch with a planted locus per flag, run twice."""
    from trtools_amd.engine import Engine
    rng = np.random.default_rng(11)
    sides, dabs, _, _, _ = random_pair(rng, 60, 520, 2)
    for sd in sides:
        sd['gt'][[7, 33]] = 0                                   # every sample called, diploid, allele 0
        sd['phased'][[7, 33]] = 0
    sides[1]['gt'][7, 515, 1] = -2                              # ploidy 2 against 1
    sides[0]['phased'][33, 3] = 1                               # one phased sample among unphased ones
    sides[0]['gt'][40, 100] = 9                                 # an allele index the record does not have
    sides[1]['gt'][40, 100] = 0
    eng = Engine(0)
    runs = [{k: v.get() for k, v in eng.compare_calls(sides, dabs).items()} for _ in range(2)]
    eng.close()
    return runs


@pytest.mark.parametrize('locus,bit,exc,text', [
    (7, 1, ValueError, r"Found sample\(s\) of different ploidy at chr1:70"),
    (33, 2, ValueError, r"Found sample\(s\) with different phasedness at chr1:330"),
    (40, 4, IndexError, r"chr1:400")])
def test_flag_marks_its_locus_and_the_host_raises(flagged, locus, bit, exc, text):
    from trtools_amd.compareSTR.compareSTR import raise_for_flags
    fl = flagged[0]['locus_int'][:, 3]
    assert fl[locus] & bit and not np.any(np.delete(fl, locus) & bit)
    chroms, pos = ['chr1'] * 60, np.arange(60) * 10
    with pytest.raises(exc, match=text):            # the first flagged locus from `locus` on
        raise_for_flags(flagged[0]['locus_int'][locus:], chroms[locus:], pos[locus:])


def test_rerun_is_bit_identical(flagged):
    for k in flagged[0]:
        assert flagged[0][k].tobytes() == flagged[1][k].tobytes(), k


def test_slot_outside_the_slots_is_rejected():
    from trtools_amd.engine import Engine
    sides, dabs, _, _, _ = random_pair(np.random.default_rng(3), 8, 16, 2)
    eng = Engine(0)
    with pytest.raises(ValueError, match="n_slots"):
        eng.compare_calls(sides, dabs, slot=np.full(8, 3, np.uint8), n_slots=3)
    eng.close()
