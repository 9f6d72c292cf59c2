"""trk_mosaic_fit against tests/mosaic_ref.py, the plain float64 restatement of its definition.  The seeds are those at
which mosaic_ref and a numpy.longdouble run of itself agree on every C and on f to 1e-10."""
import functools

import numpy as np
import pytest

import mosaic_ref as ref

pytestmark = pytest.mark.gpu

SKIPPED = ('nocall', 'noreads', 'noA', 'noB', 'single')
FITTED = ('R2', 'R16', 'R17', 'R64', 'R65', 'span16', 'span17', 'span33', 'homo', 'exact', 'third', 'mosaic')
# name: (L, S, kinds dealt to the calls in turn, output_all, seed)
CASES = {
    'one': (1, 1, ('mosaic',), False, 1),
    'kinds': (3, 5, FITTED + ('noA', 'noB', 'single'), False, 2),
    'kinds_output_all': (3, 5, ('noA', 'noB', 'single', 'homo', 'mosaic', 'exact', 'third'), True, 3),
    'skipped': (3, 5, SKIPPED, False, 4),
    # 16 calls per workgroup of the fit and a ragged tail; most calls skipped, the compaction crosses workgroups
    'wide': (5, 67, SKIPPED * 3 + FITTED, False, 5),
    # TRK_MOSAIC_BAD between fitted calls: values not strictly ascending, a count of 0, 4097 candidates, a slice of the
    # read arrays that ends before it starts, one that ends past the arrays
    'bad': (2, 4, ('mosaic', 'bad_desc', 'bad_same', 'bad_count', 'bad_span', 'mosaic', 'bad_back', 'bad_past'), False, 6),
}


def make_call(kind, rng):
    """(A, B, read values ascending, counts) of one call of a kind."""
    base = int(rng.integers(-20, 20))
    if kind in ('nocall', 'noreads'):
        return (None, None, [0, 2], [5, 5]) if kind == 'nocall' else (base, base + 2, [], [])
    if kind[0] == 'R' or kind.startswith('span'):
        n = int(kind[1:]) if kind[0] == 'R' else int(rng.integers(3, 6))
        width = n + int(rng.integers(0, 4)) if kind[0] == 'R' else int(kind[4:]) - 6   # candidates = max - min + 7
        inner = 1 + rng.choice(width - 2, n - 2, replace=False) if n > 2 else []
        vals = np.sort(np.concatenate([[0, width - 1], inner])).astype(np.int64) + base
        cnts = rng.integers(1, 4, n)
        ia, ib = sorted(rng.choice(n, 2, replace=False))
        cnts[ia] += int(rng.integers(10, 30))
        cnts[ib] += int(rng.integers(10, 30))
        if rng.random() < 0.5:   # a third allele with support
            cnts[int(rng.integers(0, n))] += int(rng.integers(3, 12))
        return int(vals[ia]), int(vals[ib]), vals.tolist(), cnts.tolist()
    if kind.startswith('bad'):
        return (1, 3) + {'bad_desc': ([3, 1], [5, 5]), 'bad_same': ([1, 1], [5, 5]), 'bad_count': ([1, 3], [5, 0]),
                         'bad_span': ([1, 4091], [5, 5])}.get(kind, ([1, 3], [5, 5]))
    A, B = base, base + int(rng.integers(1, 5))
    n_a, n_b = int(rng.integers(10, 30)), int(rng.integers(10, 30))
    if kind == 'homo':
        return A, A, [A - 1, A, A + 2], [2, n_a + n_b, int(rng.integers(1, 9))]
    if kind == 'noA':
        return A, B, [A - 1, B, B + 1], [n_a, n_b, 3]
    if kind == 'noB':
        return A, B, [A, B + 1, B + 3], [n_a, 2, n_b]
    if kind in ('single', 'exact', 'third'):
        return {'single': (A, A, [A], [n_a]), 'exact': (A, B, [A, B], [n_a, n_a + 1]),
                'third': (A, B, [A, B, B + 3], [3, 3, 40 + n_a])}[kind]
    assert kind == 'mosaic'
    return A, B, [A - 1, A, B, B + 2], [1, n_a, n_b, int(rng.integers(3, 9))]


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The inputs of a case and mosaic_ref's results, computed once."""
    L, S, kinds, output_all, seed = CASES[name]
    rng = np.random.default_rng(seed)
    stutter = np.column_stack([rng.uniform(0.01, 0.3, L), rng.uniform(0.01, 0.3, L), 0.95 - rng.uniform(0.0, 0.45, L)])
    ab = np.full((L, S, 2), -2 ** 31, dtype=np.int32)
    off, vals, cnts, want = [0], [], [], []
    for c in range(L * S):
        kind = kinds[c % len(kinds)]
        A, B, v, n = make_call(kind, rng)
        if A is not None:
            ab[c // S, c % S] = (A, B)
        vals += v
        cnts += n
        off.append(len(vals) + {'bad_back': -3, 'bad_past': 1}.get(kind, 0))
        st = 4 if kind.startswith('bad') else ref.status(A, B, v, output_all)
        want.append((st, ref.fit(v, n, A, B, ref.stutter_table(*stutter[c // S])) if st == ref.FIT else None, kind))
    arrays = (ab, np.array(off, np.int32), np.array(vals, np.int32), np.array(cnts, np.int32), stutter)
    return arrays, output_all, want


@pytest.fixture(scope='module')
def eng():
    from trtools_amd.engine import Engine
    e = Engine(0, reserve_pair_gb=0)
    yield e
    e.close()


@pytest.mark.parametrize('name', list(CASES))
def test_mosaic_fit_matches_reference(eng, name):
    arrays, output_all, want = make_case(name)
    runs = [{k: v.get() for k, v in eng.mosaic_fit(*arrays, output_all=output_all).items()} for _ in range(2)]
    got = runs[0]
    for k, v in got.items():
        assert v.tobytes() == runs[1][k].tobytes(), "a second run differs in %s" % k
    flat = {k: v.reshape(-1) for k, v in got.items()}
    # both end points of the f step are reached: f == 0 by every 'exact' call, f == 0.5 by a 'third' call of these two
    assert all(w['C'] is None and w['f'] == 0.0 for _, w, kind in want if kind == 'exact' and w)
    assert name not in ('kinds', 'wide') or any(w['f'] == 0.5 for _, w, kind in want if kind == 'third' and w)
    for c, (st, w, _) in enumerate(want):
        if w is None:
            assert flat['status'][c] == st and flat['C'][c] == 0 and flat['support'][c] == 0, c
            assert all(np.isnan(flat[k][c]) for k in ('f', 'pval', 'll_fit', 'll_null')), c
            continue
        assert flat['status'][c] == (0x10 if w['C'] is None else 0) | (0x20 if w['nonconv'] else 0), (c, w)
        assert flat['C'][c] == (0 if w['C'] is None else w['C']), (c, w)
        assert flat['support'][c] == w['support'], (c, w)
        assert abs(flat['f'][c] - w['f']) <= 1e-9, (c, w, flat['f'][c])
        for k in ('ll_fit', 'll_null', 'pval'):
            assert abs(flat[k][c] - w[k]) <= 1e-9 * abs(w[k]), (c, k, w, flat[k][c])
    assert all(w is None for _, w, _ in want) == (name == 'skipped')
