"""trk_parse_reads (Engine.parse_reads): the read vectors and (A, B) of every call parsed on the device, against
prancSTR.ExtractReadVector + read_counts on the same strings and Python's // on the same integers -- equality, no
tolerance -- and prancSTR.mosaic_fit_vcf against mosaic_fit_records on the same file."""
import os

import numpy as np
import pytest

from test_gpu_mosaic import eng   # noqa: F401 (the module's engine fixture)
from trtools_amd import _lib as L
from trtools_amd import prancSTR

pytestmark = pytest.mark.gpu

E = L.READS_MAX_ENTRIES
VCF = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data', 'statSTR', 'test_longtr.vcf')
# spellings of the read field dealt round-robin over the calls; None: the token ends before the field
SPELL = ['-1|2;-3|1;-4|5;7|1', '4|1;5|2;6|3;3|1', '9|1;3|2;-6|4', '2|0;8|3;8|0', '.', '', None, '3|2;x;5|1', '12|3;',
         ';'.join('%d|1' % (5 * i - 150) for i in range(E)), '-999999999|1000;999999999|1']
FILL = ';'.join('%d|%d' % (i - 40, i) for i in range(80))[:400]          # a 400-byte ALLREADS
# how a token is laid out around the field: (FORMAT keys before it, keys after it)
LAYOUT = {'last': (['0|1', '17'], []), 'first': ([], ['0|1', '17']), 'behind': (['0|1', FILL], ['0.5']),
          'mid': (['0|1', 'x' * 100], ['9'])}
BAD = {'pipes': ('1|2|3', L.PARSE_HOST), 'plus': ('+3|1', L.PARSE_HOST), 'digits': ('1234567890|1', L.PARSE_HOST),
       'entries': (';'.join('%d|1' % i for i in range(E + 1)), L.PARSE_HOST), 'column': (None, L.PARSE_COLUMNS)}
# name: [(samples, period, layout, read field present, bad spelling or None)] per record
CASES = {'one': [(1, 2, 'last', True, None)],
         'ragged': [(67, 1, 'last', True, None), (67, 3, 'first', True, None), (67, 4, 'behind', True, None)],
         'straddle': [(300, 3, 'mid', True, None)],
         'absent': [(5, 2, 'last', False, None), (5, 3, 'first', True, None)]}
CASES.update({k: [(5, 3, 'last', True, None), (5, 3, 'last', True, k), (5, 2, 'first', True, None)] for k in BAD})
GT = [(0, 1), (2, 0), (-1, 1), (1, -2), (3, 0), (1, 1), (0, -1)]
ALLELE_BP = [0, -7, 5]


def build(name):
    """The text of the case, the inputs of parse_reads and the expected arrays."""
    text, smp_off, line_end, ridx, period, flags, vals, cnts, off, ab, gt = '', [], [], [], [], [], [], [], [0], [], []
    for l, (ns, per, layout, present, bad) in enumerate(CASES[name]):
        before, after = LAYOUT[layout]
        fields = [SPELL[(l * 3 + s) % len(SPELL)] for s in range(ns)]
        if bad is not None and BAD[bad][0] is not None:
            fields[2] = BAD[bad][0]
        if not before:
            fields = ['' if f is None else f for f in fields]            # (no token ends before its first subfield)
        tokens = [':'.join(before if f is None else before + [f] + after) for f in fields]
        if bad == 'column':
            tokens = tokens[:-1]
        text += 'chr1\t%d\t.\tA\t.\t.\t.\tX\tFMT\t' % (100 * l + 1)
        smp_off.append(len(text))
        text += '\t'.join(tokens)
        line_end.append(len(text))
        text += '\n'
        ridx.append(len(before) if present else -1)
        period.append(per)
        flags.append(BAD[bad][1] if bad is not None else 0)
        for s, f in enumerate(fields):
            g = GT[(l + s) % len(GT)]
            gt.append(g)
            called = not flags[-1] and all(0 <= x < len(ALLELE_BP) for x in g)
            ab.append([ALLELE_BP[x] // per for x in g] if called else [L.MOSAIC_NOCALL_AB] * 2)
            v, c = prancSTR.read_counts(prancSTR.ExtractReadVector(f if present and not flags[-1] else None, per))
            vals.append(v)
            cnts.append(c)
            off.append(off[-1] + v.size)
    ns = CASES[name][0][0]
    nl = len(CASES[name])
    inputs = dict(text=text.encode(), smp_off=np.array(smp_off), line_end=np.array(line_end), n_samples=ns,
                  read_idx=np.array(ridx, np.int8), period=np.array(period, np.int32),
                  gt=np.array(gt, np.int16).reshape(nl, ns, 2), allele_off=np.arange(nl + 1, dtype=np.int32) * len(ALLELE_BP),
                  allele_bp=np.array(ALLELE_BP * nl, np.int32))
    want = dict(flags=np.array(flags, np.uint8), read_off=np.array(off, np.int32), read_val=np.concatenate(vals),
                read_cnt=np.concatenate(cnts), ab=np.array(ab, np.int32).reshape(nl, ns, 2))
    return inputs, want


def run(eng, inputs):
    res = eng.parse_reads(**inputs)
    got = {k: None if v is None else v.get() for k, v in res.items()}
    for v in res.values():
        if v is not None:
            v.free()
    return got


@pytest.mark.parametrize('name', list(CASES))
def test_parse_reads_matches_host(eng, name):
    inputs, want = build(name)
    got = run(eng, inputs)
    for k in ('flags', 'read_off', 'read_val', 'read_cnt', 'ab'):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (name, k, got[k], want[k])
    again = run(eng, inputs)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)
    if name == 'ragged':
        assert (inputs['smp_off'] % 16 != 0).any()
    if name == 'straddle':
        assert inputs['line_end'][0] - inputs['smp_off'][0] > 2 * 16384
    if name == 'absent':
        assert want['flags'][0] == 0 and not want['read_off'][:inputs['n_samples'] + 1].any()


def test_parse_reads_without_genotypes(eng):
    inputs, want = build('ragged')
    got = run(eng, {k: v for k, v in inputs.items() if k not in ('gt', 'allele_off', 'allele_bp')})
    assert got.pop('ab') is None and all(np.array_equal(got[k], want[k]) for k in got)


@pytest.mark.parametrize('output_all', [False, True])
def test_mosaic_fit_vcf_matches_records(eng, output_all):
    import trtools_amd.utils.tr_harmonizer as trh
    from trtools_amd import vcfio
    recs = [trh.HarmonizeRecord(trh.VcfTypes.hipstr, v) for v in vcfio.VCFReader(VCF)]
    want = prancSTR.mosaic_fit_records(recs, output_all=output_all, engine=eng)
    parts = list(prancSTR.mosaic_fit_vcf(VCF, output_all=output_all, batch_records=25, engine=eng))
    assert [p['ab'].shape[0] for p in parts] == [25, 25, 17]
    assert sum((p['chrom'] for p in parts), []) == [r.chrom for r in recs]
    assert np.concatenate([p['pos'] for p in parts]).tolist() == [r.pos for r in recs]
    for k in ('ab', 'stutter', 'status', 'C', 'support', 'f', 'pval', 'll_fit', 'll_null', 'read_val', 'read_cnt'):
        got = np.concatenate([p[k] for p in parts])
        assert got.dtype == want[k].dtype and got.tobytes() == want[k].tobytes(), k
    per_call = np.concatenate([np.diff(p['read_off']) for p in parts])
    assert np.array_equal(per_call, np.diff(want['read_off']))
