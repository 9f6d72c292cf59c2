"""trtools_amd.compareSTR.compareSTR.main against the tables the real reference writes for the same arguments
(tests/golden/compare/, tools/gen_golden_compare.py): integer columns and strings exact, float columns within 1e-9
(the project's bound for float statistics), nan equal to nan.  The pass runs on the device: there is no CPU fallback."""
import argparse
import json
import math
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden', 'compare')
DATA = os.path.join(HERE, 'golden', 'data', 'compareSTR')
CASES = json.load(open(os.path.join(GOLD, 'cases.json')))['cases']
DEFAULTS = dict(samples=None, region=None, stratify_fields=None, stratify_binsizes=None, stratify_file=0, period=False,
                bubble_min=None, bubble_max=None, verbose=False, numrecords=None, noplot=True, vcftype1='auto',
                vcftype2='auto', ignore_phasing=False)


def same_token(a, b):
    if a == b:
        return True
    try:
        int(a), int(b)
        return False                      # two different integers
    except ValueError:
        pass
    try:
        x, y = float(a), float(b)
    except ValueError:
        return False
    return (math.isnan(x) and math.isnan(y)) or abs(x - y) <= 1e-9


def assert_same_table(got_path, want_path):
    got, want = open(got_path).read().splitlines(), open(want_path).read().splitlines()
    assert len(got) == len(want), (got_path, len(got), len(want))
    for n, (g, w) in enumerate(zip(got, want)):
        gt, wt = g.split('\t'), w.split('\t')
        assert len(gt) == len(wt) and all(same_token(a, b) for a, b in zip(gt, wt)), (got_path, n, g, w)


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_main_writes_the_reference_tables(case, tmp_path, capsys):
    from trtools_amd.compareSTR.compareSTR import main
    kw = dict(DEFAULTS, **case['args'])
    if kw['samples']:
        kw['samples'] = os.path.join(DATA, kw['samples'])
    out = str(tmp_path / case['name'])
    rc = main(argparse.Namespace(vcf1=os.path.join(DATA, case['vcf1']), vcf2=os.path.join(DATA, case['vcf2']), out=out, **kw))
    assert rc == case['rc']
    assert capsys.readouterr().err == case['stderr']        # the reference's warnings, word for word
    for tab in ('-overall.tab', '-locuscompare.tab', '-samplecompare.tab'):
        if case['rc'] == 0:
            assert_same_table(out + tab, os.path.join(GOLD, case['name'] + tab))
        else:
            assert not os.path.exists(out + tab)
