#!/usr/bin/env python3
"""Record the tables the REAL reference's compareSTR writes (build container only).

    python tools/gen_golden_compare.py     # rewrites tests/golden/compare/ and tests/golden/data/compareSTR/

Imports the reference (cyvcf2 through tools/refshim), runs ``compareSTR.main`` with --noplot on the reference's own
test VCFs for every argument set of CASES and keeps the three tables (<case>-overall.tab, -locuscompare.tab,
-samplecompare.tab), the return code and the warnings in tests/golden/compare/; the input VCFs with their indexes
and the sample list are copied to tests/golden/data/compareSTR/ as fixtures.
"""
import argparse
import contextlib
import io
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, 'refshim'))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, 'tests', 'golden', 'compare')
DATA = os.path.join(REPO, 'tests', 'golden', 'data', 'compareSTR')
VCFS = '/root/reference/trtools/testsupport/sample_vcfs/compareSTR_vcfs'
G1, G2 = 'test_gangstr1.vcf.gz', 'test_gangstr2.vcf.gz'
STRAT = dict(stratify_fields='DP,Q', stratify_binsizes='0:50:5,0:1:0.1')

# name, vcf1, vcf2, arguments that differ from the defaults
CASES = [
    ('plain', G1, G2, {}),
    ('period', G1, G2, dict(period=True)),
    ('strat0', G1, G2, dict(stratify_file=0, **STRAT)),
    ('strat1', G1, G2, dict(stratify_file=1, **STRAT)),
    ('strat2', G1, G2, dict(stratify_file=2, **STRAT)),
    ('strat0_period', G1, G2, dict(stratify_file=0, period=True, **STRAT)),
    ('samples', G1, G2, dict(samples='sample_list.txt')),
    ('region', G1, G2, dict(region='chr1:3045469-3052474')),
    ('ignore_phasing', G1, G2, dict(ignore_phasing=True)),
    ('better_comparability', 'test_better_comparability_calculation_1.vcf.gz',
     'test_better_comparability_calculation_2.vcf.gz', {}),
    ('no_comparable', 'test_no_comparable_records_1.vcf.gz', 'test_no_comparable_records_2.vcf.gz', {}),
]
DEFAULTS = dict(samples=None, region=None, stratify_fields=None, stratify_binsizes=None, stratify_file=0, period=False,
                bubble_min=None, bubble_max=None, verbose=False, numrecords=None, noplot=True, vcftype1='auto',
                vcftype2='auto', ignore_phasing=False)


def main():
    sys.path.insert(0, '/root/reference')
    import trtools.compareSTR.compareSTR as rc     # the reference
    for d in (OUT, DATA):
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
    cases = []
    for name, v1, v2, extra in CASES:
        for f in [v1, v1 + '.tbi', v2, v2 + '.tbi'] + ([extra['samples']] if extra.get('samples') else []):
            shutil.copy(os.path.join(VCFS, f), os.path.join(DATA, f))
            os.chmod(os.path.join(DATA, f), 0o644)
        kw = dict(DEFAULTS, **extra)
        if kw['samples']:
            kw['samples'] = os.path.join(VCFS, kw['samples'])
        args = argparse.Namespace(vcf1=os.path.join(VCFS, v1), vcf2=os.path.join(VCFS, v2), out=os.path.join(OUT, name), **kw)
        err = io.StringIO()
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(err):
            code = int(rc.main(args))
        cases.append(dict(name=name, vcf1=v1, vcf2=v2, args=extra, rc=code, stderr=err.getvalue()))
        print('%-22s rc=%d' % (name, code))
    with open(os.path.join(OUT, 'cases.json'), 'w') as fh:
        json.dump({'generator': 'tools/gen_golden_compare.py', 'cases': cases}, fh, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
