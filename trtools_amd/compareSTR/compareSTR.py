"""compareSTR's host layer over the device pass (Engine.compare_calls / trk_compare, include/trk.h).

The per-record body of the reference (trtools/compareSTR/compareSTR.py:508-693) runs on the device for a batch of
matched record pairs.  This module holds what stays on the host around it: the JOINT allele tables of a pair
(``joint_tables`` / ``pack_pairs``), the reference's errors for flagged loci (``raise_for_flags``), the overall rows
with r^2 from the accumulators (``overall_rows``, ``CalcR2``) and the checks of ``--region`` (``check_region``).
``main`` is the command line: it walks the two sorted files, pairs comparable records (the reference's mergeutils walk
restated: chromosome order from the first file's contigs, the smaller position advances, ``handle_overlaps`` decides
comparability), collects the pairs into batches, runs one ``compare_calls`` per batch and writes the reference's three
tables from the accumulators.  The bubble histogram and the plots are not built.
"""
import argparse
import os
import sys

import numpy as np

from .. import _lib as L
from ..utils import common
from ..utils import tr_harmonizer as trh
from ..utils import utils

MOMENTS = ('total_len_1', 'total_len_2', 'total_len_11', 'total_len_12', 'total_len_22')


def NewOverallFormatBin():
    """The running totals of one (period, FORMAT bin) cell (reference :430-453)."""
    out = {'conc_seq_count': 0, 'conc_len_count': 0, 'numcalls': 0}
    out.update((k, 0) for k in MOMENTS)
    return out


def CalcR2(format_bin_results):
    """Squared Pearson correlation of the two length sums of a cell, from its moment sums (reference :456-485):
    nan when either side has no variance."""
    f = format_bin_results
    n = f['numcalls']
    mean1, mean2 = f['total_len_1'] / n, f['total_len_2'] / n
    var1 = f['total_len_11'] / n - mean1 ** 2
    var2 = f['total_len_22'] / n - mean2 ** 2
    if var1 == 0 or var2 == 0:
        return np.nan
    covar = f['total_len_12'] / n - f['total_len_1'] * f['total_len_2'] / n ** 2
    return covar ** 2 / (var1 * var2)


def check_region(contigs1, contigs2, region_str):
    """1 (with the reference's warning, :696-742) unless ``region_str`` is ``contig`` or ``contig:range`` with a contig
    of both files and a range of the form 42, -42, 42- or 13-42 with end > start."""
    contig, sep, rng = region_str.partition(':')
    if sep and ':' in rng:
        common.WARNING("--region should have the format contig:range")
        return 1
    if contig not in contigs1 or contig not in contigs2:
        common.WARNING("contig {} was not found in both input vcfs".format(contig))
        return 1
    if not sep:
        return 0
    ends = rng.split('-')
    ok = len(ends) in (1, 2) and any(ends) and all(e == '' or e.lstrip('+').isdigit() for e in ends) \
        and (len(ends) == 2 or ends[0] != '')
    if not ok:
        common.WARNING("The range portion of --region should have one of the forms: 42, -42, 42- or 13-42")
        return 1
    if len(ends) == 2 and ends[0] and ends[1] and int(ends[1]) <= int(ends[0]):
        common.WARNING("Cannot have range portion of --region start-end where end <= start")
        return 1
    return 0


def joint_tables(seqs1, lens1, seqs2, lens2, reflen):
    """The joint tables of one record pair.  ``seqs*``: the alleles' sequences (reference allele first, as
    GetStringGenotypes would print them), ``lens*``: their lengths in repeat units, ``reflen``:
    len(record1.ref_allele) / len(record1.motif).  Returns per side (seq_id, len_id, dlen): two ids are equal exactly
    when the sequences / lengths are, whichever side they come from."""
    seq_of, len_of = {}, {}
    out = []
    for seqs, lens in ((seqs1, lens1), (seqs2, lens2)):
        sid = np.array([seq_of.setdefault(s, len(seq_of)) for s in seqs], dtype=np.int64)
        lid = np.array([len_of.setdefault(float(x), len(len_of)) for x in lens], dtype=np.int64)
        if max(len(seq_of), len(len_of)) >= 0xfffe:
            raise ValueError("too many distinct alleles in one record pair")
        out.append((sid.astype(np.uint16), lid.astype(np.uint16), np.asarray(lens, dtype=np.float64) - reflen))
    return out


def pack_pairs(pairs):
    """``pairs``: per matched record pair (seqs1, lens1, seqs2, lens2, reflen).  Returns the two sides' table dicts
    (allele_off, seq_id, len_id, dlen) of Engine.compare_calls and dlen_absent -- what synth.pack_alleles is to one
    file's batch."""
    cols = [dict(allele_off=[0], seq_id=[], len_id=[], dlen=[]) for _ in range(2)]
    absent = []
    for seqs1, lens1, seqs2, lens2, reflen in pairs:
        for side, (sid, lid, dl) in zip(cols, joint_tables(seqs1, lens1, seqs2, lens2, reflen)):
            side['allele_off'].append(side['allele_off'][-1] + len(sid))
            side['seq_id'].append(sid)
            side['len_id'].append(lid)
            side['dlen'].append(dl)
        absent.append(-2.0 - reflen)        # GetLengthGenotypes leaves -2 in place (tr_harmonizer.py:1239)
    sides = [dict(allele_off=np.asarray(c['allele_off'], dtype=np.int32),
                  seq_id=np.concatenate(c['seq_id'] or [np.zeros(0, np.uint16)]),
                  len_id=np.concatenate(c['len_id'] or [np.zeros(0, np.uint16)]),
                  dlen=np.concatenate(c['dlen'] or [np.zeros(0)])) for c in cols]
    return sides, np.asarray(absent, dtype=np.float64)


def raise_for_flags(locus_int, chroms, positions):
    """The reference's errors (:572, :584) for the first flagged locus in file order.  An allele index outside the
    record's alleles is an IndexError as in the reference, where numpy raises it from inside GetStringGenotypes with a
    text of its own (there is none of the reference's to keep)."""
    for l in np.flatnonzero(locus_int[:, L.CMP_FLAGS]):
        fl = int(locus_int[l, L.CMP_FLAGS])
        if fl & L.CMP_F_BAD:
            raise IndexError("allele index out of range at %s:%s" % (chroms[l], positions[l]))
        if fl & L.CMP_F_PLOIDY:
            raise ValueError("Found sample(s) of different ploidy at %s:%s" % (chroms[l], positions[l]))
        raise ValueError("Found sample(s) with different phasedness at %s:%s" % (chroms[l], positions[l]))


def overall_rows(bin_int, bin_f64, periods=None):
    """The cells of the overall table from the accumulators of a run: a list of (period, bin index, cell) with
    cell = NewOverallFormatBin filled in plus 'r2'; bin 0 is the unstratified row; the 'ALL' period (the sum over
    slots, reference :632-640) comes first; cells without calls are left out."""
    bin_int, bin_f64 = np.asarray(bin_int), np.asarray(bin_f64)
    names = ['ALL'] + list(periods if periods is not None else range(bin_int.shape[0]))
    ints = np.concatenate([bin_int.sum(axis=0, keepdims=True), bin_int])
    f64s = np.concatenate([bin_f64.sum(axis=0, keepdims=True), bin_f64])
    rows = []
    for p, name in enumerate(names):
        for b in range(ints.shape[1]):
            if ints[p, b, 0] == 0:
                continue
            cell = NewOverallFormatBin()
            cell['numcalls'], cell['conc_seq_count'], cell['conc_len_count'] = (int(x) for x in ints[p, b])
            cell.update(zip(MOMENTS, (float(x) for x in f64s[p, b])))
            cell['r2'] = CalcR2(cell)
            rows.append((name, b, cell))
    return rows


def NewOverallPeriod(format_fields, format_bins):
    """The cells of one period: 'ALL' and one per bin start of every FORMAT field (reference :488-505)."""
    out = {'ALL': NewOverallFormatBin()}
    for fmt, bins in zip(format_fields, format_bins):
        out[fmt] = {start: NewOverallFormatBin() for start in bins[:-1]}
    return out


def GetFormatFields(format_fields, format_binsizes, format_fileoption, vcfreaders):
    """The FORMAT fields to stratify on and their bin edges (reference :35-93): ``min:max:step`` per field gives
    arange(min, max, step) + [max]; a field missing from a file that ``format_fileoption`` reads is a ValueError."""
    if format_fields is None or format_binsizes is None:
        return [], []
    declared = [[h['ID'] for h in vcf.header_iter() if h['HeaderType'] == 'FORMAT'] for vcf in vcfreaders]
    formats, sizes = format_fields.split(","), format_binsizes.split(",")
    if len(formats) != len(sizes):
        raise ValueError("--stratify-formats must be same length as --stratify-binsizes")
    bins = []
    for item in sizes:
        start, stop, step = (float(x) for x in item.split(":"))
        bins.append(np.arange(start, stop, step).tolist() + [stop])
    for fmt in formats:
        in1, in2 = fmt in declared[0], fmt in declared[1]
        if format_fileoption == 0 and not (in1 and in2):
            raise ValueError("FORMAT field %s must be present in both VCFs if --stratify-file=0" % fmt)
        if format_fileoption == 1 and not in1:
            raise ValueError("FORMAT field %s must be present in --vcf1 if --stratify-file=1" % fmt)
        if format_fileoption == 2 and not in2:
            raise ValueError("FORMAT field %s must be present in --vcf2 if --stratify-file=2" % fmt)
    return formats, bins


def handle_overlaps(records, chrom_indices, min_chrom_index):
    """Are the two current records comparable (reference :745-795)?  Both present, both on the chromosome that is next
    in order, and their overlap (inclusive coordinates) covers the longer reference allele entirely (min_overlap 1.0);
    records that overlap without being comparable are reported."""
    assert len(records) == 2
    if records[0] is None or records[1] is None:
        return False
    if chrom_indices[0] != min_chrom_index or chrom_indices[1] != min_chrom_index:
        return False
    left, right = records
    overlap = min(left.end_pos, right.end_pos) - max(left.pos, right.pos) + 1
    longest = max(left.ref_allele_length * len(left.motif), right.ref_allele_length * len(right.motif))
    comparable = overlap / longest >= 1.0
    if overlap >= 1 and not comparable:
        common.WARNING(f"Records {left.record_id} and {right.record_id} overlap:\n"
                       f"{left.record_id}: {left.pos, left.end_pos}\n"
                       f"{right.record_id}: {right.pos, right.end_pos},\n"
                       f"but are NOT comparable!")
    return comparable


def _write_cell(tabfile, cell, per, n_fields, fmt_idx, label):
    n = cell['numcalls']
    if n == 0:
        return
    cols = [str(per)] + [label if i == fmt_idx else 'NA' for i in range(n_fields)]
    cols += ['{}'.format(np.float64(cell['conc_seq_count']) / n), '{}'.format(np.float64(cell['conc_len_count']) / n),
             '{}'.format(CalcR2(cell)), '{}'.format(n)]
    tabfile.write('\t'.join(cols) + '\n')


def OutputOverallMetrics(overall_results, format_fields, format_bins, outprefix):
    """outprefix-overall.tab (reference :206-278): per period ('ALL' first, then ascending) the unstratified row and one
    row per non-empty FORMAT bin, the last bin printed closed."""
    periods = ['ALL'] + sorted(k for k in overall_results if k != 'ALL')
    with open(outprefix + "-overall.tab", "w") as tabfile:
        tabfile.write('\t'.join(['period'] + list(format_fields) +
                                ['concordance-seq', 'concordance-len', 'r2', 'numcalls']) + '\n')
        for per in periods:
            _write_cell(tabfile, overall_results[per]['ALL'], per, len(format_fields), None, None)
            for fmt_idx, (fmt, bins) in enumerate(zip(format_fields, format_bins)):
                for i in range(len(bins) - 1):
                    close = ']' if i == len(bins) - 2 else ')'
                    _write_cell(tabfile, overall_results[per][fmt][bins[i]], per, len(format_fields), fmt_idx,
                                "[{}, {}{}".format(bins[i], bins[i + 1], close))


def OutputLocusMetrics(locus_results, outprefix, noplot):
    """outprefix-locuscompare.tab (reference :96-123)."""
    with open(outprefix + '-locuscompare.tab', 'w') as tabfile:
        tabfile.write('chrom\tstart\tmetric-conc-seq\tmetric-conc-len\tnumcalls\n')
        for row in zip(locus_results['chrom'], locus_results['start'], locus_results['metric-conc-seq'],
                       locus_results['metric-conc-len'], locus_results['numcalls']):
            tabfile.write('{}\t{}\t{}\t{}\t{}\n'.format(*row))


def OutputSampleMetrics(sample_results, sample_names, outprefix, noplot):
    """outprefix-samplecompare.tab (reference :153-182)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        seq = sample_results['conc-seq-count'] / sample_results['numcalls']
        length = sample_results['conc-len-count'] / sample_results['numcalls']
    with open(outprefix + '-samplecompare.tab', 'w') as tabfile:
        tabfile.write('sample\tmetric-conc-seq\tmetric-conc-len\tnumcalls\n')
        for i, sample in enumerate(sample_names):
            tabfile.write('{}\t{}\t{}\t{}\n'.format(sample, seq[i], length[i], sample_results['numcalls'][i]))


def getargs():  # pragma: no cover
    parser = argparse.ArgumentParser(__doc__)
    req = parser.add_argument_group("Required arguments")
    req.add_argument("--vcf1", help="First VCF file to compare (must be sorted, bgzipped, and indexed)", type=str, required=True)
    req.add_argument("--vcf2", help="Second VCF file to compare (must be sorted, bgzipped, and indexed)", type=str, required=True)
    req.add_argument("--out", help="Prefix to name output files", type=str, required=True)
    flt = parser.add_argument_group("Filtering options")
    flt.add_argument("--samples", help="File containing list of samples to include", type=str)
    flt.add_argument("--region", help="Restrict to this region chrom:start-end", type=str)
    st = parser.add_argument_group("Metrics to stratify results")
    st.add_argument("--stratify-fields", help="Comma-separated list of FORMAT fields to stratify by", type=str)
    st.add_argument("--stratify-binsizes", help="Comma-separated list of min:max:binsize to stratify each field on. "
                    "Must be same length as --stratify-fields.", type=str)
    st.add_argument("--stratify-file", help="Set to 1 to stratify based on --vcf1. Set to 2 to stratify based on --vcf2. "
                    "Set to 0 to apply stratification to both --vcf1 and --vcf2", default=0, type=int)
    st.add_argument("--period", help="Report results overall and also stratified by repeat unit length (period)",
                    action="store_true")
    pl = parser.add_argument_group("Plotting options")
    pl.add_argument("--bubble-min", help="Minimum x/y axis value to display on bubble plots", type=int)
    pl.add_argument("--bubble-max", help="Maximum x/y axis value to display on bubble plots", type=int)
    opt = parser.add_argument_group("Optional arguments")
    opt.add_argument("--verbose", help="Print helpful debugging info", action="store_true")
    opt.add_argument("--numrecords", help="For debugging, only process this many records", type=int)
    opt.add_argument("--noplot", help="Don't output any plots. Only produce text output", action="store_true")
    opt.add_argument("--vcftype1", help="Type of --vcf1. Options=%s" % [str(t) for t in trh.VcfTypes.__members__],
                     type=str, default="auto")
    opt.add_argument("--vcftype2", help="Type of --vcf2. Options=%s" % [str(t) for t in trh.VcfTypes.__members__],
                     type=str, default="auto")
    opt.add_argument("--ignore-phasing", help="Treat all calls as if they are unphased", action="store_true")
    return parser.parse_args()


BATCH_PAIRS = 4096      # record pairs per compare_calls


class _Run:
    """The state of one comparison: the engine, the accumulators and the locus rows of the batches run so far."""

    def __init__(self, sample_idxs, ignore_phasing, by_period, format_fields, format_bins, stratify_file):
        from ..engine import Engine
        self.eng = Engine(0, reserve_pair_gb=0)
        self.idx = [np.asarray(i, dtype=np.int32) for i in sample_idxs]
        self.S = len(self.idx[0])
        self.ignore_phasing, self.by_period = ignore_phasing, by_period
        self.fields, self.bins, self.sfile = format_fields, format_bins, stratify_file
        self.slots = {}         # period -> slot, in order of appearance
        self.n_slots = L.CMP_MAX_SLOTS if by_period else 1
        n_bins = sum(len(b) - 1 for b in format_bins)
        if n_bins > L.CMP_MAX_BINS:
            raise ValueError("at most %d stratification bins in all" % L.CMP_MAX_BINS)
        self.acc, self.acc_shape = None, (self.n_slots, n_bins)
        self.pairs = []
        self.locus = {"chrom": [], "start": [], "numcalls": [], "metric-conc-seq": [], "metric-conc-len": []}

    def add(self, rec1, rec2):
        self.pairs.append((rec1, rec2))
        if len(self.pairs) >= BATCH_PAIRS:
            self.flush()

    def _shared_gt(self, g, k, s_pad):
        """[L, S_file, P] int16 on the host -> device [L, s_pad, P] in shared-sample order (trk_permute_columns; the
        padding columns are no-calls)."""
        eng = self.eng
        src = eng.upload(g)
        col = eng.upload(np.concatenate([self.idx[k], np.full(s_pad - self.S, -1, np.int32)]))
        dst = eng.empty((g.shape[0], s_pad, g.shape[2]), np.int16)
        eng._chk(eng.lib.trk_permute_columns(eng.ctx, src.ptr, dst.ptr, col.ptr, g.shape[0], g.shape[1], s_pad, g.shape[2]))
        return dst, (src, col)

    def _shared_plane(self, rows, k, s_pad, dtype, fill):
        out = np.full((len(rows), s_pad), fill, dtype=dtype)
        for l, r in enumerate(rows):
            out[l, :self.S] = np.asarray(r)[self.idx[k]]
        return out

    def flush(self):
        if not self.pairs:
            return
        pairs, self.pairs = self.pairs, []
        nl = len(pairs)
        gts = [[r[k].GetGenotypeIndicies() for r in pairs] for k in range(2)]
        ploidy = max(g.shape[1] - 1 for side in gts for g in side)
        s_pad = self.S + ((-self.S) % 4 if ploidy == 2 else 0)
        tables, dlen_absent = pack_pairs([([a.ref_allele] + list(a.alt_alleles), [a.ref_allele_length] + list(a.alt_allele_lengths),
                                           [b.ref_allele] + list(b.alt_alleles), [b.ref_allele_length] + list(b.alt_allele_lengths),
                                           len(a.ref_allele) / len(a.motif)) for a, b in pairs])
        tmp = []
        for k in range(2):
            g = np.full((nl, gts[k][0].shape[0], ploidy), -2, dtype=np.int16)     # a record of lower ploidy: absent haplotypes
            for l, x in enumerate(gts[k]):
                g[l, :, :x.shape[1] - 1] = x[:, :-1]
            tables[k]['gt'], t = self._shared_gt(g, k, s_pad)
            tmp.extend(t)
            if not self.ignore_phasing:
                tables[k]['phased'] = self._shared_plane([x[:, -1] for x in gts[k]], k, s_pad, np.uint8, 0)
        fields = []
        for fmt, bins in zip(self.fields, self.bins):
            planes = [None, None]
            for k in range(2):
                if self.sfile == 2 - k:
                    continue
                rows = [r[k].format[fmt][:, 0] for r in pairs]
                flt = np.asarray(rows[0]).dtype.kind == 'f'
                planes[k] = self._shared_plane(rows, k, s_pad, np.float32 if flt else np.int32,
                                               np.float32('nan') if flt else -2 ** 31)
            fields.append(dict(planes=planes, edges=np.asarray(bins, dtype=np.float64), stratify_file=self.sfile))
        slot = None
        if self.by_period:
            for a, _ in pairs:
                if len(a.motif) not in self.slots:
                    if len(self.slots) >= L.CMP_MAX_SLOTS:
                        raise ValueError("more than %d distinct periods" % L.CMP_MAX_SLOTS)
                    self.slots[len(a.motif)] = len(self.slots)
            slot = np.array([self.slots[len(a.motif)] for a, _ in pairs], dtype=np.uint8)
        if self.acc is None or self.acc['sample_int'].shape[1] != s_pad:
            if self.acc is not None:
                raise ValueError("records of different ploidy layouts in one run")
            self.acc = self.eng.compare_accumulators(s_pad, *self.acc_shape)
        res = self.eng.compare_calls(tables, dlen_absent, acc=self.acc, slot=slot, n_slots=self.n_slots, fields=fields,
                                     ignore_phasing=self.ignore_phasing)
        li = res['locus_int'].get()
        self.eng.sync()
        for d in (res['locus_int'], res['locus_f64'], tables[0]['gt'], tables[1]['gt']) + tuple(tmp):
            d.free()
        raise_for_flags(li, [a.chrom for a, _ in pairs], [a.pos for a, _ in pairs])
        for l in np.flatnonzero(li[:, L.CMP_N]):       # a locus without calls contributes to nothing (reference :555-556)
            n = np.int64(li[l, L.CMP_N])
            self.locus["chrom"].append(pairs[l][0].chrom)
            self.locus["start"].append(pairs[l][0].pos)
            self.locus["numcalls"].append(n)
            self.locus["metric-conc-seq"].append(np.int64(li[l, L.CMP_SEQ]) / n)
            self.locus["metric-conc-len"].append(np.int64(li[l, L.CMP_LEN]) / n)

    def results(self):
        """(overall_results in the reference's nesting, sample_results) from the accumulators."""
        self.flush()
        si = self.acc['sample_int'].get()[:, :self.S]
        bi, bf = self.acc['bin_int'].get(), self.acc['bin_f64'].get()
        self.eng.close()
        keys = ['ALL'] + [p for p in self.slots]
        ints = np.concatenate([bi.sum(axis=0, keepdims=True), bi[[self.slots[p] for p in keys[1:]]]])
        f64s = np.concatenate([bf.sum(axis=0, keepdims=True), bf[[self.slots[p] for p in keys[1:]]]])
        overall = {}
        for i, per in enumerate(keys):
            if ints[i, 0, 0] == 0:
                continue        # (a period is listed once a locus of it has calls, reference :612-613)
            overall[per] = NewOverallPeriod(self.fields, self.bins)
            cells = [overall[per]['ALL']] + [overall[per][f][s] for f, b in zip(self.fields, self.bins) for s in b[:-1]]
            for b, cell in enumerate(cells):
                cell['numcalls'], cell['conc_seq_count'], cell['conc_len_count'] = (np.int64(x) for x in ints[i, b])
                cell.update(zip(MOMENTS, (np.float64(x) for x in f64s[i, b])))
        sample = {'numcalls': si[0], 'conc-seq-count': si[1], 'conc-len-count': si[2]}
        return overall, sample


def _next(it):
    try:
        return next(it)
    except StopIteration:
        return None


def main(args):
    if not os.path.exists(os.path.dirname(os.path.abspath(args.out))):
        common.WARNING("Error: The directory which contains the output location {} does"
                       " not exist".format(args.out))
        return 1
    if os.path.isdir(args.out) and args.out.endswith(os.sep):
        common.WARNING("Error: The output location {} is a "
                       "directory".format(args.out))
        return 1
    vcfreaders = utils.LoadReaders([args.vcf1, args.vcf2], checkgz=True)
    if vcfreaders is None or len(vcfreaders) != 2:
        return 1
    chroms = utils.GetContigs(vcfreaders[0])
    samples = [s for s in vcfreaders[0].samples if s in set(vcfreaders[1].samples)]
    if len(samples) == 0:
        common.WARNING("No shared smaples found between the vcfs")
        return 1
    if args.samples:
        with open(args.samples, "r") as fh:
            use = set(line.strip() for line in fh)
        samples = [s for s in samples if s in use]
    if len(samples) == 0:
        common.WARNING("No shared samples found between the vcfs and the "
                       "--samples file")
        return 1
    samples.sort()
    sample_idxs = [np.array([list(vcf.samples).index(s) for s in samples]) for vcf in vcfreaders]
    if args.stratify_file is not None and args.stratify_file not in [0, 1, 2]:
        common.MSG("--stratify-file must be 0,1, or 2")
        return 1
    format_fields, format_bins = GetFormatFields(args.stratify_fields, args.stratify_binsizes, args.stratify_file, vcfreaders)
    vcf_types = []
    for n, (reader, vcftype) in enumerate(zip(vcfreaders, (args.vcftype1, args.vcftype2))):
        try:
            vcf_types.append(trh.InferVCFType(reader, vcftype))
        except TypeError as te:
            common.WARNING("Error with type of vcf%d: " % (n + 1) + str(te))
            return 1
    if not args.noplot:
        common.WARNING("This build makes no plots: only the three tables are written")
    if not args.region:
        walkers = [iter(r) for r in vcfreaders]
    else:
        if check_region(chroms, chroms, args.region) == 1:
            return 1
        walkers = [iter(r(args.region)) for r in vcfreaders]     # every record compared lies in the region
    current = [_next(w) for w in walkers]
    run = _Run(sample_idxs, args.ignore_phasing, args.period, format_fields, format_bins, args.stratify_file)
    num_records = compared = 0
    while current[0] is not None and current[1] is not None:
        if args.numrecords is not None and num_records >= args.numrecords:
            break
        recs = [trh.HarmonizeRecord(vcf_types[i], current[i]) for i in range(2)]
        # the record(s) next in order -- chromosomes as the first file declares them, then position -- advance
        order = [chroms.index(r.chrom) for r in recs]
        first = min(order)
        min_pos = min(r.pos for r, o in zip(recs, order) if o == first)
        increment = [o == first and r.pos == min_pos for r, o in zip(recs, order)]
        if args.verbose:
            common.MSG(" ".join("%s:%s%s" % (r.chrom, r.pos, "*" if inc else "") for r, inc in zip(recs, increment)), debug=True)
        if handle_overlaps(recs, order, first):
            run.add(*recs)
            compared += 1
        current = [_next(walkers[i]) if increment[i] else current[i] for i in range(2)]
        num_records += 1
    if compared == 0:
        run.eng.close()
        common.WARNING("No comparable records were found, exiting!")
        return 1
    overall_results, sample_results = run.results()
    OutputOverallMetrics(overall_results, format_fields, format_bins, args.out)
    OutputLocusMetrics(run.locus, args.out, args.noplot)
    OutputSampleMetrics(sample_results, samples, args.out, args.noplot)
    return 0


def run():  # pragma: no cover
    sys.exit(main(getargs()))


if __name__ == "__main__":  # pragma: no cover
    run()
