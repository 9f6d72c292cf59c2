"""prancSTR's per-call model on the device (reference: trtools/prancSTR/prancSTR.py).

The host side extracts what a call consists of -- the genotype (A, B) in repeat units, the distinct read values with
their counts, the locus's stutter parameters -- and hands whole batches of calls to ``Engine.mosaic_fit``
(trk_mosaic_fit, include/trk.h).  C, f and the p-value are computed nowhere else: there is no CPU path.

The device's f step is not SLSQP.  Both branches of the likelihood are concave in f, so the maximiser on [0, 0.5] is
an end point or the root of a monotone derivative, and the pass brackets that root to the last bit.  Where the
reference reports the point at which SLSQP's default tolerance stopped it, this package reports the optimum it was
approaching: f agrees to SLSQP's own stopping error and the likelihood is never smaller.
"""
import atexit
import itertools

import numpy as np

from .. import _lib as L

ZERO = 10e-200
MAXSTUTTEROFFSET = 200
_ENGINE = None


def _engine(engine=None):
    """``engine``, or the module's own: made at the first call that brings none, shared by every later one, and closed
    by ``close_engine()`` -- at the latest when the interpreter exits."""
    global _ENGINE
    if engine is not None:
        return engine
    if _ENGINE is None:
        from ..engine import Engine
        _ENGINE = Engine(0, reserve_pair_gb=0)
        atexit.register(close_engine)
    return _ENGINE


def close_engine():
    """Close the module's own engine, if one was made; the next call without ``engine=`` makes another."""
    global _ENGINE
    if _ENGINE is not None:
        _ENGINE.close()
        _ENGINE = None


def StutterProb(delta, stutter_u, stutter_d, stutter_rho):
    """P(r_i | genotype; error model) for a read ``delta`` copies away from the allele: 1 - u - d on the allele, else
    a step up (u) or down (d) times a geometric tail in the number of further copies."""
    if delta == 0:
        return 1 - stutter_u - stutter_d
    step = stutter_u if delta > 0 else stutter_d
    return step * stutter_rho * (1 - stutter_rho) ** (abs(delta) - 1)


def ExtractAB(trrecord):
    """[[A, B], ..] per sample in bp difference from the reference allele, [None, None] for a sample without a call."""
    ref_bp = len(trrecord.ref_allele)
    return [[len(alleles[0]) - ref_bp, len(alleles[1]) - ref_bp] if has_call else [None, None]
            for has_call, alleles in zip(trrecord.GetCalledSamples(), trrecord.GetStringGenotypes())]


def ExtractReadVector(mallreads, period):
    """One entry per read, in repeats from the reference, from 'allele1|count1;allele2|count2'.  The text is read up to
    its first field without a '|'."""
    if mallreads is None:
        return []
    fields = itertools.takewhile(lambda field: "|" in field, mallreads.split(";"))
    return [int(bp) // period for bp, n in (field.split("|") for field in fields) for _ in range(int(n))]


def ConfineRange(x, minval, maxval):
    """x confined to [minval, maxval]."""
    return min(max(x, minval), maxval)


def SF(x):
    """Survival function of a point mass at 0 (prancSTR.py:340-355)."""
    return 0 if x > 0 else 1


def read_counts(reads):
    """The distinct values of a read vector in ascending order and their counts: a call's slice of the CSR arrays."""
    vals, cnts = np.unique(np.asarray(reads, dtype=np.int64), return_counts=True)
    return vals.astype(np.int32), cnts.astype(np.int32)


def stutter_triple(info):
    """(u, d, rho) of a record's INFO with the reference's defaults and zero-replacements (prancSTR.py:499-518)."""
    if "INFRAME_UP" not in info or "INFRAME_DOWN" not in info or "INFRAME_PGEOM" not in info:
        return 0.05, 0.05, 0.90
    u, d, rho = info["INFRAME_UP"], info["INFRAME_DOWN"], info["INFRAME_PGEOM"]
    return (0.01 if u == 0.0 else u), (0.01 if d == 0.0 else d), (0.95 if rho == 1.0 else rho)


def _triple_of(stutter_probs):
    """(u, d, rho) behind a table of StutterProb values indexed delta + MAXSTUTTEROFFSET (the reference's
    ``stutter_probs``), or the triple itself.  The device builds its own table from the triple, so pass the triple
    where it is known: one recovered from a table gives that table back only to a few ulps.  P[+-1] = x * rho and
    P[+-2] = x * rho * (1 - rho) fix rho on whichever side has stutter at all; a table with none on either side
    (u = d = 0, or rho = 0) has no other entry than P[0] = 1 - u - d, which (1 - P[0], 0, 0) gives back."""
    if len(stutter_probs) == 3:
        return tuple(float(x) for x in stutter_probs)
    o = MAXSTUTTEROFFSET
    up1, dn1 = float(stutter_probs[o + 1]), float(stutter_probs[o - 1])
    if up1 > 0:
        rho = 1 - float(stutter_probs[o + 2]) / up1
    elif dn1 > 0:
        rho = 1 - float(stutter_probs[o - 2]) / dn1
    else:
        return 1 - float(stutter_probs[o]), 0.0, 0.0
    if not 0 < rho <= 1:
        raise ValueError("stutter_probs is not a table of StutterProb values: step size parameter %r" % rho)
    return up1 / rho, dn1 / rho, rho


def _fit_one(reads, A, B, stutter_probs, engine):
    vals, cnts = read_counts(reads)
    res = _engine(engine).mosaic_fit(np.array([[[A, B]]], dtype=np.int32), np.array([0, vals.size], dtype=np.int32),
                                     vals, cnts, np.array([_triple_of(stutter_probs)], dtype=np.float64), fit_all=True)
    out = {k: v.get()[0, 0] for k, v in res.items()}
    for v in res.values():
        v.free()
    if (out['status'] & 0xf) != L.MOSAIC_FIT:
        raise ValueError("no fit: status %d (include/trk.h, trk_mosaic_fit)" % out['status'])
    return out


def MaximizeMosaicLikelihoodBoth(reads, A, B, stutter_probs, maxiter=100, locname="None", quiet=False, engine=None):
    """The maximum likelihood mosaic allele C and mosaic fraction f of one call (prancSTR.py:56-117): a batch of one
    through the device pass.  ``stutter_probs``: the reference's table (StutterProb for delta = -200 .. 199) or the
    (u, d, rho) triple.  f is the EXACT maximiser of the likelihood on [0, 0.5] at the returned C, not the point at
    which SLSQP stops.  Returns (C, f), C None when f == 0.  ``maxiter`` is the reference's 100."""
    if maxiter != 100:
        raise ValueError("the device pass runs the reference's default of 100 iterations")
    out = _fit_one(reads, A, B, stutter_probs, engine)
    return (None if out['status'] & L.MOSAIC_NO_C else int(out['C'])), float(out['f'])


def ComputePvalue(reads, A, B, best_C, best_f, stutter_probs, engine=None):
    """The p-value of H0: f = 0 for one call (prancSTR.py:357-385), a batch of one through the device pass, which
    tests its own optimum: f is the exact maximiser of the likelihood at C, not SLSQP's stopping point, so ``best_f``
    is not used; ``best_C`` must be the device's C."""
    out = _fit_one(reads, A, B, stutter_probs, engine)
    C = None if out['status'] & L.MOSAIC_NO_C else int(out['C'])
    if C != best_C:
        raise ValueError("best_C %s is not the fitted mosaic allele %s" % (best_C, C))
    return float(out['pval'])


def mosaic_fit_records(records, readfield='MALLREADS', samples=None, output_all=False, engine=None):
    """The mosaic fit of every call of a batch of harmonised HipSTR records, in one device pass.  ``samples``: the
    columns to process (indices; None: all).  Returns a dict of host arrays over [L, S]: C, support, f, pval, ll_fit,
    ll_null, status (``_lib.MOSAIC_*``: which calls the reference would have tested, prancSTR.py:549-562), the inputs
    of the pass (ab in repeat units, read_off / read_val / read_cnt, stutter [L, 3]) and what a table row needs beside
    them: q, dp (negative -> 0) and ``reads``, the raw read strings.  f is the exact maximiser (module docstring)."""
    records = list(records)
    nl = len(records)
    cols = None if samples is None else [int(s) for s in samples]
    ab, off, vals, cnts, stutter, q, dp, raw = [], [0], [], [], [], [], [], []
    for rec in records:
        period = len(rec.motif)
        gts = ExtractAB(rec)
        texts = list(rec.format[readfield])
        n = len(gts)
        Q = np.asarray(rec.format['Q'], dtype=np.float64).reshape(n, -1)[:, 0]
        DP = np.asarray(rec.format['DP']).reshape(n, -1)[:, 0]
        use = range(n) if cols is None else cols
        stutter.append(stutter_triple(rec.info))
        for i in use:
            A, B = gts[i]
            ab.append([L.MOSAIC_NOCALL_AB] * 2 if A is None or B is None else [A // period, B // period])
            text = texts[i]
            if isinstance(text, bytes):
                text = text.decode()
            v, c = read_counts(ExtractReadVector(text, period))
            vals.append(v)
            cnts.append(c)
            off.append(off[-1] + v.size)
            raw.append(text)
            q.append(Q[i])
            dp.append(max(int(DP[i]), 0))
    ns = len(ab) // nl if nl else 0
    out = dict(ab=np.array(ab, dtype=np.int32).reshape(nl, ns, 2), read_off=np.array(off, dtype=np.int32),
               read_val=np.concatenate(vals + [np.empty(0, np.int32)]).astype(np.int32),
               read_cnt=np.concatenate(cnts + [np.empty(0, np.int32)]).astype(np.int32),
               stutter=np.array(stutter, dtype=np.float64).reshape(nl, 3),
               q=np.array(q, dtype=np.float64).reshape(nl, ns), dp=np.array(dp, dtype=np.int64).reshape(nl, ns),
               reads=[raw[l * ns:(l + 1) * ns] for l in range(nl)])
    if nl == 0 or ns == 0:
        return out
    res = _engine(engine).mosaic_fit(out['ab'], out['read_off'], out['read_val'], out['read_cnt'], out['stutter'],
                                     output_all=output_all)
    for k, v in res.items():
        out[k] = v.get()
        v.free()
    return out


_FIT_KEYS = ('C', 'support', 'f', 'pval', 'll_fit', 'll_null', 'status')


def _batch_tables(rb, hz, readfield):
    """What trk_parse_reads and the fit need of a raw batch beside its text, from the heads of the lines and the
    harmoniser's tables -- per RECORD, nothing per call: (chrom, id, read_idx int8 [L], gt_idx, stutter [L, 3],
    allele_bp int32 [sumA])."""
    chrom, ids, ridx, stutter, keys_of = [], [], [], [], {}
    for l in range(rb.n):
        head = rb.head_fields(l)
        chrom.append(head[0])
        ids.append(head[2])
        fmt = head[8] if len(head) > 8 else ''
        if fmt not in keys_of:
            keys = fmt.split(':')
            keys_of[fmt] = keys.index(readfield) if readfield in keys and keys.index(readfield) < 128 else -1
        ridx.append(keys_of[fmt])
        info = dict(item.split('=', 1) for item in head[7].split(';') if item.startswith('INFRAME_') and '=' in item)
        stutter.append(stutter_triple({k: float(v) for k, v in info.items()}))
    # an allele's length in bp is the length of its harmonised sequence: key str_class[allele] of its locus
    first = np.repeat(hz.allele_off[:-1], np.diff(hz.allele_off)).astype(np.int64)
    at = first + hz.str_class
    bp = (hz.key_off[at + 1] - hz.key_off[at]).astype(np.int64)
    ref = first + hz.str_class[first] if first.size else first
    bp -= hz.key_off[ref + 1] - hz.key_off[ref]
    return chrom, ids, np.array(ridx, dtype=np.int8), np.array(stutter, dtype=np.float64).reshape(rb.n, 3), bp.astype(np.int32)


def _splice(out, rows, sub):
    """The rows ``rows`` of the batch's result ``out`` replaced by the rows of ``sub`` (mosaic_fit_records of those
    records): dense arrays row by row, the CSR arrays record by record."""
    nl, ns = out['ab'].shape[:2]
    for k in _FIT_KEYS + ('ab', 'stutter'):
        out[k][rows] = sub[k]
    cut = out['read_off'][::ns] if ns else out['read_off']
    scut = sub['read_off'][::ns] if ns else sub['read_off']
    vals = [out['read_val'][cut[l]:cut[l + 1]] for l in range(nl)]
    cnts = [out['read_cnt'][cut[l]:cut[l + 1]] for l in range(nl)]
    per_call = np.diff(out['read_off']).reshape(nl, ns)
    for j, l in enumerate(rows):
        vals[l], cnts[l] = sub['read_val'][scut[j]:scut[j + 1]], sub['read_cnt'][scut[j]:scut[j + 1]]
        per_call[l] = np.diff(sub['read_off'])[j * ns:(j + 1) * ns]
    out['read_val'] = np.concatenate(vals + [np.empty(0, np.int32)]).astype(np.int32)
    out['read_cnt'] = np.concatenate(cnts + [np.empty(0, np.int32)]).astype(np.int32)
    out['read_off'] = np.concatenate([[0], np.cumsum(per_call.reshape(-1))]).astype(np.int32)


def mosaic_fit_vcf(path, readfield='MALLREADS', samples=None, output_all=False, batch_records=1024, engine=None):
    """The mosaic fit of every call of a HipSTR VCF, a batch of records at a time, with no Python object per call:
    native reader -> native harmoniser -> the text on the device -> trk_parse_samples (genotypes) -> trk_parse_reads
    (ab and the read vectors) -> trk_mosaic_fit.  A generator: per batch ``mosaic_fit_records``' dict of host arrays
    without ``reads``, ``q`` and ``dp``, plus ``chrom``, ``pos`` (TRRecord.pos) and ``id`` of the records.  ``samples``: the columns to
    report (indices; None: all).  Records the native harmoniser leaves to Python, records either device parser flags and
    batches of another ploidy than two go through the record objects and ``mosaic_fit_records``; their rows are put in
    place."""
    from .. import vcfnative
    from ..utils import tr_harmonizer as trh
    eng = _engine(engine)
    reader = vcfnative.NativeVCFReader(path, batch_records=batch_records)
    reader.device_parse(eng)
    cols = None if samples is None else [int(s) for s in samples]
    try:
        while True:
            rb = reader.read_raw_batch(batch_records)
            if rb.n == 0:
                break
            try:
                nl, ns = rb.n, reader.n_samples
                hz = rb.harmonize('hipstr')
                chrom, ids, ridx, stutter, allele_bp = _batch_tables(rb, hz, readfield)
                host = np.asarray(hz.status) != 0
                d = rb.dev
                if d is None or d['gt'].shape[2] != 2:
                    host[:] = True
                out = dict(chrom=chrom, id=ids, pos=np.array(hz.tr_pos, dtype=np.int64), stutter=stutter)
                if not host.all():
                    ridx[host] = -1
                    pr = eng.parse_reads(d['text'], d['smp_off'], d['line_end'], ns, ridx, np.maximum(hz.period, 1),
                                         gt=d['gt'], allele_off=hz.allele_off, allele_bp=allele_bp)
                    flags = pr.pop('flags')
                    host |= flags.get() != 0
                    flags.free()
                    res = eng.mosaic_fit(pr['ab'], pr['read_off'], pr['read_val'], pr['read_cnt'], stutter,
                                         output_all=output_all)
                    for k, v in list(pr.items()) + list(res.items()):
                        out[k] = v.get()
                        v.free()
                else:
                    out.update(ab=np.empty((nl, ns, 2), np.int32), read_off=np.zeros(nl * ns + 1, np.int32),
                               read_val=np.empty(0, np.int32), read_cnt=np.empty(0, np.int32))
                    out.update({k: np.empty((nl, ns), dt) for k, dt in zip(
                        _FIT_KEYS, (np.int32, np.int32, np.float64, np.float64, np.float64, np.float64, np.uint8))})
                if host.any():
                    rows = np.flatnonzero(host)
                    recs = rb.records()
                    trs = [trh.HarmonizeRecord(trh.VcfTypes.hipstr, recs[l]) for l in rows]
                    _splice(out, rows, mosaic_fit_records(trs, readfield=readfield, output_all=output_all, engine=eng))
                    out['pos'][rows] = [tr.pos for tr in trs]
                if cols is not None:
                    cnt = np.diff(out['read_off']).reshape(nl, ns)[:, cols].reshape(-1)
                    src = np.repeat(out['read_off'][:-1].reshape(nl, ns)[:, cols].reshape(-1), cnt)
                    new_off = np.concatenate([[0], np.cumsum(cnt)])
                    src = src + np.arange(src.size) - np.repeat(new_off[:-1], cnt)
                    out.update(read_off=new_off.astype(np.int32), read_val=out['read_val'][src], read_cnt=out['read_cnt'][src])
                    for k in _FIT_KEYS + ('ab',):
                        out[k] = np.ascontiguousarray(out[k][:, cols])
                yield out
            finally:
                rb.release_device()
    finally:
        reader.close()
