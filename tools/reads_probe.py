"""trk_parse_reads on a synthetic HipSTR-shape text (profiles/reads_probe_notes.md): pass 1 and pass 2 by the library's
timers, trk_parse_samples on the same text as the yardstick, and the host road (ExtractReadVector + read_counts) on
10 000 of the same calls.  Usage: python tools/reads_probe.py [records samples reps]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trtools_amd import _lib as L                     # noqa: E402
from trtools_amd import prancSTR                      # noqa: E402
from trtools_amd.engine import Engine                 # noqa: E402

NL, NS, REPS = (int(x) for x in (sys.argv[1:4] + ['2000', '5000', '5'][len(sys.argv) - 1:]))
rng = np.random.default_rng(7)
pool, fields = [], []
for _ in range(4096):                                # tokens GT:DP:Q:ALLREADS:MALLREADS, MALLREADS of 4 - 12 entries
    n = int(rng.integers(4, 13))
    bps = rng.integers(-24, 25, size=n)
    mall = ';'.join('%d|%d' % (b, c) for b, c in zip(bps, rng.integers(1, 30, size=n)))
    alls = ';'.join('%d|%d' % (b, c) for b, c in zip(bps + rng.integers(-1, 2, size=n), rng.integers(1, 40, size=n)))
    pool.append('%d|%d:%d:%.2f:%s:%s' % (rng.integers(0, 3), rng.integers(0, 3), rng.integers(5, 60), rng.random(), alls, mall))
    fields.append(mall)
lines, smp_off, line_end, at, calls = [], [], [], 0, []
for l in range(NL):
    pick = rng.integers(0, len(pool), size=NS)
    head = 'chr1\t%d\t.\tA\t.\t.\t.\tPERIOD=3\tGT:DP:Q:ALLREADS:MALLREADS\t' % (l + 1)
    line = head + '\t'.join(pool[i] for i in pick) + '\n'
    smp_off.append(at + len(head))
    at += len(line)
    line_end.append(at - 1)
    lines.append(line)
    if l < 2:
        calls += [fields[i] for i in pick]
text = np.frombuffer(''.join(lines).encode(), dtype=np.uint8)
del lines
print("text %.1f MB, %d calls, %.1f bytes per token" % (text.size / 1e6, NL * NS, text.size / (NL * NS)))
eng = Engine(0, reserve_pair_gb=0)
td = eng.empty((text.size + 32,), np.uint8)
eng._chk(eng.lib.trk_memcpy_h2d(eng.ctx, td.ptr, text.ctypes.data, text.size))
so, le = eng.upload(np.array(smp_off, np.int64)), eng.upload(np.array(line_end, np.int64))
ridx, per, gi = eng.upload(np.full(NL, 4, np.int8)), eng.upload(np.full(NL, 3, np.int32)), np.zeros(NL, np.int8)
rin = L.ReadsIn(td.ptr, td.nbytes, NL, NS, so.ptr, le.ptr, ridx.ptr, per.ptr, None, None, None)
off, flags = eng.empty((NL * NS + 1,), np.int32), eng.empty((NL,), np.uint8)
ws = eng.empty((L.reads_ws_bytes(NL, NS),), np.uint8)
rout = L.ReadsOut(off.ptr, flags.ptr, ws.ptr, None, None, None)
t = {'pass 1': [], 'pass 2': [], 'parse_samples': []}
for rep in range(REPS + 1):                          # (the first round warms up)
    eng.timer_start(0)
    eng._chk(eng.lib.trk_parse_reads(eng.ctx, C.byref(rin), C.byref(rout), 1))
    eng.timer_stop(0)
    n_ent = int(off.get_rows(NL * NS, NL * NS + 1)[0])
    val, cnt = eng.empty((n_ent,), np.int32), eng.empty((n_ent,), np.int32)
    rout.read_val, rout.read_cnt = val.ptr, cnt.ptr
    eng.timer_start(1)
    eng._chk(eng.lib.trk_parse_reads(eng.ctx, C.byref(rin), C.byref(rout), 2))
    eng.timer_stop(1)
    eng.sync()
    eng.timer_start(2)
    ps = eng.parse_samples(td, so, le, NS, 2, gi)
    eng.timer_stop(2)
    eng.sync()
    for a in [ps['gt'], ps['locus_ploidy'], ps['flags'], val, cnt]:
        a.free()
    if rep:
        for k, slot in zip(t, range(3)):
            t[k].append(eng.timer_ms(slot))
print("entries %d, flagged records %d" % (n_ent, int((flags.get() != 0).sum())))
for k, v in t.items():
    print("%-14s median %.3f ms (min %.3f, max %.3f)  %.1f GB/s of text" % (k, np.median(v), min(v), max(v),
                                                                           text.size / np.median(v) / 1e6))
calls = calls[:10000]
t0 = time.perf_counter()
for f in calls:
    prancSTR.read_counts(prancSTR.ExtractReadVector(f, 3))
dt = time.perf_counter() - t0
print("host road: %d calls in %.3f s, %.2f us per call (%.1f s per %d calls)" % (len(calls), dt, 1e6 * dt / len(calls),
                                                                               dt / len(calls) * NL * NS, NL * NS))
eng.close()
