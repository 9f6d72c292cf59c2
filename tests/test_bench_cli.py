"""bench.py's command line without a GPU: what a plain run leaves out and --full puts back, and --dump-outputs' files
(dtype, the byte budget, the same sample in every run) on stand-ins for the device arrays."""
import glob
import os
import types

import numpy as np

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr('sys.argv', ['bench.py'] + list(argv))
    return bench.parse()


def test_plain_run_leaves_out_everything_but_the_headline(monkeypatch):
    a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_check and a.no_cpu_baseline and a.no_assoc and a.no_extras


def test_full_run_keeps_its_switches(monkeypatch):
    a = _parse(monkeypatch, '--full')
    assert a.full and not (a.no_check or a.no_cpu_baseline or a.no_assoc or a.no_extras)
    a = _parse(monkeypatch, '--full', '--no-extras', '--dump-outputs', 'd')
    assert a.no_extras and not a.no_check and a.dump_outputs == 'd'


class _Dev:
    """DeviceArray's reading side over a host array."""

    def __init__(self, a):
        self.a, self.shape, self.dtype, self.nbytes = a, a.shape, a.dtype, a.nbytes

    def get(self):
        return self.a.copy()

    def get_rows(self, lo, hi):
        return self.a[lo:hi].copy()


def _workload(rng, L=300, S=64):
    def stats():
        return types.SimpleNamespace(allele_count=_Dev(rng.integers(0, 2 * S, (1, 7 * L)).astype(np.int32)),
                                     locus_int=_Dev(rng.integers(0, 9, (1, L, 12)).astype(np.int32)),
                                     locus_f64=_Dev(rng.normal(size=(1, L, 12))))
    co = types.SimpleNamespace(gt_out=_Dev(rng.integers(-1, 9, (L, S, 2)).astype(np.int16)),
                               filter_mask=_Dev(rng.integers(0, 2 ** 32, (L, S), dtype=np.uint32)),
                               sample_counters=_Dev(rng.integers(0, L, (4, S)).astype(np.int64)),
                               sample_totaldp=_Dev(rng.integers(0, 2 ** 40, S).astype(np.int64)),
                               sample_dp_missing=_Dev(np.zeros(S, np.int64)))
    return types.SimpleNamespace(last=0, stats_a=[stats()], stats_b=[stats()], call_out=co,
                                 bits=_Dev(rng.integers(0, 16, L).astype(np.uint32)),
                                 loc_counters=_Dev(np.arange(32, dtype=np.int64)))


def test_dump_outputs_files(tmp_path, monkeypatch):
    wl = _workload(np.random.default_rng(1))
    f64 = wl.stats_b[0].locus_f64.a            # statistics of loci without calls are undefined
    f64[0, 5, 2:4], f64[0, 7, 0], f64[0, 9, 1] = np.nan, np.inf, -np.inf
    # whole arrays: every value survives the conversion
    w = bench.dump_outputs(wl, str(tmp_path / 'whole'), 3)
    assert len(w) == 13 and all(tuple(got) == tuple(whole) for got, whole in w.values())
    gt = np.load(tmp_path / 'whole' / 'dump_gt_out.npy')
    assert gt.dtype == np.float32 and np.array_equal(gt, wl.call_out.gt_out.a)
    mask = np.load(tmp_path / 'whole' / 'dump_filter_mask.npy')
    assert mask.dtype == np.float64 and np.array_equal(mask.astype(np.uint32), wl.call_out.filter_mask.a)
    assert np.array_equal(np.load(tmp_path / 'whole' / 'stat_locus_f64.npy'), wl.stats_a[0].locus_f64.a)
    assert not np.load(tmp_path / 'whole' / 'stat_locus_f64_nonfinite.npy').any()
    # undefined statistics: 0 in the array, marked beside it; everything else untouched
    got, marks = (np.load(tmp_path / 'whole' / ('dump_locus_f64%s.npy' % x)) for x in ('', '_nonfinite'))
    assert marks.dtype == np.float32 and marks.shape == got.shape and np.isfinite(got).all()
    assert list(marks[0, 5]) == [0, 0, 1, 1] + [0] * 8 and marks[0, 7, 0] == 2 and marks[0, 9, 1] == 3 and marks.sum() == 7
    assert np.array_equal(got[marks == 0], f64[marks == 0]) and not got[marks != 0].any()
    assert np.array_equal(np.load(tmp_path / 'whole' / 'dump_sample_totaldp.npy').astype(np.int64),
                          wl.call_out.sample_totaldp.a)
    # a budget the large arrays do not fit: row samples, within the budget, the same in every run
    monkeypatch.setattr(bench, 'DUMP_TOTAL_BYTES', 13 * 4096)
    monkeypatch.setattr(bench, 'DUMP_ROWWISE_BYTES', 2 ** 16)      # the two planes are fetched row by row, the rest whole
    w1 = bench.dump_outputs(wl, str(tmp_path / 'a'), 3)
    w2 = bench.dump_outputs(wl, str(tmp_path / 'b'), 3)
    assert w1 == w2 and w1['dump_gt_out'][0][1:] == [64, 2] and w1['dump_gt_out'][0][0] < 300
    assert w1['stat_locus_f64'][0] == [4096 // (12 * 12), 12]       # (8 bytes a value + 4 for its mark)
    assert w1['dump_loc_counters'][0] == [32]
    files = sorted(glob.glob(str(tmp_path / 'a' / '*.npy')))
    assert len(files) == 15         # the 13 arrays and the marks of the two float ones
    for f in files:
        x, y = np.load(f), np.load(os.path.join(str(tmp_path / 'b'), os.path.basename(f)))
        assert x.dtype in (np.float32, np.float64) and x.nbytes <= 4096 and np.isfinite(x).all()
        assert np.array_equal(x, y, equal_nan=True)
    # the sampled rows are rows of the whole array
    rows = np.load(tmp_path / 'a' / 'dump_gt_out.npy')
    whole = wl.call_out.gt_out.a.astype(np.float32)
    assert all((whole == r).all(axis=(1, 2)).any() for r in rows)
