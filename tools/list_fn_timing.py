"""Timing of the list function kernels (csrc/lists.hip: k_lfn_lengths, k_lfn_fill) on one GPU.

    python tools/list_fn_timing.py [--out FILE] [--reps N] [--log2-lists L]

Workload: one LIST<INTEGER> column in two settings holding the same number of
elements (2^(L+3); L = 22 by default, 2^25 elements, 256 MiB):
 uniform  2^L lists, the elements spread over them evenly at random (mean 8);
 skewed   2^L lists, one of them holding half of all elements, the others
          sharing the rest evenly at random.
Timed per setting: slice xs[1..], reverse(xs), xs + xs and range(0, k) with
k = size(xs) − 1 per row (the same lengths), each as
`table.withColumns((e, "z")).select("z").materialize()` followed by a session
synchronise, under a host clock: the lengths launch, the exclusive scan with
its read-back of the total, and the fill launch.  The yardstick is the same
LIST column pushed through filter(TRUE) — lists.hip::gather_list, one thread
per row, which moves the same bytes (this change does not touch it).

Medians of --reps runs after two warm-up runs of the same shape in the same
process.  `bytes` counts what the operation must move: 8 B per element read
and per element written, plus 8 B per row for each pass over an offsets-sized
array (source offsets, lengths written and scanned, new offsets written and
read back by the fill: 5 passes; range reads its argument columns instead of
source offsets).  `hbm_share` is bytes / time over the 8.0 TB/s HBM3E peak — an
end-to-end figure for the whole operation, not a kernel's share of peak.
One JSON line per measurement goes to stdout and, with --out, is appended to
FILE.  Every result is checked against numpy before it is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12


def lengths(setting, n, rng):
    total = 8 * n
    if setting == "uniform":
        return rng.multinomial(total, np.full(n, 1.0 / n)).astype(np.int64)
    lens = np.zeros(n, dtype=np.int64)
    lens[n // 3] = total // 2
    rest = rng.multinomial(total - total // 2, np.full(n - 1, 1.0 / (n - 1))).astype(np.int64)
    lens[np.arange(n) != n // 3] = rest
    return lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log2-lists", type=int, default=22)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import capf_import
    capf_import.load()
    from capf_amd import expr as ex
    from capf_amd.header import RecordHeader
    from capf_amd.table import GpuSession

    sess = GpuSession(0)
    H = RecordHeader({ex.Var(c): c for c in ("xs", "k")})
    X, K = ex.Var("xs"), ex.Var("k")
    n = 1 << args.log2_lists

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for setting in ("uniform", "skewed"):
        rng = np.random.default_rng(5)
        lens = lengths(setting, n, rng)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        total = int(offs[-1])
        vals = rng.integers(-1 << 40, 1 << 40, total).astype(np.int64)
        ok = np.ones(n, dtype=np.uint8)
        base = sess.table([("k", ex.T_INT, lens - 1, None)], nrows=n)
        t = base._new("capf_table_add_list", base._h, b"xs", int(ex.T_INT), offs.ctypes.data, vals.ctypes.data,
                      ok.ctypes.data)
        t.materialize()
        sess.sync()
        nz = lens > 0
        sl_lens = np.where(nz, lens - 1, 0)
        ops = {
            # name: (table builder, elements read, elements written, offsets-sized passes)
            "slice_from_1": (lambda: t.withColumns((ex.ListSliceFrom(X, ex.IntegerLit(1)), "z"), header=H, params={}),
                             int(sl_lens.sum()), int(sl_lens.sum()), 5),
            "reverse": (lambda: t.withColumns((ex.Reverse(X), "z"), header=H, params={}), total, total, 5),
            "self_concat": (lambda: t.withColumns((ex.Add(X, X), "z"), header=H, params={}), 2 * total, 2 * total, 5),
            "range_0_k": (lambda: t.withColumns((ex.Range(ex.IntegerLit(0), K), "z"), header=H, params={}),
                          0, total, 6),
            "filter_true_gather_list": (lambda: t.select(("xs", "z")).filter(ex.BoolLit(True), header=H, params={}),
                                        total, total, 5),
        }
        # check each result once against numpy
        first = np.repeat(offs[:-1], lens)
        pos = np.arange(total, dtype=np.int64) - first
        want = {
            "slice_from_1": vals[pos > 0],
            "reverse": vals[np.repeat(offs[1:], lens) - 1 - pos],
            "range_0_k": pos,
            "filter_true_gather_list": vals,
        }
        for name, (build, rd, wr, passes) in ops.items():
            out = build().select("z")
            et, o2, v2, valid, ev = out.list_arrays("z")
            if name in want:
                assert np.array_equal(v2, want[name]), name
            else:
                assert len(v2) == 2 * total and np.array_equal(v2[:lens[0]], vals[:lens[0]]), name
            assert ev is None
            del out, o2, v2
            times = []
            for rep in range(args.reps + 2):
                out = build().select("z")
                sess.sync()
                t0 = time.perf_counter()
                out.materialize()
                sess.sync()
                dt = time.perf_counter() - t0
                if rep >= 2:
                    times.append(dt)
                del out
            by = 8 * (rd + wr) + 8 * passes * (n + 1)
            med = statistics.median(times)
            emit({"setting": setting, "op": name, "lists": n, "elements": total, "max_list": int(lens.max()),
                  "median_ms": round(med * 1e3, 3), "min_ms": round(min(times) * 1e3, 3),
                  "max_ms": round(max(times) * 1e3, 3), "reps": args.reps, "bytes": by,
                  "GBps": round(by / med / 1e9, 1), "hbm_share": round(by / med / HBM_PEAK, 4)})
        del t, base


if __name__ == "__main__":
    main()
