"""Timing of the lambda-expression kernels (csrc/kernels_basic.hip: k_lam_pred,
k_lam_kept, k_lam_rows, k_lam_map, k_lam_reduce) on one GPU.

    python tools/list_lambda_timing.py [--out FILE] [--reps N] [--log2-lists L]

Workload: tools/list_fn_timing.py's — one LIST<INTEGER> column in two settings
holding the same number of elements (2^(L+3); L = 22 by default, 2^25 elements):
 uniform  2^L lists, the elements spread over them evenly at random (mean 8);
 skewed   2^L lists, one of them holding half of all elements, the others
          sharing the rest evenly at random.
Timed per setting, each as `table.withColumns((e, "z")).select("z").materialize()`
followed by a session synchronise, under a host clock:
  [x IN xs | x * 3]              k_lam_map alone (the offsets are shared)
  [x IN xs WHERE x % 2 = 0]      k_lam_pred, the scan, k_lam_kept, k_lam_rows, k_lam_map (copy)
  any(x IN xs WHERE x < 0)       k_lam_pred, the scan, k_lam_rows
  reduce(a = 0, x IN xs | a + x) k_lam_reduce: one thread per row (the known limit)
  reverse(xs)                    the yardstick of the same run: lists.hip's k_lfn_fill copies the
                                 same elements with the same row search, without the interpreter
Medians of --reps runs (5 by default) after two warm-up runs of the same shape
in the same process; `spread_ms` is max − min of the repeats.  After both
settings one `ratios` record gives, per operation, skewed median / uniform
median, reverse's own ratio, and whether the operation's ratio exceeds
reverse's by more than the spread of the repeats (relative: the larger of the
operation's and reverse's (max − min) / median, over both settings) — `reduce`
is exempt, it walks each list in one thread.  A `per_element` record puts the
map-only comprehension next to reverse: the difference of the uniform medians
over the element count is what the interpreter costs per element.
One JSON line per record goes to stdout and, with --out, is appended to FILE.
Every result is checked against numpy before it is timed."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from list_fn_timing import lengths  # noqa: E402  (the same two shapes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
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
    X, x, a = ex.Var("xs"), ex.LambdaVar("x"), ex.LambdaVar("a")
    I = ex.IntegerLit  # noqa: E741
    n = 1 << args.log2_lists
    exprs = {
        "map_x_times_3": ex.ListComprehension(x, None, ex.Multiply(x, I(3)), X),
        "filter_even": ex.ListComprehension(x, ex.Equals(ex.Modulo(x, I(2)), I(0)), None, X),
        "any_negative": ex.ListAny(x, ex.LessThan(x, I(0)), X),
        "reduce_sum": ex.ListReduction(a, x, ex.Add(a, x), I(0), X),
        "reverse": ex.Reverse(X),
    }

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    med, rel = {}, {}
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
        first = np.repeat(offs[:-1], lens)
        pos = np.arange(total, dtype=np.int64) - first
        even = vals % 2 == 0
        sums = np.add.reduceat(np.concatenate([vals, [0]]), offs[:-1])
        sums[lens == 0] = 0
        neg = np.add.reduceat(np.concatenate([(vals < 0).astype(np.int64), [0]]), offs[:-1])
        neg[lens == 0] = 0
        for name, e in exprs.items():
            build = lambda e=e: t.withColumns((e, "z"), header=H, params={}).select("z")  # noqa: E731
            out = build()
            if name in ("any_negative", "reduce_sum"):
                got, valid = out.column_arrays("z")
                want = neg > 0 if name == "any_negative" else sums
                assert valid.all() and np.array_equal(got.astype(want.dtype), want), name
            else:
                et, o2, v2, valid, ev = out.list_arrays("z")
                want = {"map_x_times_3": vals * 3, "filter_even": vals[even],
                        "reverse": vals[np.repeat(offs[1:], lens) - 1 - pos]}[name]
                assert np.array_equal(v2, want) and ev is None, name
                del o2, v2
            del out
            times = []
            for rep in range(args.reps + 2):
                out = build()
                sess.sync()
                t0 = time.perf_counter()
                out.materialize()
                sess.sync()
                dt = time.perf_counter() - t0
                if rep >= 2:
                    times.append(dt)
                del out
            m = statistics.median(times)
            med[setting, name] = m
            rel[setting, name] = (max(times) - min(times)) / m
            emit({"setting": setting, "op": name, "lists": n, "elements": total, "max_list": int(lens.max()),
                  "median_ms": round(m * 1e3, 3), "min_ms": round(min(times) * 1e3, 3),
                  "max_ms": round(max(times) * 1e3, 3), "spread_ms": round((max(times) - min(times)) * 1e3, 3),
                  "reps": args.reps})
        del t, base
    ref = med["skewed", "reverse"] / med["uniform", "reverse"]
    for name in exprs:
        r = med["skewed", name] / med["uniform", name]
        spread = max(rel[s, k] for s in ("uniform", "skewed") for k in (name, "reverse"))
        emit({"ratios": name, "skewed_over_uniform": round(r, 3), "reverse_ratio": round(ref, 3),
              "spread_rel": round(spread, 3),
              "within_bound": None if name == "reduce_sum" else bool(r <= ref * (1 + spread))})
    d = med["uniform", "map_x_times_3"] - med["uniform", "reverse"]
    emit({"per_element": "map_x_times_3 vs reverse (uniform)",
          "map_ms": round(med["uniform", "map_x_times_3"] * 1e3, 3),
          "reverse_ms": round(med["uniform", "reverse"] * 1e3, 3),
          "interpreter_ns_per_element": round(d * 1e9 / (8 * n), 4)})


if __name__ == "__main__":
    main()
