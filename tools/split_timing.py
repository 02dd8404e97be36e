"""Timing of split(s, ',') (csrc/string_fn.hip: k_split_count, k_split_write and
their wave-tier twins, then the interning of the pieces) on one GPU.

    python tools/split_timing.py [--out profiles/split_timing.txt] [--reps N] [--log2-rows 20,22]

Workloads, each a one-column STRING table:
 short   2^k rows (k = 20 and 22 by default) of subjects "w<i>,x<j>,<t>" of 9 to
         17 bytes drawn from 2^16 distinct strings, three pieces each;
 long    2^10 rows of 64 short subjects and 8 subjects of 64 KiB (4096 pieces
         of 15 bytes each), so that both tiers run.
Timed per workload and route, under a host clock around
`table.withColumns((split(s, ','), "z")).select("z").materialize()` and a session
synchronise: `cold` is the first run of a fresh session (the pieces are new
strings: the dictionary's index is built and the pieces appended), `warm` the
median of --reps further runs (every piece is in the dictionary).  Device
route: the per-kernel profile of one more warm run beside it (label, launches,
ms, profiled bytes).  Host route: the same table with CAPF_STR_SPLIT=host
(expr.split_fn per distinct pair, the column built with add_list), one cold
and one warm run.  The delimiter is a literal, so the route is chosen without
a download (a delimiter column's distinct values would be fetched first).
Every result is checked against Python's str.split on a sample of rows before
it is timed.  One JSON line per measurement goes to stdout and, with --out, is
appended to FILE.  Nothing here is a target: the parent commit has no split."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def short_rows(n, rng):
    pool = [f"w{i},x{i % 977},{'t' * (1 + i % 5)}" for i in range(1 << 16)]
    return [pool[i] for i in rng.integers(0, len(pool), n).tolist()]


def long_rows():
    big = [",".join(f"piece{j:05d}{k:05d}" for j in range(4096)) for k in range(8)]
    rows = [f"s{i},u{i % 7}" for i in range(1 << 10)]
    for k, b in enumerate(big):
        rows[100 * k + 3] = b
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2-rows", default="20,22")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import capf_import
    capf_import.load()
    from capf_amd import expr as ex
    from capf_amd.header import RecordHeader
    from capf_amd.table import GpuSession

    H = RecordHeader({ex.Var("s"): "s"})
    E = ex.Split(ex.Var("s"), ex.StringLit(","))

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def once(sess, t):
        sess.sync()
        t0 = time.perf_counter()
        out = t.withColumns((E, "z"), header=H, params={}).select("z").materialize()
        sess.sync()
        return out, time.perf_counter() - t0

    workloads = [(f"short_2^{k}", lambda k=k: short_rows(1 << int(k), np.random.default_rng(11)))
                 for k in args.log2_rows.split(",")] + [("long_64KiB", long_rows)]
    for name, make in workloads:
        rows = make()
        n = len(rows)
        src_bytes = sum(len(r) for r in rows)
        for route in ("device", "host"):
            if route == "host":
                os.environ["CAPF_STR_SPLIT"] = "host"
            else:
                os.environ.pop("CAPF_STR_SPLIT", None)
            sess = GpuSession(0)
            t = sess.table([("s", ex.T_STRING, rows, None)], nrows=n)
            t.materialize()
            out, cold = once(sess, t)
            et, offs, vals, valid, ev = out.list_arrays("z")
            for i in list(range(0, n, max(1, n // 50))) + [n - 1]:
                got = [sess.lookup(int(c)) for c in vals[offs[i]:offs[i + 1]]]
                assert got == rows[i].split(","), (name, route, i)
            pieces = int(offs[-1])
            del out, offs, vals
            reps = args.reps if route == "device" else 1
            warm = [once(sess, t)[1] for _ in range(reps)]
            rec = {"workload": name, "route": route, "rows": n, "subject_bytes": src_bytes, "pieces": pieces,
                   "cold_ms": round(cold * 1e3, 3), "warm_median_ms": round(statistics.median(warm) * 1e3, 3),
                   "warm_min_ms": round(min(warm) * 1e3, 3), "warm_max_ms": round(max(warm) * 1e3, 3), "reps": reps}
            if route == "device":
                sess.set_profiling(True)
                sess.reset_profile()
                once(sess, t)
                rec["profile"] = {k: {"launches": v["launches"], "ms": round(v["total_ms"], 4), "bytes": v["bytes"]}
                                  for k, v in sorted(sess.profile().items()) if k.startswith("str_")}
                sess.set_profiling(False)
            emit(rec)
            sess.close()
    os.environ.pop("CAPF_STR_SPLIT", None)


if __name__ == "__main__":
    main()
