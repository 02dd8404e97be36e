"""Timing of STARTS WITH / ENDS WITH / CONTAINS with a literal pattern on one GPU.

    python tools/string_match_timing.py [all | dict | rows | host | long BYTES]
                                        [--out FILE] [--reps N] [--dict-log2 D] [--rows-log2 R]

Workload: a dictionary of 2^20 strings of 8-40 bytes (lowercase letters), 1 %
of them 1-16 KiB instead, and a table of 2^24 rows whose STRING column draws
its codes uniformly from the dictionary.  The timed call is
`table.filter(s <kind> 'pattern').size` — the predicate, the compaction of the
passing rows and the count, ended by the device synchronise of the count's
read-back — a host clock around it; medians of N runs after one warm-up run.

Per kind (each route in a process of its own):
 (a) dict  the dictionary path (CAPF_STR_MATCH=dict): cold — a pattern the
           session has not seen, so the per-dictionary-string kernels run —
           and cached (the same pattern again: the rows only look up).  One
           more cold run with HIP events gives the kernels' device time, and
           with the bytes each must move (an 8-byte offset and an answer byte
           per string; of the strings' bytes the pattern's length for STARTS /
           ENDS WITH, all of them for CONTAINS) their achieved bytes/s.
 (b) rows  the per-row path (CAPF_STR_MATCH=rows).
 (c) host  the route the device path replaces, a code map: Python evaluates the
           predicate over the dictionary, uploads 'true' / 'false' codes with
           capf_session_code_map, and the rows look the answer up
           (CAPF_OP_STR_MAP, CAPF_OP_TO_BOOLEAN).  A fresh map per run, as a
           pattern not seen before costs.
 long BYTES  CONTAINS on the cold dictionary path with CAPF_STR_LONG=BYTES (the
           subject length from which a wave scans a string): 64, 256, 1024.

Every run's row count is checked against Python's over the same strings.  One
JSON line per measurement goes to stdout and, with --out, is appended to FILE;
`all` stops at the first measurement that fails or runs into its limit."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("StartsWith", "EndsWith", "Contains")
CHILD_LIMIT = 900  # seconds one measurement process may take
LONGS = (64, 256, 1024)


def make_dictionary(dict_log2, seed=2024):
    """The dictionary's strings: 8-40 lowercase bytes, 1 % of them 1-16 KiB."""
    import numpy as np
    rng = np.random.default_rng(seed)
    n = 1 << dict_log2
    lens = rng.integers(8, 41, n)
    long_ix = rng.choice(n, max(n // 100, 1), replace=False)
    lens[long_ix] = rng.integers(1024, 16 * 1024 + 1, len(long_ix))
    letters = (rng.integers(0, 26, int(lens.sum()), dtype=np.uint8) + ord("a")).tobytes().decode("ascii")
    ends = np.cumsum(lens)
    out, seen = [], set()
    for i in range(n):
        s = letters[int(ends[i] - lens[i]):int(ends[i])]
        if s in seen:  # (8 random letters collide about never; keep the codes dense anyway)
            s = s + format(i, "x")
        seen.add(s)
        out.append(s)
    return out


def patterns(kind, count, seed):
    """Distinct 3-letter patterns (a fresh one per cold run)."""
    import numpy as np
    rng = np.random.default_rng(seed + KINDS.index(kind))
    out = []
    while len(out) < count:
        p = "".join(chr(ord("a") + int(c)) for c in rng.integers(0, 26, 3))
        if p not in out:
            out.append(p)
    return out


def py_matches(kind, strings, p):
    import numpy as np
    fn = {"StartsWith": str.startswith, "EndsWith": str.endswith, "Contains": lambda s, q: q in s}[kind]
    return np.fromiter((fn(s, p) for s in strings), dtype=bool, count=len(strings))


def child(mode, arg, reps, dict_log2, rows_log2, result):
    import numpy as np
    recs = []

    def emit(rec):
        recs.append(rec)
        with open(result, "w") as f:
            f.write("\n".join(json.dumps(r) for r in recs) + "\n")
        print(json.dumps(rec), flush=True)

    sys.path.insert(0, ROOT)
    if mode in ("dict", "long"):
        os.environ["CAPF_STR_MATCH"] = "dict"
    elif mode == "rows":
        os.environ["CAPF_STR_MATCH"] = "rows"
    if mode == "long":
        os.environ["CAPF_STR_LONG"] = str(arg)
    else:
        os.environ.pop("CAPF_STR_LONG", None)
    import capf_import
    capf_import.load()
    from ctypes import POINTER, byref, c_int32, c_int64
    from capf_amd import _lib, expr as ex
    from capf_amd.header import RecordHeader
    from capf_amd.table import GpuSession

    strings = make_dictionary(dict_log2)
    heap_bytes = sum(len(x) for x in strings)
    s = GpuSession(0)
    t0 = time.perf_counter()
    codes = np.array([s.intern(x) for x in strings], dtype=np.int64)
    rng = np.random.default_rng(7)
    rows = codes[rng.integers(0, len(codes), 1 << rows_log2)]
    per_code = np.bincount(rows, minlength=int(codes.max()) + 1)[codes]
    t = s.table([("s", ex.T_STRING, rows, None)])
    h = RecordHeader({ex.Var("s"): "s"})
    print(f"  {mode}: {len(strings)} strings, {heap_bytes} heap bytes, {len(rows)} rows, "
          f"set up in {time.perf_counter() - t0:.1f} s", flush=True)

    def timed(fn):
        s.sync()
        a = time.perf_counter()
        got = fn()
        return (time.perf_counter() - a) * 1e3, got

    def device_filter(kind, p):
        return t.filter(getattr(ex, kind)(ex.Var("s"), ex.StringLit(p)), h, {}).size

    def host_filter(kind, p):  # the code-map route
        hit = py_matches(kind, strings, p)
        m = np.full(int(codes.max()) + 1, -1, dtype=np.int64)
        m[codes] = np.where(hit, s.intern("true"), s.intern("false"))
        mid = c_int32()
        _lib.call("capf_session_code_map", s._h, m.ctypes.data_as(POINTER(c_int64)), len(m), byref(mid))
        prog = ((ex.OP_COL, ex.OP_STR_MAP, ex.OP_TO_BOOLEAN), (0, 1, 0), (0.0, 0.0, 0.0), ("s", "\x01map:%d" % mid.value))
        e, keep = _lib._keepalive_expr(prog)
        return t._new("capf_table_filter", t._h, byref(e), cols=t._cols).size

    def stats(ts):
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3),
                "max_ms": round(max(ts), 3)}

    kinds = ("Contains",) if mode == "long" else KINDS
    for kind in kinds:
        pats = patterns(kind, reps + 2, 99)
        want = {p: int(per_code[py_matches(kind, strings, p)].sum()) for p in pats}
        base = {"mode": mode, "kind": kind, "reps": reps, "strings": len(strings), "heap_bytes": heap_bytes,
                "rows": len(rows)}
        if mode == "long":
            base["str_long"] = arg
        run = host_filter if mode == "host" else device_filter
        if mode == "host":  # the string → BOOLEAN table is not the route's cost: build it first
            s.intern("true"), s.intern("false")
        cold, cached = [], []
        for i, p in enumerate(pats[:reps + 1]):  # the first run is the warm-up
            dt, got = timed(lambda: run(kind, p))
            assert got == want[p], (kind, p, got, want[p])
            print(f"  {mode} {kind} '{p}' run {i}: {dt:.2f} ms ({got} rows)", flush=True)
            if i:
                cold.append(dt)
            if mode == "dict":
                dt2, got2 = timed(lambda: run(kind, p))
                assert got2 == want[p]
                if i:
                    cached.append(dt2)
        rec = dict(base, **{("cold" if mode in ("dict", "long") else "run"): stats(cold)})
        if mode == "dict":
            rec["cached"] = stats(cached)
        if mode in ("dict", "long"):  # the kernels' device time: one more cold run with HIP events
            p = pats[reps + 1]
            s.reset_profile()
            s.set_profiling(True)
            assert run(kind, p) == want[p]
            s.set_profiling(False)
            prof = s.profile()
            # the bytes each kernel must read or write: an 8-byte offset and an answer byte per
            # string, and of the strings' bytes the pattern's length (STARTS / ENDS WITH) or all
            # of them (CONTAINS: subjects under the threshold in the thread tier, the rest — and
            # their 8-byte worklist entries, written by one tier and read by the other — in the
            # wave tier)
            thr = arg if mode == "long" else 256
            lens = np.array([len(x) for x in strings])
            if kind == "Contains":
                listed = lens >= thr
                must = {"str_match": int(9 * len(strings) + lens[~listed].sum() + 8 * listed.sum()),
                        "str_contains_long": int(lens[listed].sum() + 8 * listed.sum())}
            else:
                must = {"str_match": int(9 * len(strings) + np.minimum(lens, len(p)).sum())}
            rec["kernels_ms"] = {k: round(prof[k]["total_ms"], 4) for k in must if k in prof}
            rec["must_move_bytes"] = must
            rec["kernels_GBps"] = {k: round(must[k] / (prof[k]["total_ms"] * 1e-3) / 1e9, 1) for k in must if k in prof}
        emit(rec)
    s.close()
    return 0


def measure(mode, arg, reps, dict_log2, rows_log2, out):
    """One route in a fresh process; its JSON records, or None when it failed
    or ran into its limit."""
    with tempfile.TemporaryDirectory() as tmp:
        result = os.path.join(tmp, "result.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, str(arg), str(reps), str(dict_log2),
               str(rows_log2), result]
        try:
            rc = subprocess.run(cmd, timeout=CHILD_LIMIT).returncode  # progress lines pass through
        except subprocess.TimeoutExpired:
            print(f"{mode} {arg}: no result within {CHILD_LIMIT} s", flush=True)
            return None
        text = open(result).read() if os.path.exists(result) else ""
    if text and out:
        with open(out, "a") as f:
            f.write(text)
    if rc != 0 or not text:
        print(f"{mode} {arg}: ended with status {rc}", flush=True)
        return None
    return [json.loads(line) for line in text.splitlines()]


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], int(args[2]), int(args[3]), int(args[4]), int(args[5]), args[6])
    opts = {"--out": None, "--reps": "7", "--dict-log2": "20", "--rows-log2": "24"}
    for flag in opts:
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    out, reps, dl, rl = opts["--out"], int(opts["--reps"]), int(opts["--dict-log2"]), int(opts["--rows-log2"])
    what = args[0] if args else "all"
    todo = [(what, int(args[1]) if what == "long" else 0)] if what != "all" else \
        [("dict", 0), ("host", 0), ("rows", 0)] + [("long", b) for b in LONGS]
    done = {}
    for mode, arg in todo:
        recs = measure(mode, arg, reps, dl, rl, out)
        if recs is None:
            return 1  # nothing more is started
        done[(mode, arg)] = {r["kind"]: r for r in recs}
    if ("dict", 0) in done and ("host", 0) in done:
        for kind in KINDS:
            d, c = done[("dict", 0)][kind], done[("host", 0)][kind]
            verdict = "beats" if d["cold"]["median_ms"] < c["run"]["median_ms"] else "DOES NOT beat"
            print(f"{kind}: dictionary path cold {d['cold']['median_ms']} ms (cached {d['cached']['median_ms']} ms, "
                  f"kernels {d['kernels_ms']} ms, {d['kernels_GBps']} GB/s) {verdict} the host code map "
                  f"{c['run']['median_ms']} ms")
    longs = {b: done[("long", b)]["Contains"] for b in LONGS if ("long", b) in done}
    if longs:
        print("CONTAINS cold by CAPF_STR_LONG: " + ", ".join(
            f"{b}: {r['cold']['median_ms']} ms [{r['cold']['min_ms']}, {r['cold']['max_ms']}]" for b, r in longs.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
