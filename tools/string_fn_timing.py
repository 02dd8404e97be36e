"""Timing of toUpper / trim / substring / replace over a large dictionary on one GPU.

    python tools/string_fn_timing.py [all | host | device] [--out FILE] [--reps N] [--dict-log2 D[,D...]]

Workload: a dictionary of 2^D strings (D = 16, 20, 22) of 8-40 bytes
(lowercase letters), 1 % of them 1-16 KiB instead, and a table with one row
per string.  The timed call is `table.withColumns((f(s), "x")).size` — the
lowering builds the function's map (a code map of the dictionary up to 2^16
strings, a value map of the column's distinct values above), the projection
looks every row up — a host clock around it, ended by the device synchronise
of the count's read-back.

Per size and route (each in a process of its own, under a limit of its own):
 host    CAPF_STR_FN=host: Python applies expr.string_fn to every string and
         interns each result (the path before the device route existed).
 device  CAPF_STR_FN=device: one capf_string_fn_codes call (csrc/string_fn.hip)
         and Python only for the strings it answers −2 for.
 cold      a session that has not seen the function: every result is new;
 extended  the same function again after 1/64 more strings entered the
           dictionary, over a table of those.
Medians of N sessions (--reps; one for the host route at 2^22, minutes of
Python) after a warm-up at 2^12 in the same process.  One more device run with
HIP events gives the kernels' device time and, with the bytes each launch
accounts for (KernelTimer: source bytes read, result bytes written, the
per-string offsets and outputs), their achieved bytes/s.

Every run's column is checked against Python's (all rows up to 2^20, a sample
of 2^16 above).  One JSON line per measurement goes to stdout and, with --out,
is appended to FILE; `all` stops at the first run that fails or hits its limit."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = ("toUpper", "trim", "substring", "replace")
LIMITS = {16: 240, 20: 420, 22: 1000}  # seconds one measurement process may take, by dictionary size


def make_strings(n, seed):
    """n distinct strings: 8-40 lowercase bytes (a third with spaces around
    them, so that trim has work), 1 % of them 1-16 KiB."""
    import numpy as np
    rng = np.random.default_rng(seed)
    lens = rng.integers(8, 41, n)
    long_ix = rng.choice(n, max(n // 100, 1), replace=False)
    lens[long_ix] = rng.integers(1024, 16 * 1024 + 1, len(long_ix))
    letters = (rng.integers(0, 26, int(lens.sum()), dtype=np.uint8) + ord("a")).tobytes().decode("ascii")
    ends = np.cumsum(lens)
    out = []
    for i in range(n):
        x = letters[int(ends[i] - lens[i]):int(ends[i])]
        # the position in hex keeps the strings distinct (and those of two seeds apart)
        out.append(f" {x[:-6]}{seed:x}{i:05x} " if i % 3 == 0 else f"{x[:-6]}{seed:x}{i:05x}")
    return out


def child(route, dict_log2, reps, result):
    import numpy as np
    recs = []

    def emit(rec):
        recs.append(rec)
        with open(result, "w") as f:
            f.write("\n".join(json.dumps(r) for r in recs) + "\n")
        print(json.dumps(rec), flush=True)

    sys.path.insert(0, ROOT)
    os.environ["CAPF_STR_FN"] = route
    os.environ.pop("CAPF_STR_LONG", None)
    import capf_import
    capf_import.load()
    from capf_amd import expr as ex
    from capf_amd.header import RecordHeader
    from capf_amd.table import GpuSession

    S = ex.Var("s")
    h = RecordHeader({S: "s"})
    exprs = {"toUpper": (ex.ToUpper(S), ("upper",)), "trim": (ex.Trim(S), ("trim",)),
             "substring": (ex.Substring(S, ex.IntegerLit(2), ex.IntegerLit(12)), ("substring", 3, 12)),
             "replace": (ex.Replace(S, ex.StringLit("ab"), ex.StringLit("xyz")), ("replace", "ab", "xyz"))}

    def run(s, t, fn):
        s.sync()
        a = time.perf_counter()
        out = t.withColumns((exprs[fn][0], "x"), header=h, params={})
        out.size
        return (time.perf_counter() - a) * 1e3, out

    def check(s, out, strings, fn):
        vals, valid = out.column_arrays("x")
        assert valid.all()
        idx = np.arange(len(strings)) if len(strings) <= 1 << 20 else \
            np.random.default_rng(3).integers(0, len(strings), 1 << 16)
        for i in idx:
            want = ex.string_fn(exprs[fn][1], strings[i])
            assert s.lookup(int(vals[i])) == want, (fn, strings[i][:50], s.lookup(int(vals[i]))[:50], want[:50])

    def session(strings):
        s = GpuSession(0)
        codes = np.array([s.intern(x) for x in strings], dtype=np.int64)
        return s, s.table([("s", ex.T_STRING, codes, None)])

    def stats(ts):
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3),
                "max_ms": round(max(ts), 3)}

    t0 = time.perf_counter()
    n = 1 << dict_log2
    strings, more = make_strings(n, 1), make_strings(n // 64, 2)
    warm = make_strings(1 << 12, 3)
    s, t = session(warm)  # the warm-up: modules loaded, kernels resident
    for fn in FNS:
        check(s, run(s, t, fn)[1], warm, fn)
    s.close()
    print(f"  {route} 2^{dict_log2}: strings made and warm-up done in {time.perf_counter() - t0:.1f} s", flush=True)
    base = {"route": route, "strings": n, "heap_bytes": sum(len(x) for x in strings), "reps": reps}
    # up to 2^16 strings the map covers the dictionary, results of earlier functions included: a
    # session per function there; above, a function maps the table's distinct values: one per rep
    groups = [[fn] for fn in FNS] if dict_log2 <= 16 else [list(FNS)]
    cold, ext = {fn: [] for fn in FNS}, {fn: [] for fn in FNS}
    profile = {}
    for rep in range(reps + (1 if route == "device" else 0)):
        profiled = rep == reps  # the device route's last run: HIP events on, not timed
        for group in groups:
            t1 = time.perf_counter()
            s, t = session(strings)
            t2 = None
            for fn in group:
                if profiled:
                    s.reset_profile()
                    s.set_profiling(True)
                dt, out = run(s, t, fn)
                if profiled:
                    s.set_profiling(False)
                    profile[fn] = {k: v for k, v in s.profile().items() if k.startswith(("str_fn", "str_idx"))}
                    continue
                cold[fn].append(dt)
                print(f"  {route} 2^{dict_log2} rep {rep} {fn} cold: {dt:.1f} ms", flush=True)
                if rep == 0:
                    check(s, out, strings, fn)
            if not profiled:
                t2 = s.table([("s", ex.T_STRING, np.array([s.intern(x) for x in more], dtype=np.int64), None)])
                for fn in group:
                    dt, out = run(s, t2, fn)
                    ext[fn].append(dt)
                    if rep == 0:
                        check(s, out, more, fn)
            s.close()
            print(f"  {route} 2^{dict_log2} rep {rep} {group}: {time.perf_counter() - t1:.1f} s", flush=True)
    for fn in FNS:
        rec = dict(base, fn=fn, cold=stats(cold[fn]), extended=stats(ext[fn]), extended_strings=len(more))
        if fn in profile:
            rec["kernels_ms"] = {k: round(v["total_ms"], 4) for k, v in profile[fn].items()}
            rec["kernels_bytes"] = {k: int(v["bytes"]) for k, v in profile[fn].items()}
            rec["kernels_GBps"] = {k: round(v["bytes"] / (v["total_ms"] * 1e-3) / 1e9, 1)
                                   for k, v in profile[fn].items() if v["total_ms"] > 0}
        emit(rec)
    return 0


def measure(route, dict_log2, reps, out):
    """One route at one size in a fresh process; its JSON records, or None
    when it failed or ran into its limit."""
    limit = LIMITS.get(dict_log2, 600)
    with tempfile.TemporaryDirectory() as tmp:
        result = os.path.join(tmp, "result.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", route, str(dict_log2), str(reps), result]
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode  # progress lines pass through
        except subprocess.TimeoutExpired:
            print(f"{route} 2^{dict_log2}: no result within {limit} s", flush=True)
            return None
        text = open(result).read() if os.path.exists(result) else ""
    if text and out:
        with open(out, "a") as f:
            f.write(text)
    if rc != 0 or not text:
        print(f"{route} 2^{dict_log2}: ended with status {rc}", flush=True)
        return None
    return [json.loads(line) for line in text.splitlines()]


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], int(args[2]), int(args[3]), args[4])
    opts = {"--out": None, "--reps": "3", "--dict-log2": "16,20,22"}
    for flag in opts:
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    out, reps = opts["--out"], int(opts["--reps"])
    sizes = [int(x) for x in opts["--dict-log2"].split(",")]
    what = args[0] if args else "all"
    routes = ("device", "host") if what == "all" else (what,)
    done = {}
    for d in sizes:
        for route in routes:
            # (the host route is minutes of Python per run at 2^22: once there, twice at 2^20)
            recs = measure(route, d, reps if route == "device" or d < 20 else 1 if d >= 22 else min(reps, 2), out)
            if recs is None:
                return 1  # nothing more is started
            done[(route, d)] = {r["fn"]: r for r in recs}
    for d in sizes:
        if ("device", d) in done and ("host", d) in done:
            for fn in FNS:
                dv, ho = done[("device", d)][fn], done[("host", d)][fn]
                for phase in ("cold", "extended"):
                    a, b = dv[phase], ho[phase]
                    spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
                    verdict = "is not slower" if a["median_ms"] <= b["median_ms"] + spread else "IS SLOWER"
                    line = {"summary": f"2^{d} {fn} {phase}", "device_median_ms": a["median_ms"],
                            "host_median_ms": b["median_ms"], "spread_ms": round(spread, 3),
                            "verdict": f"device {verdict} than host"}
                    print(json.dumps(line), flush=True)
                    if out:
                        with open(out, "a") as f:
                            f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
