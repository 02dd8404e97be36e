"""Timing of the fused undirected var-length reach on one GPU.

    python tools/undirected_timing.py [all | fused | config5 | relational SCALE] [--out FILE] [--reps N]

Query: MATCH (a:Person)-[:KNOWS*1..3]-(b:Person) WITH DISTINCT a, b
WITH a, count(*) AS reach RETURN reach, count(*) AS n on R-MAT (Graph500
a/b/c) graphs whose nodes are all :Person, generated in HBM.

(a) fused against the relational plan: R-MAT s6 / s8 / s10 with edge factor
    16, the fused path (plan "fused_var_length_undirected") and the relational
    join chain (CAPF_FUSED_REACH=0, plan "none"), median of N runs each.  The
    comparison is quoted at the largest scale whose relational query finishes
    within RUN_LIMIT seconds.
(b) `config5 --force`: fused at the config-5 shape (2^16 nodes, edge factor 30)
    beside config 5's own directed *1..3 time.  Without --force it only says
    why it is not run today (an estimated 800 s per query).

Every measurement runs in a process of its own, and every query in it under
its own time limit (SIGALRM).  `all` runs the fused measurements of (a) first
and the relational ones by increasing scale, and stops at the first one that
runs into its limit or fails: nothing is started on a GPU after that.  (b) is
a call of its own.  One JSON line per measurement goes to stdout and, with
--out, is appended to FILE."""
import json
import os
import signal
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_LIMIT = 60       # seconds one relational query may take
FUSED_LIMIT = 240    # seconds one fused query may take
SCALES = (6, 8, 10)
EF = 16


def child(mode, scale, ef, direction, lower, upper, reps, result):
    """One measurement; writes its JSON record to `result` and prints it."""
    def emit(rec):
        with open(result, "w") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    if mode == "relational":
        os.environ["CAPF_FUSED_REACH"] = "0"
    import capf_import
    capf_import.load()
    from capf_amd.expr import CountStar, Var
    from capf_amd.graph import ElementTable, ScanGraph
    from capf_amd.planner import Match, NodeP, Query, RelP, Stage, run
    from capf_amd.synthetic import rmat_seed, thresholds
    from capf_amd.table import GpuSession

    s = GpuSession(0)
    m = ef << scale
    rels = s.rmat_rels(scale, rmat_seed(scale), thresholds(), 0, m)
    nodes = s.range_nodes(0, 1 << scale, id_col="id")
    g = ScanGraph(s, [ElementTable("node", frozenset(["Person"]), nodes, {})],
                  [ElementTable("rel", frozenset(["KNOWS"]), rels, {})])
    q = Query([Match([NodeP("a", ("Person",)), NodeP("b", ("Person",))],
                     [RelP("k", "a", "b", ("KNOWS",), direction=direction, length=(lower, upper))])],
              [Stage([("a", Var("a")), ("b", Var("b"))], distinct=True),
               Stage([("a", Var("a")), ("reach", CountStar())]),
               Stage([("reach", Var("reach")), ("n", CountStar())])])
    want = "none" if mode == "relational" else \
        "fused_var_length_undirected" if direction == "both" else \
        "fused_var_length_trails" if lower >= 2 else "fused_var_length_reach"
    base = {"mode": mode, "scale": scale, "ef": ef, "direction": direction, "lower": lower, "upper": upper}
    ts, res = [], None
    for i in range(reps + 1):  # the first run is the warm-up (index build, caches)
        s.reset_profile()
        signal.alarm(RUN_LIMIT + 15 if mode == "relational" else FUSED_LIMIT)
        t0 = time.perf_counter()
        try:
            res = run(g, q)
        except Exception as e:  # e.g. the relational plan out of device memory: keep what was timed
            signal.alarm(0)
            emit(dict(base, failed_at_run=i, error=type(e).__name__, runs_ms=[round(t, 3) for t in ts]))
            return 4
        dt = time.perf_counter() - t0
        signal.alarm(0)
        assert s.last_plan() == want, (s.last_plan(), want)
        print(f"  {mode} s{scale} ef{ef} {direction} *{lower}..{upper} run {i}: {dt * 1e3:.2f} ms", flush=True)
        if mode == "relational" and dt > RUN_LIMIT:
            emit(dict(base, over_limit_s=dt))
            return 3
        if i:
            ts.append(dt * 1e3)
    hist = sorted([r["reach"], r["n"]] for r in res)
    dev = {}
    if mode == "fused":  # device time of the kernels, one more run with HIP events
        s.reset_profile()
        s.set_profiling(True)
        signal.alarm(FUSED_LIMIT)
        run(g, q)
        signal.alarm(0)
        s.set_profiling(False)
        dev = {k: round(v["total_ms"], 4) for k, v in s.profile().items()}
    emit(dict(base, reps=reps, median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3),
              max_ms=round(max(ts), 3), sources=sum(n for _, n in hist), pairs=sum(r * n for r, n in hist),
              device_ms=dev))
    return 0


def measure(mode, scale, ef, direction, lower, upper, reps, out):
    """Runs one measurement in a fresh process; its JSON record, or None when
    it ran into a limit or failed."""
    per_run = RUN_LIMIT + 15 if mode == "relational" else FUSED_LIMIT
    limit = per_run * (reps + 2) + 120
    with tempfile.TemporaryDirectory() as tmp:
        result = os.path.join(tmp, "result.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, str(scale), str(ef), direction,
               str(lower), str(upper), str(reps), result]
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode  # progress lines pass through
        except subprocess.TimeoutExpired:
            print(f"{mode} s{scale}: no result within {limit} s", flush=True)
            return None
        last = open(result).read().strip() if os.path.exists(result) else ""
    if last and out:
        with open(out, "a") as f:
            f.write(last + "\n")
    if rc != 0 or not last:
        print(f"{mode} s{scale}: ended with status {rc}", flush=True)
        return None
    return json.loads(last)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        mode, scale, ef, direction = args[1], int(args[2]), int(args[3]), args[4]
        lower, upper, reps = map(int, args[5:8])
        sys.exit(child(mode, scale, ef, direction, lower, upper, reps, args[8]))
    out, reps = None, 10
    for flag in ("--out", "--reps"):
        if flag in args:
            i = args.index(flag)
            val = args[i + 1]
            del args[i:i + 2]
            if flag == "--out":
                out = val
            else:
                reps = int(val)
    what = args[0] if args else "all"
    fused, relational = {}, {}
    if what == "config5":
        if "--force" not in args:
            print("config5: not started.  The kernel has no expanded-rows shortcut; from the s10 rate the\n"
                  f"config-5 shape takes about 800 s per query, above the {FUSED_LIMIT} s limit per fused query\n"
                  "(DESIGN.md, Undirected steps).  After a kernel change that brings it under the limit:\n"
                  "    python tools/undirected_timing.py config5 --force")
            return 2
        c5 = measure("fused", 16, 30, "out", 1, 3, reps, out)
        if c5 is None:
            return 1
        b = measure("fused", 16, 30, "both", 1, 3, reps, out)
        if b is None:
            return 1
        print(f"(b) config-5 shape (2^16 nodes, ef 30): undirected *1..3 fused {b['median_ms']} ms "
              f"[{b['min_ms']}, {b['max_ms']}], {b['pairs']} pairs; config 5 (directed *1..3) "
              f"{c5['median_ms']} ms [{c5['min_ms']}, {c5['max_ms']}]")
        return 0
    if what in ("all", "fused"):
        for sc in SCALES:
            r = measure("fused", sc, EF, "both", 1, 3, reps, out)
            if r is None:
                return 1
            fused[sc] = r
    if what in ("all", "relational"):
        scales = SCALES if what == "all" else (int(args[1]),)
        for sc in scales:
            r = measure("relational", sc, EF, "both", 1, 3, reps, out)
            if r is None:
                break  # a limit or a failure: nothing more is started
            relational[sc] = r
            f = fused.get(sc)
            if f:
                assert (f["sources"], f["pairs"]) == (r["sources"], r["pairs"]), "fused and relational disagree"
                print(f"(a) s{sc} ef{EF}: fused {f['median_ms']} ms, relational {r['median_ms']} ms "
                      f"({r['median_ms'] / f['median_ms']:.1f}x)")
        if what == "all" and relational:
            print(f"(a) is quoted at s{max(relational)}: the largest scale whose relational query "
                  f"finishes within {RUN_LIMIT} s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
