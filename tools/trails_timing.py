"""Timing of the fused trail reach (var-length with lower bound 2) on one GPU.

    python tools/trails_timing.py [all | fused | relational SCALE] [--out FILE] [--reps N]

Query: MATCH (a:Person)-[:KNOWS*2..3]->(b:Person) WITH DISTINCT a, b
WITH a, count(*) AS reach RETURN reach, count(*) AS n on R-MAT (Graph500
a/b/c) graphs whose nodes are all :Person, generated in HBM.

(a) fused against the relational plan: R-MAT s8 / s10 / s12 with edge factor
    16, the fused path (plan "fused_var_length_trails") and the relational
    join chain (CAPF_FUSED_REACH=0, plan "none"), median of N runs each.  The
    comparison is quoted at the largest scale whose relational query finishes
    within RUN_LIMIT seconds.
(b) fused at the config-5 shape (2^16 nodes, edge factor 30) beside config 5's
    own *1..3 time.  The relational plan cannot run *2..3 at this size (about
    1e10 path rows of 40 B), so there is no ratio to quote.

Every measurement runs in a process of its own, and every query in it under
its own time limit (SIGALRM).  `all` runs the fused measurements first and the
relational ones by increasing scale, and stops at the first one that runs
into its limit or fails: nothing is started on a GPU after that.  One JSON
line per measurement goes to stdout and, with --out, is appended to FILE."""
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
SCALES = (8, 10, 12)
EF = 16


def child(mode, scale, ef, lower, upper, reps, result):
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
                     [RelP("k", "a", "b", ("KNOWS",), length=(lower, upper))])],
              [Stage([("a", Var("a")), ("b", Var("b"))], distinct=True),
               Stage([("a", Var("a")), ("reach", CountStar())]),
               Stage([("reach", Var("reach")), ("n", CountStar())])])
    want = "none" if mode == "relational" else \
        "fused_var_length_trails" if lower >= 2 else "fused_var_length_reach"
    ts, res = [], None
    for i in range(reps + 1):  # the first run is the warm-up (index build, caches)
        s.reset_profile()
        signal.alarm(RUN_LIMIT + 15 if mode == "relational" else 300)
        t0 = time.perf_counter()
        try:
            res = run(g, q)
        except Exception as e:  # e.g. the relational plan out of device memory: keep what was timed
            signal.alarm(0)
            emit({"mode": mode, "scale": scale, "ef": ef, "lower": lower, "upper": upper,
                  "failed_at_run": i, "error": type(e).__name__, "runs_ms": [round(t, 3) for t in ts]})
            return 4
        dt = time.perf_counter() - t0
        signal.alarm(0)
        assert s.last_plan() == want, (s.last_plan(), want)
        print(f"  {mode} s{scale} ef{ef} *{lower}..{upper} run {i}: {dt * 1e3:.2f} ms", flush=True)
        if mode == "relational" and dt > RUN_LIMIT:
            emit({"mode": mode, "scale": scale, "ef": ef, "lower": lower, "upper": upper, "over_limit_s": dt})
            return 3
        if i:
            ts.append(dt * 1e3)
    hist = sorted([r["reach"], r["n"]] for r in res)
    dev = {}
    if mode == "fused":  # device time of the kernels, one more run with HIP events
        s.reset_profile()
        s.set_profiling(True)
        run(g, q)
        s.set_profiling(False)
        dev = {k: round(v["total_ms"], 4) for k, v in s.profile().items()}
    emit({"mode": mode, "scale": scale, "ef": ef, "lower": lower, "upper": upper, "reps": reps,
          "median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3),
          "max_ms": round(max(ts), 3), "sources": sum(n for _, n in hist),
          "pairs": sum(r * n for r, n in hist), "device_ms": dev})
    return 0


def measure(mode, scale, ef, lower, upper, reps, out):
    """Runs one measurement in a fresh process; its JSON record, or None when
    it ran into a limit or failed."""
    limit = (RUN_LIMIT + 15) * (reps + 1) + 120
    with tempfile.TemporaryDirectory() as tmp:
        result = os.path.join(tmp, "result.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, str(scale), str(ef), str(lower),
               str(upper), str(reps), result]
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
        mode, scale, ef, lower, upper, reps = args[1], *map(int, args[2:7])
        sys.exit(child(mode, scale, ef, lower, upper, reps, args[7]))
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
    if what in ("all", "fused"):
        for rec_args in [("fused", 16, 30, 2, 3), ("fused", 16, 30, 1, 3)] + \
                        [("fused", sc, EF, 2, 3) for sc in SCALES]:
            r = measure(*rec_args, reps, out)
            if r is None:
                return 1
            fused[(r["scale"], r["ef"], r["lower"])] = r
        b, c5 = fused[(16, 30, 2)], fused[(16, 30, 1)]
        print(f"(b) config-5 shape (2^16 nodes, ef 30): *2..3 fused {b['median_ms']} ms "
              f"[{b['min_ms']}, {b['max_ms']}], {b['pairs']} pairs; config 5 (*1..3) {c5['median_ms']} ms "
              f"[{c5['min_ms']}, {c5['max_ms']}]; the relational plan cannot run *2..3 at this size")
    if what in ("all", "relational"):
        scales = SCALES if what == "all" else (int(args[1]),)
        for sc in scales:
            r = measure("relational", sc, EF, 2, 3, reps, out)
            if r is None:
                break  # a limit or a failure: nothing more is started
            relational[sc] = r
            f = fused.get((sc, EF, 2))
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
