"""Timing of the grouped count (`RETURN a, count(*)` over an inner-join tree) on one GPU.

    python tools/group_count_timing.py [--out FILE] [--reps N] [--max-scale S] [--step K] [--parent-lib REL]

Queries on R-MAT (Graph500 a/b/c, edge factor 16) graphs generated in HBM:
    2hop_a   MATCH (a)-->(b)-->(c) RETURN a, count(*)
    2hop_b   MATCH (a)-->(b)-->(c) RETURN b, count(*)
    1hop_a   MATCH (a)-->(b)       RETURN a, count(*)
each through the fused path (plan "message_passing_grouped") from s10 upward
by K (default 2) while it runs, and through the relational plan (CAPF_FUSED_GROUP=0: the
join chain, then the hash grouping) from s10 upward while the join chain fits
and one query stays under RUN_LIMIT seconds.  With --parent-lib (a library
built from the parent commit, a path relative to the package directory, loaded
through CAPF_LIB_AB) the smallest scale also runs on the parent's library: the
switch must reproduce it.

Every (mode, query, scale) runs in a process of its own, each query under a
time limit (SIGALRM).  A measurement that ends in order without a time — the
join chain out of device memory or refused as too large, or a query that finished but took longer than
RUN_LIMIT — ends its mode's series for that query.  Any other end of a child (a
HIP error, an abort, a signal, the alarm, no result within the limit) ends the
tool: what was gathered is written and nothing more is started on the GPU.  A
time is the median of N synchronised runs after one warm-up run (the result is
downloaded, which waits for the device); the fused runs add one run with HIP
events for the per-kernel share (the session's KernelTimers).  Records are
JSON lines on stdout; the summary (and the ratios) is written to
profiles/group_count_timing.txt (--out)."""
import json
import os
import signal
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_LIMIT = 30
QUERIES = ("2hop_a", "2hop_b", "1hop_a")
PLAN = "message_passing_grouped"


def child(mode, query, scale, reps, result):
    sys.path.insert(0, ROOT)
    if mode != "fused":
        os.environ["CAPF_FUSED_GROUP"] = "0"
    import capf_import
    capf_import.load()
    from capf_amd.expr import CountStar, Var
    from capf_amd.planner import Match, NodeP, Query, RelP, Stage, plan_query
    from capf_amd.synthetic import rmat_graph
    from capf_amd.table import GpuSession

    s = GpuSession(0)
    g = rmat_graph(s, scale, compact=True)
    hops, by = int(query[0]), query[-1]
    names = "abc"[:hops + 1]
    q = Query([Match([NodeP(v) for v in names], [RelP(f"r{i + 1}", names[i], names[i + 1]) for i in range(hops)])],
              [Stage([(by, Var(by, "NODE")), ("n", CountStar())])])
    ts, rows, total = [], 0, 0
    rec = {"mode": mode, "query": query, "scale": scale, "reps": reps}

    def emit():
        with open(result, "w") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec), flush=True)

    for i in range(reps + 1):
        s.reset_profile()
        signal.alarm(RUN_LIMIT + 30)
        t0 = time.perf_counter()
        try:
            op = plan_query(g, q)
            n = op.table.column_arrays("__n")[0]  # the count column as numpy (waits for the device)
        except Exception as e:
            signal.alarm(0)
            rec.update(failed_at_run=i, error=type(e).__name__ + ": " + str(e)[:120])
            emit()
            # the join chain out of device memory, or refused by the library as too large for its hash
            # tables, ends the series in order; anything else (a HIP error) ends the tool
            return 4 if type(e).__name__ in ("DeviceOutOfMemoryException", "NotImplementedException") else 6
        dt = time.perf_counter() - t0
        signal.alarm(0)
        plan = s.last_plan()
        if (plan == PLAN) != (mode == "fused"):
            rec.update(error=f"plan {plan}")
            emit()
            return 5
        rows, total = len(n), int(n.sum())
        if dt > RUN_LIMIT:
            rec.update(over_limit_s=round(dt, 2))
            emit()
            return 3
        if i:
            ts.append(dt * 1e3)
    rec.update(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3),
               groups=rows, joined_rows=total, detail=s.last_plan_detail())
    if mode == "fused":
        s.reset_profile()
        s.set_profiling(True)
        plan_query(g, q).table.column_arrays("__n")
        s.set_profiling(False)
        rec["device_ms"] = {k: round(v["total_ms"], 4) for k, v in s.profile().items()}
    emit()
    return 0


def measure(mode, query, scale, reps, lib=None):
    """One measurement in a fresh process: (status, record).  "ok": measured;
    "benign": the child ended in order without a time (out of device memory or
    too large for the library's hash tables, rc 4, or a query over RUN_LIMIT, rc 3) — the series ends, others may run;
    "abnormal": any other status, a signal or no result within the limit —
    nothing more may be started on the GPU."""
    env = dict(os.environ)
    if lib:
        env["CAPF_LIB_AB"] = lib
    limit = (RUN_LIMIT + 30) * (reps + 2) + 120
    with tempfile.TemporaryDirectory() as tmp:
        result = os.path.join(tmp, "result.json")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, query, str(scale), str(reps), result]
        try:
            rc = subprocess.run(cmd, timeout=limit, env=env).returncode
        except subprocess.TimeoutExpired:
            return "abnormal", {"mode": mode, "query": query, "scale": scale, "error": f"no result within {limit} s"}
        last = open(result).read().strip() if os.path.exists(result) else ""
    rec = json.loads(last) if last else {"mode": mode, "query": query, "scale": scale}
    if rc == 0 and last:
        return "ok", rec
    if rc in (3, 4) and last:
        return "benign", rec
    rec.setdefault("error", f"ended with status {rc}")
    return "abnormal", rec


def summarise(query, fused, rel, parent):
    lines = []
    for sc, f in sorted(fused.items()):
        line = (f"{query} s{sc}: fused {f['median_ms']} [{f['min_ms']}, {f['max_ms']}] ms, {f['groups']} groups, "
                f"{f['joined_rows']} joined rows")
        r = rel.get(sc)
        if r:
            same = (r["groups"], r["joined_rows"]) == (f["groups"], f["joined_rows"])
            line += (f"; relational {r['median_ms']} [{r['min_ms']}, {r['max_ms']}] ms = "
                     f"{r['median_ms'] / f['median_ms']:.2f}x the fused time" + ("" if same else " (RESULTS DIFFER)"))
        if sc == 10 and parent:
            line += f"; parent library {parent['median_ms']} [{parent['min_ms']}, {parent['max_ms']}] ms"
        lines.append(line)
        dev = f.get("device_ms", {})
        tot = sum(dev.values())
        if tot:
            share = ", ".join(f"{k} {v:.3f} ms ({100 * v / tot:.0f}%)"
                              for k, v in sorted(dev.items(), key=lambda kv: -kv[1]))
            lines.append(f"    timed kernels {tot:.3f} ms: {share}")
        lines.append(f"    detail: {f['detail']}")
    return lines + [""]


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        sys.exit(child(args[1], args[2], int(args[3]), int(args[4]), args[5]))
    opts = {"--out": os.path.join(ROOT, "profiles", "group_count_timing.txt"), "--reps": "7", "--max-scale": "24",
            "--step": "2", "--parent-lib": ""}
    for flag in list(opts):
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    reps, top, step = int(opts["--reps"]), int(opts["--max-scale"]), int(opts["--step"])
    lines = ["grouped count on one MI355X: R-MAT, edge factor 16, FOR32 ids; median [min, max] ms of "
             f"{reps} synchronised runs after a warm-up, plan call to downloaded count column", ""]

    def write():
        with open(opts["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")

    for query in QUERIES:
        fused, rel, parent = {}, {}, None
        todo = [("fused", sc, None) for sc in range(10, top + 1, step)] + \
               [("relational", sc, None) for sc in range(10, top + 1, step)]
        if opts["--parent-lib"]:
            todo.append(("parent", 10, opts["--parent-lib"]))
        ended = set()  # series ended in order (out of memory, over the limit)
        for mode, sc, lib in todo:
            if mode in ended:
                continue
            status, rec = measure(mode, query, sc, reps, lib)
            if status == "ok":
                if mode == "parent":
                    parent = rec
                else:
                    (fused if mode == "fused" else rel)[sc] = rec
                continue
            why = rec.get("error") or f"over the limit: {rec.get('over_limit_s')} s"
            if status == "benign":
                ended.add(mode)
                lines.append(f"{query} s{sc} {mode}: this series ends here ({why})")
                continue
            # a fault, an abort, a signal or a hang: what was gathered is written, nothing more is started on the GPU
            lines.append(f"{query} s{sc} {mode}: ENDED ABNORMALLY ({why}); nothing more was started")
            lines.extend(summarise(query, fused, rel, parent))
            write()
            print("\n".join(lines))
            return 1
        lines.extend(summarise(query, fused, rel, parent))
        write()  # (after every query)
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
