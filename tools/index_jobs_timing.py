"""Timing of the indexed 2-hop count's job rule (k_c5_gather<…, IDX>) on one GPU.

    python tools/index_jobs_timing.py [--libs LIB,LIB] [--variants SPEC;SPEC…] [--rounds N] [--reps N]
                                      [--scale S] [--out FILE]

Two graphs, FOR24 ids, 16 << S rels (S = 24: the headline shape):
  rmat    the headline R-MAT graph, generated in HBM;
  skewed  uniform rels of the same row count with 60 % of the sources drawn
          from 40,000 ids of bucket 77 under the node mix (oracle.nodemix, as
          tests/test_two_hop_jobs.py) — one out-run ≈150 × the mean.  Drawn on
          the host and uploaded once per process.

A variant is a knob setting, NAME:VAR=VALUE,VAR=VALUE (the knobs, CAPF_C5_JOB_SPLIT,
CAPF_C5_STEAL_TILES and CAPF_C5_EXCESS_SPLIT, are read per query); `default` sets nothing.  Every library (--libs: file names beside the
package's own, loaded through CAPF_LIB_AB; default: this build) gets ONE
process, which builds both graphs, runs the first (index-building) query, and
then takes the variants in turn, round after round (--rounds ≥ 2): per variant
two warm-up queries and --reps timed ones, each plan → scalar bracketed by a
device sync, and one profiled query for P3's device time and the job
counters.  One JSON line per (library, graph, variant) with the medians of
the rounds goes to stdout and, with --out, is appended to FILE.  The counts of
a graph must be equal across variants and libraries."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_VARIANTS = "default;" + ";".join(
    [f"split{j}_tiles{t}:CAPF_C5_JOB_SPLIT={j},CAPF_C5_STEAL_TILES={t}" for j in (2, 4, 8) for t in (16, 32, 64)] +
    [f"excess{x}_tiles{t}:CAPF_C5_EXCESS_SPLIT={x},CAPF_C5_STEAL_TILES={t}" for x in (0, 1, 2, 4, 8) for t in (16, 32, 64)])
KNOBS = ("CAPF_C5_JOB_SPLIT", "CAPF_C5_STEAL_TILES", "CAPF_C5_EXCESS_SPLIT")


def parse_variants(spec):
    out = []
    for v in spec.split(";"):
        name, _, sets = v.partition(":")
        out.append((name, dict(kv.split("=") for kv in sets.split(",") if kv)))
    return out


def skewed_graph(s, scale, m):
    import numpy as np
    from capf_amd.expr import T_INT
    from capf_amd.graph import ElementTable, ScanGraph
    from capf_amd.table import compact_as
    from oracle import nodemix
    n = 1 << scale
    h = nodemix.node_mix(np.arange(n, dtype=np.int64), scale)
    pool = np.nonzero((h >> 16) == 77)[0].astype(np.int64)[:40000]
    rng = np.random.default_rng(41)
    src = rng.integers(0, n, m)
    heavy = rng.random(m) < 0.6
    src[heavy] = pool[rng.integers(0, len(pool), int(heavy.sum()))]
    del heavy
    dst = rng.integers(0, n, m)
    rels = s.table([("id", T_INT, np.arange(m), None), ("source", T_INT, src, None), ("target", T_INT, dst, None)])
    nodes = s.range_nodes(0, n, id_col="id")
    return ScanGraph(s, [ElementTable("node", frozenset(["V"]), compact_as(nodes, 3), {})],
                     [ElementTable("rel", frozenset(["E"]), compact_as(rels, 3), {})])


def child(lib, variants, rounds, reps, scale, result):
    sys.path.insert(0, ROOT)
    import capf_import
    capf_import.load()
    from capf_amd.expr import CountStar
    from capf_amd.planner import Match, NodeP, Query, RelP, Stage, run
    from capf_amd.synthetic import rmat_graph
    from capf_amd.table import GpuSession

    q = Query([Match([NodeP("a"), NodeP("b"), NodeP("c")], [RelP("r1", "a", "b"), RelP("r2", "b", "c")])],
              [Stage([("count", CountStar())])])
    s = GpuSession(0)
    m = 16 << scale
    recs = []
    for gname in ("rmat", "skewed"):
        g = rmat_graph(s, scale, 16, compact=3) if gname == "rmat" else skewed_graph(s, scale, m)
        step = lambda: run(g, q)[0]["count"]  # noqa: E731
        for k in KNOBS:
            os.environ.pop(k, None)
        first = step()  # builds the index
        per = {name: {"ms": [], "p3_ms": [], "jobs": [], "steals": []} for name, _ in variants}
        for _ in range(rounds):
            for name, sets in variants:
                for k in KNOBS:
                    os.environ.pop(k, None)
                os.environ.update(sets)
                ts = []
                for i in range(2 + reps):
                    s.sync()
                    t0 = time.perf_counter()
                    c = step()
                    dt = time.perf_counter() - t0
                    assert c == first, (gname, name, c, first)
                    if i >= 2:
                        ts.append(dt * 1e3)
                s.reset_profile()
                s.set_profiling(True)
                assert step() == first
                s.set_profiling(False)
                prof = s.profile()
                per[name]["ms"].append(statistics.median(ts))
                per[name]["p3_ms"].append(prof["c5_gather"]["total_ms"])
                per[name]["jobs"].append(prof.get("c5_jobs", {"bytes": 0.0})["bytes"])
                per[name]["steals"].append(prof.get("c5_steals", {"bytes": 0.0})["bytes"])
        for name, sets in variants:
            p = per[name]
            rec = {"lib": lib or "libcapf_gpu.so", "graph": gname, "variant": name, "knobs": sets, "count": first,
                   "rounds_ms": [round(x, 4) for x in p["ms"]], "median_ms": round(statistics.median(p["ms"]), 4),
                   "p3_ms": [round(x, 4) for x in p["p3_ms"]], "jobs": p["jobs"], "steals": p["steals"]}
            print(json.dumps(rec), flush=True)
            recs.append(rec)
        del g
    with open(result, "w") as f:
        json.dump(recs, f)
    return 0


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], parse_variants(args[2]), int(args[3]), int(args[4]), int(args[5]), args[6])
    opt = {"--libs": "", "--variants": DEFAULT_VARIANTS, "--rounds": "2", "--reps": "9", "--scale": "24", "--out": ""}
    for flag in list(opt):
        if flag in args:
            i = args.index(flag)
            opt[flag] = args[i + 1]
            del args[i:i + 2]
    rounds = max(2, int(opt["--rounds"]))
    counts = {}
    for lib in opt["--libs"].split(","):
        env = dict(os.environ)
        if lib:
            env["CAPF_LIB_AB"] = lib
        with tempfile.TemporaryDirectory() as tmp:
            result = os.path.join(tmp, "result.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", lib, opt["--variants"], str(rounds),
                   opt["--reps"], opt["--scale"], result]
            rc = subprocess.run(cmd, env=env, timeout=900).returncode
            if rc != 0:  # nothing more is started on the GPU
                print(f"{lib or 'this build'}: ended with status {rc}", flush=True)
                return 1
            recs = json.load(open(result))
        for r in recs:
            assert counts.setdefault(r["graph"], r["count"]) == r["count"], "counts differ between variants"
        if opt["--out"]:
            with open(opt["--out"], "a") as f:
                for r in recs:
                    f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
