"""LIST, DATE and LOCALDATETIME columns through the distributed Table layer
(dist_table.py GpuExchange): ONE spawn of two ranks on cuda:0 under gloo
(host-staged all-to-alls; RCCL refuses two ranks on one device) runs every
check, each rank reporting its failures per check through the queue.

 a. the reference cases marked `local_only` (LIST property columns) through
    dist_scan_graph, int64 and FOR24 element tables;
 b. shuffle / to_root / replicate of a table with an INT key, a DATE, a
    LOCALDATETIME (values before 1970), a nullable LIST<INT> and a LIST<STRING>;
 c. join (both sides shuffled), distinct, group + collect + orderBy and a
    global min / max of a DATE against the same operator on the local session;
 d. the dictionary check for LIST<STRING> after one rank interned alone.
"""
import os
import socket

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LOCAL_ONLY = 4


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _row_key(row):
    return tuple((c, tuple(v) if isinstance(v, list) else v) for c, v in sorted(row.items()))


def _bag(rows):
    return sorted((_row_key(r) for r in rows), key=repr)


def _worker(rank, world, port, q):
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import datetime
    import traceback
    import torch
    import torch.distributed as dist
    bad, ran = [], []
    try:
        import capf_import  # noqa: F401
        from conftest import case_parts, check_case
        from reference_cases import CASES
        from capf_amd import _lib
        from capf_amd.dist_table import DistSession, DistTable, GpuExchange, dist_scan_graph
        from capf_amd.expr import T_INT, T_STRING, Collect, Max, Min, Var
        from capf_amd.graph import ScanGraph
        from capf_amd.header import RecordHeader
        from capf_amd.planner import run
        from capf_amd.table import GpuSession
        from oracle.create_parser import parse_create
        T_LIST, T_DATE, T_LDT = 5, 6, 7
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90))
        s = GpuSession.on_torch_stream(0)
        ex = GpuExchange(s)
        ds = DistSession(s, ex)

        def check(name, fn):
            """Both ranks run fn (every exchange is collective); a failure is
            recorded and the next check still runs."""
            ran.append(name)
            try:
                msg = fn()
                if msg:
                    bad.append((name, str(msg)[:400]))
            except Exception as e:  # noqa: BLE001 - reported per check
                bad.append((name, repr(e)[:400]))

        # ---- a. the local_only reference cases
        local_only = [c for c in CASES if case_parts(c)[5].get("local_only")]
        ran.append(("n_local_only", len(local_only)))
        for compact in (False, 3):
            for case in local_only:
                cid, src, create, query, expected, opts = case_parts(case)

                def one(create=create, query=query, expected=expected, opts=opts, compact=compact):
                    full = ScanGraph.from_data(s, parse_create(create), compact=compact)
                    got = run(dist_scan_graph(ds, full), query, opts.get("params"))
                    return None if check_case(got, expected, opts) else f"got {got}"
                check(f"case:{cid}:{compact}", one)

        # ---- b. table-level moves
        n = 203
        d0 = datetime.date(1970, 1, 1)
        t0 = datetime.datetime(1970, 1, 1)
        keys = [i % 37 for i in range(n)]
        dates = [None if i % 11 == 0 else d0 + datetime.timedelta(days=(i * 997) % 40_000 - 20_000) for i in range(n)]
        stamps = [t0 + datetime.timedelta(seconds=i * 7_777_777 - 600_000_000, microseconds=i) for i in range(n)]
        ints = [None if i % 7 == 0 else [] if i % 7 == 1 else [None if j == 2 else i * 1000 + j for j in range(i % 5 + 1)]
                for i in range(n)]
        strs = [["w%d" % ((i + j) % 13) for j in range(i % 4)] for i in range(n)]
        columns = [("k", T_INT, keys, None), ("d", T_DATE, dates, None), ("ts", T_LDT, stamps, None),
                   ("xs", T_LIST, ints, None), ("ss", T_LIST, strs, None), ("row", T_INT, list(range(n)), None)]
        full = s.table(columns)                      # the single-process table
        want = _bag(full.rows)
        want_types = {c: full.capf_type(c) for c in full.physicalColumns}
        root = ds.table(columns)                     # rank 0 keeps the rows
        assert root.local.size == (n if rank == 0 else 0)

        def types_kept(t):
            got = {c: t.capf_type(c) for c in t.physicalColumns}
            return None if got == want_types else f"types {got}"

        def gathered(local):
            return [r for part in ex.all_gather_obj(local.rows) for r in part]

        def shuffle():
            moved = ex.shuffle(root.local, ["k"])
            rows = moved.rows
            owners = ex.all_gather_obj(sorted({r["k"] for r in rows}))
            if set(owners[0]) & set(owners[1]):
                return f"keys on both ranks: {set(owners[0]) & set(owners[1])}"
            if not owners[0] or not owners[1]:
                return "one rank received nothing: the shuffle did not spread the rows"
            return types_kept(moved) or (None if _bag(gathered(moved)) == want else "rows differ")
        check("shuffle", shuffle)

        def to_root():
            # from a hash placement back to rank 0: rank 1 receives zero rows and still takes part
            moved = ex.to_root(ex.shuffle(root.local, ["k"]))
            if moved.size != (n if rank == 0 else 0):
                return f"rank {rank} holds {moved.size} rows"
            return types_kept(moved) or (None if rank or _bag(moved.rows) == want else "rows differ")
        check("to_root", to_root)

        def replicate():
            moved = ex.replicate(root.local)
            return types_kept(moved) or (None if _bag(moved.rows) == want else "rows differ")
        check("replicate", replicate)

        def replicate_hashed():
            moved = ex.replicate(ex.shuffle(root.local, ["row"]))
            return types_kept(moved) or (None if _bag(moved.rows) == want else "rows differ")
        check("replicate_hashed", replicate_hashed)

        def int64_min():
            # a column and a list holding only INT64_MIN: −min does not fit the all-reduce's int64
            lo = -(1 << 63)
            cols = [("k", T_INT, list(range(50)), None), ("m", T_INT, [lo] * 50, None),
                    ("ms", T_LIST, [[lo] * (i % 3) for i in range(50)], None),
                    ("near", T_INT, [lo + i % 7 for i in range(50)], None)]
            moved = ex.shuffle(ds.table(cols).local, ["k"])
            return None if _bag(gathered(moved)) == _bag(s.table(cols).rows) else f"rows differ: {moved.rows[:2]}"
        check("int64_min_column_and_list", int64_min)

        def own_share_list_key():
            # keys that are all LIST columns route nothing: rank 0 keeps every row
            mine = ex.own_share(full, ["xs"])
            return None if mine.size == (n if rank == 0 else 0) else f"rank {rank} keeps {mine.size}"
        check("own_share_list_key", own_share_list_key)

        def element_types_differ():
            # LIST<INTEGER> on rank 0, LIST<FLOAT> on rank 1: refused on BOTH ranks, before any
            # rank waits in a collective the other never enters
            elems = [[1, 2], [3]] if rank == 0 else [[1.5, 2.5], [3.5]]
            t = s.table([("k", T_INT, [1, 2], None), ("xs", T_LIST, elems, None)])
            try:
                ex.shuffle(t, ["k"])
            except _lib.IllegalStateException as e:
                return None if "different types" in str(e) else str(e)
            return "no error"
        check("element_types_differ", element_types_differ)

        # ---- c. operators against the single-process session
        hdr = RecordHeader({Var(c): c for c in ("k", "d", "ts", "xs", "ss", "row", "k2", "v", "row2")})
        hashed = DistTable(ds, ex.shuffle(root.local, ["row"]), part={"row"})
        rcols = [("k2", T_INT, list(range(37)), None),
                 ("v", T_LIST, [[i, i + 1] if i % 3 else None for i in range(37)], None),
                 ("row2", T_INT, list(range(37)), None)]
        right_full = s.table(rcols)
        right = DistTable(ds, ex.shuffle(ds.table(rcols).local, ["row2"]), part={"row2"})

        def join():
            # neither side partitioned on the key; |right| · G ≥ |left| is false here, so force the
            # co-partitioned plan with a full outer join (never broadcast): both sides shuffle
            got = hashed.join(right, "full_outer", ("k", "k2"))
            exp = full.join(right_full, "full_outer", ("k", "k2"))
            return None if _bag(got.rows) == _bag(exp.rows) else "rows differ"
        check("join_shuffles_both_sides", join)

        def inner_join():
            got = hashed.join(right, "inner", ("k", "k2"))
            exp = full.join(right_full, "inner", ("k", "k2"))
            return None if _bag(got.rows) == _bag(exp.rows) else "rows differ"
        check("join_inner", inner_join)

        def distinct():
            # every row twice: whichever representative a key keeps, its list is the same
            both = hashed.select("row", "xs", "ss").unionAll(hashed.select("row", "xs", "ss"))
            got = both.distinct("row")                         # partitioned on the key: local
            got2 = DistTable(ds, both.local).distinct("row")   # partition unknown: shuffles by the key
            exp = _bag(full.select("row", "xs", "ss").rows)
            for g in (got, got2):
                if _bag(g.rows) != exp:
                    return "rows differ"
            return None
        check("distinct_carries_list", distinct)

        def collect_order():
            aggs = {"rows": Collect(Var("row"))}
            got = hashed.group([Var("k")], aggs, header=hdr, params={}).orderBy((Var("k"), "asc"), header=hdr)
            exp = full.group([Var("k")], aggs, header=hdr, params={}).orderBy((Var("k"), "asc"), header=hdr)
            if got.placement != "root":
                return got.placement
            g, e = got.rows, exp.rows
            if [r["k"] for r in g] != [r["k"] for r in e]:
                return f"order {[r['k'] for r in g][:8]}"
            return None if [sorted(r["rows"]) for r in g] == [sorted(r["rows"]) for r in e] else "lists differ"
        check("group_collect_orderBy", collect_order)

        def date_min_max():
            aggs = {"lo": Min(Var("d")), "hi": Max(Var("d")), "first": Min(Var("ts"))}
            got = hashed.group([], aggs, header=hdr, params={})
            exp = full.group([], aggs, header=hdr, params={}).rows
            if {c: got.capf_type(c) for c in ("lo", "hi", "first")} != {"lo": T_DATE, "hi": T_DATE, "first": T_LDT}:
                return "types"
            return None if got.rows == exp and exp[0]["lo"] < d0 < exp[0]["hi"] else f"{got.rows} vs {exp}"
        check("date_min_max", date_min_max)

        # ---- d. the dictionary check covers LIST<STRING> elements (last: the dictionaries differ afterwards)
        def dictionaries():
            only_lists = root.local.select("row", "ss")  # no STRING column, only LIST<STRING>
            if rank == 1:
                s.intern("a string rank 1 alone has seen")
            try:
                ex.shuffle(only_lists, ["row"])
            except _lib.IllegalStateException as e:
                return None if "string dictionaries differ" in str(e) else str(e)
            return "no error"
        check("dictionary_check", dictionaries)
        assert T_STRING == 4
        q.put((rank, bad, ran))
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001 - report, do not hang the parent
        q.put((rank, bad + [("worker", traceback.format_exc()[-1500:])], ran))


@pytest.mark.timeout(300)
def test_lists_and_temporals_move_between_ranks():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=240) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=20)
            if p.is_alive():
                p.kill()
    for rank, bad, ran in res:
        print(f"rank {rank}: ran {len(ran)} checks, {len(bad)} failing")
        assert not bad, f"rank {rank}: {len(bad)} failing: {bad}"
        assert ("n_local_only", N_LOCAL_ONLY) in ran, ran  # none skipped
        names = [x for x in ran if isinstance(x, str)]
        assert sum(x.startswith("case:") for x in names) == 2 * N_LOCAL_ONLY
        for name in ("shuffle", "to_root", "replicate", "int64_min_column_and_list", "own_share_list_key",
                     "element_types_differ", "join_shuffles_both_sides", "distinct_carries_list",
                     "group_collect_orderBy", "date_min_max", "dictionary_check"):
            assert name in names, (name, names)
