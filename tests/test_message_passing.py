"""The message-passing count (fused_count.hip tree_count), path by path.

count(*) over an acyclic inner-join tree is answered by one integer, so every
case here pins down WHICH code answered — `last_plan()` must be
"message_passing" and `last_plan_detail()` must name the expected message
kinds and root kernel (DESIGN.md "Plan detail") — and compares the integer
with exact host arithmetic: a dynamic programme over the tree in Python ints
(`dp_count`), numpy set arithmetic for the two inputs too large for it, brute
force or the oracle's materialised joins where inequalities are involved.
Every comparison is ==.

The tables go through the Table SPI directly: `session.table`, lazy inner
`join`s, `filter` for the r_i <> r_j predicates; the count is read through
`.size`, `group([], {count(*)})` and `count_async`, which must agree.

Which table is the root: the engine roots the tree at its centre, the first
leaf (in join order, left to right) of least eccentricity.  For two tables that
is the LEFT one; the right one sends the message, keyed by the left key
column's [min, max].
"""
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

from capf_amd.expr import CountStar, Equals, GreaterThan, IntegerLit, Not, T_INT, Var
from capf_amd.header import RecordHeader
from conftest import bag
from oracle.table_np import OracleSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN, MAX = -(1 << 63), (1 << 63) - 1
PLAN = "message_passing"


# ------------------------------------------------------------------ key_range.h
KEY_RANGE_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "key_range.h"
int main(int argc, char **argv) {
  for (int i = 1; i + 1 < argc; i += 2) {
    const capf::KeyRange r = capf::key_range(strtoll(argv[i], nullptr, 10), strtoll(argv[i + 1], nullptr, 10));
    printf("%llu %d %d\n", (unsigned long long)r.n, (int)r.wide,
           (int)capf::key_range_fits(strtoll(argv[i], nullptr, 10), strtoll(argv[i + 1], nullptr, 10), 1ull << 28));
  }
}
"""


def test_key_range_under_ubsan(tmp_path):
    """csrc/key_range.h, compiled alone with the host compiler and
    -fsanitize=undefined (any report aborts): the number of keys in [lo, hi]
    for the pairs where `(uint64_t)(max - min) + 1` overflowed or wrapped."""
    pairs = [(MIN, MAX), (MIN, MIN), (MAX, MAX), (-1, 0), (0, (1 << 28) - 1), (0, 1 << 28), (5, 4), (MIN, -1),
             (MIN, 0), (-1, MAX)]
    src = tmp_path / "key_range_main.cpp"
    src.write_text(KEY_RANGE_MAIN)
    exe = tmp_path / "key_range_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "cypher-for-apache-flink_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)] + [str(x) for p in pairs for x in p], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    want = []
    for lo, hi in pairs:
        n = hi - lo + 1 if hi >= lo else 0  # Python ints: exact
        wide = n > (1 << 64) - 1
        want.append(((1 << 64) - 1 if wide else n, int(wide), int(not wide and 0 < n <= 1 << 28)))
    assert got == want
    assert got[0] == ((1 << 64) - 1, 1, 0) and got[4] == (1 << 28, 0, 1) and got[5] == ((1 << 28) + 1, 0, 0)


# ------------------------------------------------------------------ the reference
def K(vals, nulls=None):
    """One key column: (int64 values, validity or None)."""
    v = np.array(vals, dtype=np.int64)
    return v, (None if nulls is None else ~np.asarray(nulls, dtype=bool))


def nrows(table):
    return len(next(iter(table.values()))[0])


def dp_count(tables, edges, root=0):
    """count(*) of the inner equi-join tree: tables = [{column: (values,
    valid)}], edges = [(table a, column, table b, column)].  Weighted
    histograms passed leaf to root, in Python ints; NULL never joins."""
    adj = {i: [] for i in range(len(tables))}
    for a, ca, b, cb in edges:
        adj[a].append((b, ca, cb))
        adj[b].append((a, cb, ca))

    def keys(t, c):
        v, ok = tables[t][c]
        v = v.tolist()
        return v if ok is None else [x if o else None for x, o in zip(v, ok.tolist())]

    def weights(v, parent):
        w = [1] * nrows(tables[v])
        for u, mine, theirs in adj[v]:
            if u == parent:
                continue
            m = message(u, v, theirs)
            w = [wi * m.get(k, 0) if k is not None else 0 for wi, k in zip(w, keys(v, mine))]
        return w

    def message(v, parent, col):
        m = {}
        for wi, k in zip(weights(v, parent), keys(v, col)):
            if k is not None and wi:
                m[k] = m.get(k, 0) + wi
        return m

    return sum(weights(root, -1))


# ------------------------------------------------------------------ the engine
def gpu_tables(session, tables, enc=None):
    """enc: None (int64), 4 (FOR32), 3 (FOR24), or one of them per table."""
    out = []
    for i, t in enumerate(tables):
        cols = [(c, T_INT, v, None if ok is None else ok.astype(np.uint8)) for c, (v, ok) in t.items()]
        g = session.table(cols, nrows=nrows(t))
        e = enc[i] if isinstance(enc, (list, tuple)) else enc
        out.append(g.compact(e) if e else g)
    return out


def join_tree(tabs, edges, start=None):
    """Left-deep inner joins from table `start` (default: the first edge's
    first table), each edge as soon as one of its sides is in."""
    start = edges[0][0] if start is None else start
    cur, seen, todo = tabs[start], {start}, list(edges)
    while todo:
        for e in todo:
            a, ca, b, cb = e
            if a in seen and b not in seen:
                cur = cur.join(tabs[b], "inner", (ca, cb))
                seen.add(b)
            elif b in seen and a not in seen:
                cur = cur.join(tabs[a], "inner", (cb, ca))
                seen.add(a)
            else:
                continue
            todo.remove(e)
            break
        else:
            raise AssertionError("edges do not form a connected tree")
    return cur


def norm(detail):
    return detail.replace("bits_cached", "bits")


def read3(session, make):
    """(count, plan, detail) of make().size; group(∅, count(*)) and
    count_async over fresh copies of the same lazy table must agree with it
    and take the same plan (a cached bitmap aside)."""
    import torch
    session.reset_profile()
    n = make().size
    plan, detail = session.last_plan(), session.last_plan_detail()
    session.reset_profile()
    assert make().group([], {"c": CountStar()}).rows == [{"c": n}]
    assert (session.last_plan(), norm(session.last_plan_detail())) == (plan, norm(detail))
    slot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    session.reset_profile()
    make().count_async(slot.data_ptr())
    session.sync()
    assert int(slot.item()) == n
    assert (session.last_plan(), norm(session.last_plan_detail())) == (plan, norm(detail))
    return n, plan, detail


def check_tree(session, tables, edges, detail, enc=None, where=""):
    """The tree counts what dp_count says, by message passing, along `detail`
    (None: any)."""
    tabs = gpu_tables(session, tables, enc)
    got, plan, d = read3(session, lambda: join_tree(tabs, edges))
    assert plan == PLAN, (where, plan)
    if detail is not None:
        assert d == detail, (where, d)
    assert got == dp_count(tables, edges), (where, d)
    return d


# ------------------------------------------------------------------ message kinds
RNG = np.random.default_rng(20240607)
SPARSE_POOL = RNG.choice(10 ** 12, size=600, replace=False).astype(np.int64)  # range > 2^34
MID_POOL = RNG.choice(1 << 20, size=600, replace=False).astype(np.int64)  # 16·1024 < range < 2^28


def kind_case(kind, variation):
    """(root keys, sender keys, expected message token) of a two-table join
    whose right table sends a `kind` message; the root keys always stray
    outside the sender's so no child is dropped."""
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{variation}".encode()))
    n = 700
    if kind == "ones":  # a dense unique range, shuffled
        send = rng.permutation(np.arange(100, 500))
        root = rng.integers(90, 510, n)
        root[:2] = [90, 509]
    elif kind == "bits":  # unique, gapped
        send = rng.permutation(3 * np.arange(400) + 7)
        root = rng.integers(0, 1300, n)
    elif kind == "dense":  # repeated keys over a compact range
        send = rng.integers(0, 200, 500)
        root = rng.integers(-5, 230, n)
    elif kind == "hash_wide":  # root key range > 2^28 (and > 2^34: no bitmap either)
        send = SPARSE_POOL[rng.integers(0, 500, 450)]
        root = SPARSE_POOL[rng.integers(0, 600, n)]
    else:  # hash_mid: 16·max(rows, 1024) < root key range < 2^28; repeated sender keys rule the bitmap out
        assert kind == "hash_mid"
        send = MID_POOL[rng.integers(0, 500, 450)]
        root = MID_POOL[rng.integers(0, 600, n)]
        root[:2] = [0, (1 << 20) - 1]
    send, root = send.astype(np.int64), root.astype(np.int64)
    send_nulls = root_nulls = None
    token = kind.split("_")[0]
    if variation == "sender_nulls":
        send_nulls = rng.random(len(send)) < 0.2
        send_nulls[0] = True
        if kind == "ones":
            token = "bits"  # a key column with NULLs is no dense range: the leaf sends its bitmap
    elif variation == "parent_nulls":
        root_nulls = rng.random(n) < 0.2
        root_nulls[-1] = True
    elif variation == "sender_outside":
        lo, hi = int(root.min()), int(root.max())
        if kind == "ones":  # stays a dense range, now wider than the root's keys on one side
            send = rng.permutation(np.arange(100, 900)).astype(np.int64)
        else:
            extra = np.array([lo - 1, lo - 1000, hi + 1, hi + 12345, lo - 1, hi + 1], dtype=np.int64)
            if kind == "bits":
                extra = np.unique(extra)
            send = np.concatenate([send, extra])
    return K(root, root_nulls), K(send, send_nulls), token


@pytest.mark.gpu
@pytest.mark.parametrize("variation", ["plain", "sender_nulls", "parent_nulls", "sender_outside"])
@pytest.mark.parametrize("kind", ["ones", "bits", "dense", "hash_wide", "hash_mid"])
def test_message_kinds(gpu_session, kind, variation):
    root, send, token = kind_case(kind, variation)
    if kind == "hash_wide":
        assert int(root[0].max()) - int(root[0].min()) + 1 > 1 << 34
    if kind == "hash_mid":
        assert 16 * 1024 < int(root[0].max()) - int(root[0].min()) + 1 < 1 << 28
    # a nullable root key, or a counted (dense / hash) message: the generic kernel
    rootk = f"root1:{token}:w8" if root[1] is None and token in ("ones", "bits") else "generic:1"
    gpu_session.reset_profile()
    assert gpu_session.last_plan_detail() == "" and gpu_session.last_plan() == "none"
    check_tree(gpu_session, [{"rk": root}, {"sk": send}], [(0, "rk", 1, "sk")], f"{token} {rootk}")


@pytest.mark.gpu
@pytest.mark.parametrize("variation", ["plain", "sender_nulls", "sender_outside"])
@pytest.mark.parametrize("root", ["all_null", "zero_rows", "filtered_away"])
def test_empty_message(gpu_session, root, variation):
    """The parent's key column holds no value — all NULL, no rows, or no row
    left by its pushed predicate: the sender's message is the empty map."""
    send = 3 * np.arange(300, dtype=np.int64) + 7
    send_nulls = None
    if variation == "sender_nulls":
        send_nulls = np.arange(300) % 5 == 0
    if variation == "sender_outside":
        send = np.concatenate([send, [MIN, MAX]]).astype(np.int64)
    n = 0 if root == "zero_rows" else 40
    rk = K(np.arange(n, dtype=np.int64) * 3 + 7, np.ones(n, dtype=bool) if root == "all_null" else None)
    tables = [{"rk": rk, "rw": K(np.arange(n))}, {"sk": K(send, send_nulls)}]
    tabs = gpu_tables(gpu_session, tables)
    if root == "filtered_away":
        h = RecordHeader({Var(c): c for c in ("rk", "rw")})
        tabs[0] = tabs[0].filter(GreaterThan(Var("rw"), IntegerLit(1000)), h, {})
    got, plan, detail = read3(gpu_session, lambda: tabs[0].join(tabs[1], "inner", ("rk", "sk")))
    assert (got, plan) == (0, PLAN)
    # no rows at all: the empty map over no rows is "every row counts once"
    assert detail == {"all_null": "empty generic:1", "zero_rows": "empty all_rows",
                      "filtered_away": "empty no_rows"}[root]


# ------------------------------------------------------------------ root kernels
SIZES = [0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1027]
WIDTH = {None: 8, 4: 4, 3: 3}
ENC_ID = {None: 0, 4: 1, 3: 2}


def tail_hits(keys, hit, n):
    """The last rows (the ragged tail of every vector width) all carry a hit
    while the body hits about every other row: a dropped tail or one counted
    twice changes the sum."""
    keys[max(0, n - 7):] = hit
    return keys


def bits_child(base=0):
    return K(np.random.default_rng(5).permutation(3 * np.arange(400) + 7 + base))


def ones_child(base=0):
    return K(np.random.default_rng(6).permutation(np.arange(100, 500) + base))


def dense_child(base=0):
    """Repeated keys; key base + 150 occurs 7 times (the tail rows' weight), the rest 1..3 times."""
    rng = np.random.default_rng(7)
    body = np.concatenate([np.repeat(np.arange(0, 100), 1), np.repeat(np.arange(100, 140), 3),
                           np.repeat([150], 7)]) + base
    return K(rng.permutation(body))


def root_keys(kind, n, base, rng):
    """Root keys against a `kind` child at `base`.  Against a 0/1 child row 0
    strays outside the child's range (an all-ones child is then kept, not
    dropped); against a counted child every size holds the 7-fold key, so the
    sender's keys repeat inside the root's key range however few rows it has."""
    if kind == "bits":
        k = tail_hits(rng.integers(0, 1300, n) + base, 3 * 17 + 7 + base, n)
    elif kind == "ones":
        k = tail_hits(rng.integers(90, 520, n) + base, 321 + base, n)
    else:
        k = tail_hits(rng.integers(-3, 160, n) + base, 150 + base, n)
    if n and kind != "dense":
        k[0] = base + (95 if kind == "ones" else -3)
    return k.astype(np.int64)


def child_of(kind, base):
    return {"bits": bits_child, "ones": ones_child, "dense": dense_child}[kind](base)


@pytest.mark.gpu
@pytest.mark.parametrize("enc", [None, 4, 3], ids=["w8", "w4", "w3"])
@pytest.mark.parametrize("kind", ["bits", "ones"])
def test_root1(gpu_session, kind, enc):
    """k_message_root1<kind, width>: one remaining child, 8 rows in flight, ragged tail."""
    for n in SIZES:
        rng = np.random.default_rng(n)
        tables = [{"rk": K(root_keys(kind, n, 1000, rng))}, {"sk": child_of(kind, 1000)}]
        if n:
            assert gpu_tables(gpu_session, tables[:1], enc)[0].encoding("rk")[0] == ENC_ID[enc]
        want = f"{kind} root1:{kind}:w{WIDTH[enc]}" if n else ("ones" if kind == "ones" else "empty") + " all_rows"
        check_tree(gpu_session, tables, [(0, "rk", 1, "sk")], want, enc=[enc, None], where=f"n={n}")


def star2(ka, kb, n, nulls=False):
    """Root(ra, rb) with children A(ak) and B(bk) at different bases."""
    rng = np.random.default_rng(100 + n)
    ra, rb = root_keys(ka, n, 1000, rng), root_keys(kb, n, 70000, rng)
    rnull = None
    if nulls and n:  # a validity mask at every size; a NULL from 3 rows on, never in the last row
        rnull = rng.random(n) < 0.25
        rnull[n // 2] = n >= 3
        rnull[n - 1] = False
    tables = [{"ra": K(ra, rnull), "rb": K(rb)}, {"ak": child_of(ka, 1000)}, {"bk": child_of(kb, 70000)}]
    return tables, [(0, "ra", 1, "ak"), (0, "rb", 2, "bk")]


def star_tokens(kinds, n, rootk):
    if n:
        return " ".join(kinds) + " " + rootk
    # no root rows: no key range, so nothing but a dense range (known from the sender alone) has a kind
    return " ".join("ones" if k == "ones" else "empty" for k in kinds) + " all_rows"


@pytest.mark.gpu
@pytest.mark.parametrize("ka,kb", [("bits", "bits"), ("bits", "ones"), ("ones", "bits"), ("ones", "ones")])
def test_root2_f32(gpu_session, ka, kb):
    """k_message_root2_f32<kindA, kindB>: both root key columns FOR32 with different bases."""
    for n in SIZES:
        tables, edges = star2(ka, kb, n)
        if n:
            t = gpu_tables(gpu_session, tables[:1], 4)[0]
            ea, eb = t.encoding("ra"), t.encoding("rb")
            assert ea[0] == eb[0] == 1 and ea[1] != eb[1]
        check_tree(gpu_session, tables, edges, star_tokens((ka, kb), n, f"root2_f32:{ka},{kb}"), enc=4, where=f"n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("ka,kb,enc", [(a, b, e) for e in (None, 3) for a in ("bits", "ones") for b in ("bits", "ones")] +
                         [(a, b, e) for e in (None, 3, 4) for a, b in (("dense", "bits"), ("ones", "dense"))])
def test_root2(gpu_session, ka, kb, enc):
    """k_message_root2: the same stars on int64 and FOR24 key columns, and with
    a counted (dense) child, which also keeps FOR32 columns off the f32 kernel."""
    for n in SIZES:
        tables, edges = star2(ka, kb, n)
        check_tree(gpu_session, tables, edges, star_tokens((ka, kb), n, "root2"), enc=enc, where=f"n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("enc", [None, 4, 3], ids=["int64", "for32", "for24"])
def test_generic_root(gpu_session, enc):
    """k_message at the root: a nullable key column; three children."""
    for n in SIZES:
        tables, edges = star2("bits", "ones", n, nulls=True)
        check_tree(gpu_session, tables, edges, star_tokens(("bits", "ones"), n, "generic:2"), enc=enc,
                   where=f"nullable n={n}")
        tables, edges = star2("bits", "dense", n)
        rng = np.random.default_rng(n)
        tables[0]["rc"] = K(root_keys("ones", n, -400, rng))
        tables.append({"ck": ones_child(-400)})
        edges = edges + [(0, "rc", 3, "ck")]
        check_tree(gpu_session, tables, edges, star_tokens(("bits", "dense", "ones"), n, "generic:3"), enc=enc,
                   where=f"three n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bits", "ones"])
def test_root1_second_trip_through_the_capped_grid(gpu_session, kind):
    """The root grid is capped at 16 blocks per CU; 256 threads × 8 rows each
    cover CUs · 32768 rows per trip.  One int64 column just past one trip (its
    last rows in the second trip and the ragged tail), against numpy.isin."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 16 * 256 * 8 + 1027
    rng = np.random.default_rng(11)
    child = child_of(kind, 0)[0]
    root = rng.integers(0, 1300 if kind == "bits" else 560, n).astype(np.int64)
    root[-1027:] = child[rng.integers(0, len(child), 1027)]  # the second trip: all hits
    root[0] = 5000
    want = int(np.isin(root, child).sum())
    assert want > 1027 and want - 1027 < n - 1027
    tabs = gpu_tables(gpu_session, [{"rk": K(root)}, {"sk": K(child)}])
    got, plan, detail = read3(gpu_session, lambda: tabs[0].join(tabs[1], "inner", ("rk", "sk")))
    assert (plan, detail) == (PLAN, f"{kind} root1:{kind}:w8")
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("enc", [4, 3], ids=["for32", "for24"])
def test_bits_partitioned_root(gpu_session, enc):
    """From 2^20 rows a FOR-encoded root key column probes the sender's bitmap
    through the radix-partitioned kernels instead of k_message_root1."""
    n = (1 << 20) + 1027
    rng = np.random.default_rng(12)
    child = child_of("bits", 0)[0]
    root = rng.integers(0, 1300, n).astype(np.int64)
    root[-1027:] = child[rng.integers(0, len(child), 1027)]
    want = int(np.isin(root, child).sum())
    tabs = gpu_tables(gpu_session, [{"rk": K(root)}, {"sk": K(child)}], enc=[enc, None])
    got, plan, detail = read3(gpu_session, lambda: tabs[0].join(tabs[1], "inner", ("rk", "sk")))
    assert (plan, norm(detail)) == (PLAN, "bits bits_partitioned")
    assert got == want


# ------------------------------------------------------------------ the drop rule
@pytest.mark.gpu
@pytest.mark.parametrize("enc", [None, 4], ids=["int64", "for32"])
def test_drop_rule(gpu_session, enc):
    """A root key column that lies wholly inside an all-ones child's range, no
    NULL: the child is dropped.  One row out of range, or one NULL: it is
    kept and the count is one lower."""
    n = 300
    rng = np.random.default_rng(3)
    inside = rng.integers(100, 500, n).astype(np.int64)
    inside[:2] = [100, 499]
    send = ones_child(0)
    edges = [(0, "rk", 1, "sk")]
    w = WIDTH[enc]
    assert dp_count([{"rk": K(inside)}, {"sk": send}], edges) == n
    check_tree(gpu_session, [{"rk": K(inside)}, {"sk": send}], edges, "ones all_rows", enc=enc)
    for stray in (99, 500):
        out = inside.copy()
        out[n // 2] = stray
        assert dp_count([{"rk": K(out)}, {"sk": send}], edges) == n - 1
        check_tree(gpu_session, [{"rk": K(out)}, {"sk": send}], edges, f"ones root1:ones:w{w}", enc=enc)
    nulls = np.zeros(n, dtype=bool)
    nulls[n // 3] = True
    assert dp_count([{"rk": K(inside, nulls)}, {"sk": send}], edges) == n - 1
    check_tree(gpu_session, [{"rk": K(inside, nulls)}, {"sk": send}], edges, "ones generic:1", enc=enc)
    # two children, the all-ones one dropped: the remaining child alone, through root1
    tables = [{"rk": K(inside), "rb": K(root_keys("bits", n, 0, rng))}, {"sk": send}, {"bk": bits_child(0)}]
    check_tree(gpu_session, tables, edges + [(0, "rb", 2, "bk")], f"ones bits root1:bits:w{w}", enc=enc)
    tables[0]["rk"] = K(inside, nulls)
    check_tree(gpu_session, tables, edges + [(0, "rb", 2, "bk")], "ones bits generic:2", enc=enc)


# ------------------------------------------------------------------ column caches
@pytest.mark.gpu
def test_bitmap_cache_follows_the_parent_range(gpu_session):
    """One node table (one column object) probed from two rel tables with
    different key ranges, A, B, A: every count is right whichever bitmap the
    column holds, and a repeat of the last query reuses it."""
    rng = np.random.default_rng(21)
    ids = K(rng.permutation(5 * np.arange(2000) + 3))
    ra = K(rng.integers(0, 4000, 900))
    rb = K(rng.integers(3000, 10100, 1100))
    nodes, ta, tb = gpu_tables(gpu_session, [{"id": ids}, {"ka": ra}, {"kb": rb}])
    want_a = dp_count([{"ka": ra}, {"id": ids}], [(0, "ka", 1, "id")])
    want_b = dp_count([{"kb": rb}, {"id": ids}], [(0, "kb", 1, "id")])
    assert want_a != want_b and want_a and want_b
    seen = []
    for rel, col, want in [(ta, "ka", want_a), (tb, "kb", want_b), (ta, "ka", want_a), (ta, "ka", want_a)]:
        gpu_session.reset_profile()
        got = rel.join(nodes, "inner", (col, "id")).size
        assert gpu_session.last_plan() == PLAN
        assert got == want
        seen.append(gpu_session.last_plan_detail())
    assert seen[0] == "bits root1:bits:w8" and seen[1] == "bits root1:bits:w8"
    assert seen[2] in ("bits root1:bits:w8", "bits_cached root1:bits:w8")
    assert seen[3] == "bits_cached root1:bits:w8"


def _unique_inside_duplicated_outside():
    """ids unique in [0, 1000), every id from 5000 on twice; rel keys A inside
    the unique part, B over both."""
    rng = np.random.default_rng(22)
    ids = np.concatenate([2 * np.arange(400) + 1, np.repeat(5000 + 3 * np.arange(150), 2)]).astype(np.int64)
    ids = rng.permutation(ids)
    ka = rng.integers(0, 1000, 500).astype(np.int64)
    kb = np.concatenate([rng.integers(0, 1000, 300), 5000 + 3 * rng.integers(0, 150, 300), [0, 5600]]).astype(np.int64)
    return ids, ka, kb


@pytest.mark.gpu
def test_uniqueness_is_not_learnt_from_a_partial_range(gpu_session):
    """A bitmap pass over the first parent's key range sees no duplicate; the
    column's duplicates lie outside it.  The next query, over a wider range,
    must count them (weight 2, not the 1 of a membership bitmap)."""
    ids, ka, kb = _unique_inside_duplicated_outside()
    nodes, ta, tb = gpu_tables(gpu_session, [{"id": K(ids)}, {"ka": K(ka)}, {"kb": K(kb)}])
    gpu_session.reset_profile()
    assert ta.join(nodes, "inner", ("ka", "id")).size == int(np.isin(ka, ids).sum())
    assert (gpu_session.last_plan(), gpu_session.last_plan_detail()) == (PLAN, "bits root1:bits:w8")
    want = dp_count([{"kb": K(kb)}, {"id": K(ids)}], [(0, "kb", 1, "id")])
    assert want == int(np.bincount(ids, minlength=6000)[kb].sum()) > int(np.isin(kb, ids).sum())
    got, plan, detail = read3(gpu_session, lambda: tb.join(nodes, "inner", ("kb", "id")))
    assert (plan, detail) == (PLAN, "dense generic:1")
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize("join", [None, "radix"], ids=["dense", "radix"])
def test_join_after_a_partial_range_bitmap_returns_every_match(gpu_session, monkeypatch, join):
    """After the same first query, an inner join built on that id column — by
    the index path and by CAPF_JOIN=radix — returns both rows of every
    duplicated id."""
    if join:
        monkeypatch.setenv("CAPF_JOIN", join)
    ids, ka, kb = _unique_inside_duplicated_outside()
    tables = [{"id": K(ids), "tag": K(np.arange(len(ids)))}, {"ka": K(ka)}, {"kb": K(kb), "row": K(np.arange(len(kb)))}]
    nodes, ta, tb = gpu_tables(gpu_session, tables)
    gpu_session.reset_profile()
    assert ta.join(nodes.select("id"), "inner", ("ka", "id")).size == int(np.isin(ka, ids).sum())
    assert gpu_session.last_plan_detail() == "bits root1:bits:w8"
    o = OracleSession()
    on = o.table([("id", T_INT, ids, None), ("tag", T_INT, np.arange(len(ids)), None)])
    ob = o.table([("kb", T_INT, kb, None), ("row", T_INT, np.arange(len(kb)), None)])
    want = ob.join(on, "inner", ("kb", "id")).rows
    assert bag(tb.join(nodes, "inner", ("kb", "id")).rows) == bag(want)
    assert bag(nodes.join(tb, "inner", ("id", "kb")).rows) == bag(want)


# ------------------------------------------------------------------ inclusion–exclusion
def hub_graph(seed, n_nodes=30, hub=70, extra=60):
    """(ids, src, dst) of rels with self-loops, parallel rels and a hub node
    of in- and out-degree above 64 (a self-loop on it too)."""
    rng = np.random.default_rng(seed)
    src = list(rng.integers(0, n_nodes, extra)) + [0] * hub + list(rng.integers(1, n_nodes, hub))
    dst = list(rng.integers(0, n_nodes, extra)) + list(rng.integers(1, n_nodes, hub)) + [0] * hub
    src += [0, 3, 3, 7, 7, 7]  # self-loops (one on the hub), parallel rels
    dst += [0, 3, 3, 9, 9, 9]
    src, dst = np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64)
    ids = 10 ** 6 + 7 * rng.permutation(len(src)).astype(np.int64)  # unique, gapped, unordered
    return ids, src, dst


def brute_paths(ids, src, dst, joins, forbid=True):
    """#(r1, ..., rk) with pairwise different rels, r_i.<a> = r_{i+1}.<b> for
    (a, b) = joins[i]; a, b in "st"."""
    col = {"s": src.tolist(), "t": dst.tolist()}
    m = len(ids)
    total = 0

    def extend(path):
        nonlocal total
        if len(path) == len(joins) + 1:
            total += 1
            return
        a, b = joins[len(path) - 1]
        v = col[a][path[-1]]
        for r in index[b].get(v, ()):
            if not forbid or r not in path:
                extend(path + [r])

    index = {c: {} for c in "st"}
    for c in "st":
        for r in range(m):
            index[c].setdefault(col[c][r], []).append(r)
    for r in range(m):
        extend([r])
    return total


def rel_chain(rels, joins, hops, with_nodes=None):
    """rels scanned `hops` times (columns i<k>, s<k>, t<k>), joined in a chain
    by `joins`, all r_i <> r_j filters on top; with_nodes: a node table joined
    to the chain's first start and last end column."""
    scans = [rels.select(("id", f"i{k}"), ("s", f"s{k}"), ("t", f"t{k}")) for k in range(hops)]
    cur = scans[0]
    if with_nodes is not None:
        cur = with_nodes.select(("id", "na")).join(cur, "inner", ("na", "s0"))
    for k, (a, b) in enumerate(joins):
        cur = cur.join(scans[k + 1], "inner", (f"{a}{k}", f"{b}{k + 1}"))
    if with_nodes is not None:
        cur = cur.join(with_nodes.select(("id", "nz")), "inner", (f"t{hops - 1}", "nz"))
    names = [f"{c}{k}" for k in range(hops) for c in "ist"] + ["na", "nz"]
    h = RecordHeader({Var(c): c for c in names})
    for x in range(hops):
        for y in range(x + 1, hops):
            cur = cur.filter(Not(Equals(Var(f"i{x}"), Var(f"i{y}"))), h, {})
    return cur


@pytest.mark.gpu
@pytest.mark.parametrize("enc", [None, 4], ids=["int64", "for32"])
@pytest.mark.parametrize("joins", [[("t", "s"), ("t", "s")], [("t", "t"), ("s", "s")], [("s", "s"), ("t", "s")]],
                         ids=["directed", "out-in-out", "in-out-out"])
def test_three_hop_inclusion_exclusion(gpu_session, joins, enc):
    """Three scans of one rel table, 3 uniqueness filters, 8 terms; each
    r_i = r_j term merges two scans into one leaf.

    In the `directed` and `out-in-out` orientations the r1 = r3 term joins
    the merged scan to the middle scan on two keys at once (r1.t = r2.s AND
    r2.t = r1.s: the 2-cycles).  That pair of leaves is contracted into one
    leaf, their two-key inner join (`pair_join`), and the term stays a tree;
    `in-out-out` has no such term."""
    ids, src, dst = hub_graph(31)
    want = brute_paths(ids, src, dst, joins)
    assert 0 < want < brute_paths(ids, src, dst, joins, forbid=False)
    rels, nodes = gpu_tables(gpu_session, [{"id": K(ids), "s": K(src), "t": K(dst)},
                                           {"id": K(np.concatenate([np.arange(30), [100, 205]]))}], enc)
    seen = []
    for with_nodes in (None, nodes):
        got, plan, detail = read3(gpu_session, lambda: rel_chain(rels, joins, 3, with_nodes))
        print(f"three-hop {joins} nodes={with_nodes is not None}: count {got} (brute force {want}) "
              f"plan {plan} detail {detail!r}")
        assert got == want, detail
        seen.append((plan, ["pair_join" in t.split() for t in detail.split("|")]))
    # filters (r1,r2), (r1,r3), (r2,r3): mask 2 is the r1 = r3 term alone
    pair = [m == 2 and joins != [("s", "s"), ("t", "s")] for m in range(8)]
    assert seen == [(PLAN, pair), (PLAN, pair)], seen


@pytest.mark.gpu
def test_pushed_predicate_on_a_rel_leaf_falls_back(gpu_session):
    """A filtered scan cannot merge with an unfiltered scan of the same rels:
    the count is not fused, and still exact."""
    ids, src, dst = hub_graph(32, hub=66, extra=20)
    rels = gpu_tables(gpu_session, [{"id": K(ids), "s": K(src), "t": K(dst)}])[0]
    joins = [("t", "s"), ("t", "s")]
    scans = [rels.select(("id", f"i{k}"), ("s", f"s{k}"), ("t", f"t{k}")) for k in range(3)]
    h = RecordHeader({Var(f"{c}{k}"): f"{c}{k}" for k in range(3) for c in "ist"})
    scans[1] = scans[1].filter(GreaterThan(Var("s1"), IntegerLit(0)), h, {})
    cur = scans[0].join(scans[1], "inner", ("t0", "s1")).join(scans[2], "inner", ("t1", "s2"))
    for x, y in [(0, 1), (0, 2), (1, 2)]:
        cur = cur.filter(Not(Equals(Var(f"i{x}"), Var(f"i{y}"))), h, {})
    gpu_session.reset_profile()
    got = cur.size
    assert gpu_session.last_plan() != PLAN and gpu_session.last_plan_detail() == ""
    keep = src != 0  # brute force with the middle rel restricted
    col = {"s": src.tolist(), "t": dst.tolist()}
    want = sum(1 for a in range(len(ids)) for b in range(len(ids)) if keep[b] and col["t"][a] == col["s"][b] and a != b
               for c in range(len(ids)) if col["t"][b] == col["s"][c] and c != a and c != b)
    assert got == want
    assert want != brute_paths(ids, src, dst, joins)


@pytest.mark.gpu
def test_more_than_four_filters_fall_back(gpu_session):
    """Four hops carry 6 uniqueness filters (> 4): the joins materialise;
    checked against the oracle's joins and brute force."""
    ids, src, dst = hub_graph(33, n_nodes=12, hub=0, extra=40)
    joins = [("t", "s")] * 3
    rels = gpu_tables(gpu_session, [{"id": K(ids), "s": K(src), "t": K(dst)}])[0]
    gpu_session.reset_profile()
    got = rel_chain(rels, joins, 4).size
    assert gpu_session.last_plan() != PLAN and gpu_session.last_plan_detail() == ""
    orels = OracleSession().table([("id", T_INT, ids, None), ("s", T_INT, src, None), ("t", T_INT, dst, None)])
    assert got == rel_chain(orels, joins, 4).size == brute_paths(ids, src, dst, joins)


@pytest.mark.gpu
def test_star_with_too_many_children_falls_back(gpu_session):
    """A centre joined to 7 tables (a job holds 6 child messages): the count
    declines and the joins materialise."""
    rng = np.random.default_rng(41)
    centre = {f"c{k}": K(rng.integers(0, 4, 6)) for k in range(7)}
    tables = [centre] + [{f"k{k}": K(rng.integers(0, 4, 5))} for k in range(7)]
    edges = [(0, f"c{k}", k + 1, f"k{k}") for k in range(7)]
    want = dp_count(tables, edges)
    assert want > 0
    tabs = gpu_tables(gpu_session, tables)
    gpu_session.reset_profile()
    assert join_tree(tabs, edges).size == want
    assert gpu_session.last_plan() != PLAN
    # six children still run fused
    check_tree(gpu_session, [{c: centre[c] for c in list(centre)[:6]}] + tables[1:7], edges[:6], None)
    assert gpu_session.last_plan_detail().endswith("generic:6")


# ------------------------------------------------------------------ id extremes
def fmix64(k):
    k = np.asarray(k).astype(np.uint64)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
    return k


@pytest.mark.gpu
def test_int64_min_is_a_key_of_a_hash_message(gpu_session):
    """INT64_MIN among 2500 sparse sender keys of a hash message.  24 of them
    have INT64_MIN's home slot as theirs (the table holds 8192 slots), at the
    far end of the sender from the INT64_MIN rows: had that id shared its
    marker with a free slot, one of them would claim the slot and its weight."""
    rng = np.random.default_rng(51)
    cap = 8192
    cand = rng.integers(-(1 << 62), 1 << 62, 600000)
    home = int(fmix64(np.array([MIN], dtype=np.int64))[0]) & (cap - 1)
    collide = np.unique(cand[(fmix64(cand) & np.uint64(cap - 1)) == np.uint64(home)])[:24]
    assert len(collide) == 24
    others = np.setdiff1d(np.unique(cand[:2600]), collide)[:2476]
    send = np.concatenate([[MIN] * 3, rng.permutation(others), collide]).astype(np.int64)
    assert 2 * len(send) <= cap < 4 * len(send)
    root = np.concatenate([[MIN, MIN], collide, collide, others[:300], cand[-200:], [MIN + 1]]).astype(np.int64)
    root = rng.permutation(root)
    tables, edges = [{"rk": K(root)}, {"sk": K(send)}], [(0, "rk", 1, "sk")]
    assert dp_count(tables, edges) == 2 * 3 + 2 * 24 + 300 + int(np.isin(cand[-200:], send).sum())
    check_tree(gpu_session, tables, edges, "hash generic:1")
    # the id as a sender key with a child of its own, and as a NULL-masked value
    nulls = np.zeros(len(send), dtype=bool)
    nulls[1] = True
    check_tree(gpu_session, [{"rk": K(root)}, {"sk": K(send, nulls)}], edges, "hash generic:1")


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["parent", "sender", "both"])
def test_both_int64_extremes_in_a_key_column(gpu_session, where):
    """[INT64_MIN, INT64_MAX] holds 2^64 keys: no dense array, no bitmap."""
    rng = np.random.default_rng(52)
    body = rng.integers(-1000, 1000, 300).astype(np.int64)
    ext = np.array([MIN, MAX, MIN, MAX, MAX, 0, -1], dtype=np.int64)
    root = np.concatenate([body, ext]) if where in ("parent", "both") else body
    uniq = np.unique(rng.integers(-1000, 1000, 200)).astype(np.int64)
    send = np.concatenate([uniq, [MIN, MAX]]) if where in ("sender", "both") else uniq
    tables, edges = [{"rk": K(root)}, {"sk": K(rng.permutation(send))}], [(0, "rk", 1, "sk")]
    # a parent range of 2^64 keys: a hash message; else the sender's unique keys as a bitmap over the parent's range
    want = "hash generic:1" if where != "sender" else "bits root1:bits:w8"
    check_tree(gpu_session, tables, edges, want)
    dup = np.concatenate([send, send[:50], [MAX] if where != "parent" else [7]]).astype(np.int64)
    check_tree(gpu_session, [{"rk": K(root)}, {"sk": K(dup)}], edges,
               "hash generic:1" if where != "sender" else "dense generic:1")


@pytest.mark.gpu
def test_two_hop_over_a_node_table_with_both_extremes(gpu_session):
    """The exact 2-hop shape whose node ids span [INT64_MIN, INT64_MAX]: the
    one-pass plan's per-id weights do not fit, message passing answers."""
    rng = np.random.default_rng(53)
    nid = np.concatenate([[MIN, MAX], rng.choice(5000, 60, replace=False)]).astype(np.int64)
    m = 400
    src, dst = nid[rng.integers(0, len(nid), m)], nid[rng.integers(0, len(nid), m)]
    src[:40], dst[:40] = MIN, MAX
    src[40:80], dst[40:80] = MAX, MIN
    src[80:90], dst[80:90] = MAX, MAX  # self-loops on an extreme
    ids = np.arange(m, dtype=np.int64)
    nodes, rels = gpu_tables(gpu_session, [{"id": K(nid)}, {"id": K(ids), "s": K(src), "t": K(dst)}])
    h = RecordHeader({Var(c): c for c in ("i0", "i1")})

    def make():
        r0, r1 = (rels.select(("id", f"i{k}"), ("s", f"s{k}"), ("t", f"t{k}")) for k in range(2))
        a, b, c = (nodes.select(("id", x)) for x in "abc")
        return (a.join(r0, "inner", ("a", "s0")).join(b, "inner", ("t0", "b")).join(r1, "inner", ("b", "s1"))
                .join(c, "inner", ("t1", "c")).filter(Not(Equals(Var("i0"), Var("i1"))), h, {}))

    got, plan, detail = read3(gpu_session, make)
    assert plan == PLAN and detail.count("|") == 1, (plan, detail)
    assert got == brute_paths(ids, src, dst, [("t", "s")])


@pytest.mark.gpu
@pytest.mark.parametrize("sender", ["unique", "repeated"])
@pytest.mark.parametrize("span", [1 << 28, (1 << 28) + 1, 1 << 34, (1 << 34) + 1],
                         ids=["2^28", "2^28+1", "2^34", "2^34+1"])
def test_key_range_cut_offs(gpu_session, span, sender):
    """Parent key ranges of exactly `span` keys, few rows.  A bitmap serves
    unique sender keys up to 2^34 keys; repeated ones need counts: with few
    rows (16 · max(rows, 1024) < 2^28) that is the hash map on either side of
    the dense array's 2^28 limit."""
    rng = np.random.default_rng(span % 1000 + len(sender))
    lo = -12345
    inner = lo + rng.permutation(np.unique(rng.integers(0, span, 400)))[:300].astype(np.int64)
    root = np.concatenate([[lo, lo + span - 1], inner[:200], [lo + 1, lo + span - 2]]).astype(np.int64)
    assert int(root.max()) - int(root.min()) + 1 == span
    send = np.concatenate([inner[100:], [lo, lo + span - 1, lo - 1, lo + span]]).astype(np.int64)
    if sender == "repeated":
        send = np.concatenate([send, inner[150:180], [lo + span - 1]])
    token = "bits root1:bits:w8" if sender == "unique" and span <= 1 << 34 else "hash generic:1"
    check_tree(gpu_session, [{"rk": K(root)}, {"sk": K(rng.permutation(send))}], [(0, "rk", 1, "sk")], token)


# ------------------------------------------------------------------ seeded fuzz
def fuzz_pool(r, flavour, size):
    if flavour == "dense":
        base = r.choice([0, -50, 10 ** 9, MAX - size + 1, MIN])
        return [base + i for i in range(size)]
    if flavour == "gapped":
        base, step = r.randint(-1000, 1000), r.choice([2, 3, 17])
        return [base + step * i for i in range(size)]
    if flavour == "sparse":
        return r.sample(range(-(10 ** 13), 10 ** 13), size)
    return [MIN, MAX, MIN + 1, MAX - 1, 0, -1] + r.sample(range(-(1 << 61), 1 << 61), max(size - 6, 0))


def fuzz_tree(seed):
    """(tables, edges, encodings, first table) of one random tree: 2–5 tables of 0–400
    rows, a chain or a star; each edge draws both key columns from one pool of
    50–400 ids (dense, gapped, sparse or extreme), so keys repeat ≤ 8 times on
    average; some columns are permutations (unique), some hold NULLs."""
    r = random.Random(seed)
    nt = r.randint(2, 5)
    shape = r.choice(["chain", "star"])
    rows = [r.choice([0, 1, r.randint(2, 40), r.randint(41, 400)]) for _ in range(nt)]
    pairs = [(i, i + 1) for i in range(nt - 1)] if shape == "chain" else [(0, i) for i in range(1, nt)]
    tables = [dict() for _ in range(nt)]
    edges = []
    for e, (a, b) in enumerate(pairs):
        pool = fuzz_pool(r, r.choice(["dense", "gapped", "sparse", "extreme"]), r.randint(50, 400))
        for t, name in ((a, f"e{e}a"), (b, f"e{e}b")):
            n = rows[t]
            if r.random() < 0.4 and n <= len(pool):
                vals = r.sample(pool, n) if r.random() < 0.5 else pool[:n]  # unique (a whole dense range when n fits)
            else:
                vals = [r.choice(pool) for _ in range(n)]
            nulls = None
            if r.random() < 0.3:
                nulls = [r.random() < 0.15 for _ in range(n)]
            tables[t][name] = K(vals, nulls)
        edges.append((a, f"e{e}a", b, f"e{e}b"))
    encs = [r.choice([None, 4, 3]) for _ in range(nt)]
    return tables, edges, encs, r.randrange(nt)  # the joins start from any table


FUZZ_SEEDS = list(range(200))


def test_fuzz_generator_draws_acyclic_int64_trees():
    """Every shape the fuzz draws is a tree of int64 key columns: nothing the
    fused count may decline."""
    flavours = set()
    for seed in FUZZ_SEEDS:
        tables, edges, encs, start = fuzz_tree(seed)
        nt = len(tables)
        assert 2 <= nt <= 5 and len(edges) == nt - 1 and len(encs) == nt and 0 <= start < nt
        rep = list(range(nt))

        def find(x):
            while rep[x] != x:
                x = rep[x]
            return x
        for a, ca, b, cb in edges:
            assert find(a) != find(b), seed  # no cycle, no parallel edge
            rep[find(a)] = find(b)
            assert ca in tables[a] and cb in tables[b]
        assert len({find(i) for i in range(nt)}) == 1, seed
        for t in tables:
            assert t and len({len(v) for v, _ in t.values()}) == 1 and nrows(t) <= 400
            for v, ok in t.values():
                assert v.dtype == np.int64 and (ok is None or ok.dtype == bool)
                flavours.add("null" if ok is not None and not ok.all() else "plain")
        assert dp_count(tables, edges) == dp_count(tables, edges, root=nt - 1)  # any root gives the count
    assert flavours == {"null", "plain"}
    assert len({len(fuzz_tree(s)[0]) for s in FUZZ_SEEDS}) == 4


def test_dynamic_programme_equals_materialised_joins():
    """The reference itself, against the oracle's joins materialising every row."""
    for seed in FUZZ_SEEDS:
        tables, edges, _, start = fuzz_tree(seed)
        ot = [OracleSession().table([(c, T_INT, [x if ok is None or ok[i] else None for i, x in enumerate(v.tolist())],
                                      None) for c, (v, ok) in t.items()], nrows=nrows(t)) for t in tables]
        assert join_tree(ot, edges, start).size == dp_count(tables, edges), seed


@pytest.mark.gpu
def test_fuzz_trees_vs_dynamic_programme(gpu_session):
    bad, skipped, kinds = [], [], set()
    for seed in FUZZ_SEEDS:
        tables, edges, encs, start = fuzz_tree(seed)
        want = dp_count(tables, edges)
        tabs = gpu_tables(gpu_session, tables, encs)
        gpu_session.reset_profile()
        try:
            got = join_tree(tabs, edges, start).size
        except Exception as e:  # noqa: BLE001 - reported with the seed
            bad.append((seed, repr(e)[:200]))
            continue
        if got != want:
            bad.append((seed, got, want, gpu_session.last_plan(), gpu_session.last_plan_detail()))
        if gpu_session.last_plan() != PLAN:
            skipped.append((seed, gpu_session.last_plan()))
        kinds.update(norm(gpu_session.last_plan_detail()).split())
    assert not bad, f"{len(bad)} of {len(FUZZ_SEEDS)} seeds differ: {bad[:5]}"
    assert len(skipped) <= len(FUZZ_SEEDS) // 10, skipped[:10]
    assert {"ones", "bits", "dense", "hash", "empty", "all_rows"} <= kinds, kinds
