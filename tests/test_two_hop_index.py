"""The in-side index of the fused 2-hop count (csrc/chain2_partitioned.hip,
C5InIndex): the first query over a rel table answers through the unindexed
mode-P pipeline and stores every bucket's finished image (in-degree halves,
special keys) and the self-loop count on the end column; later queries
partition the source column only and probe the images.

Shapes follow test_two_hop_steal.py: ids below 2^24 (256 buckets: mode P by
default), CAPF_CHAIN2=partitioned, jobs of 16 tiles.  Every assertion on a
count is exact equality with oracle.cmodel.count_2hop.  The profile counters
c5_index_builds (images installed: settled by the query after the build),
c5_index_refused and c5_index_queries are read as differences within a test:
the session is shared.
"""
import numpy as np
import pytest

from capf_amd.expr import CountStar, T_INT
from capf_amd.graph import ElementTable, ScanGraph
from capf_amd.planner import Match, NodeP, Query, RelP, Stage, plan_query, run
from capf_amd.table import compact_as
from oracle import cmodel, nodemix

pytestmark = pytest.mark.gpu

TWO_HOP = Query([Match([NodeP("a"), NodeP("b"), NodeP("c")], [RelP("r1", "a", "b"), RelP("r2", "b", "c")])],
                [Stage([("count", CountStar())])])
BITS = 24
N = 1 << BITS
TILE = 32768  # rows per tile of the one-sided P1 (two 16 Ki-row tiles of the two-sided one)
WIDTH = {False: 8, 4: 4, 3: 3}  # bytes per id: int64, FOR32, FOR24
COUNTERS = ("c5_index_builds", "c5_index_refused", "c5_index_queries")


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("CAPF_CHAIN2", "partitioned")
    monkeypatch.setenv("CAPF_C5_STEAL_TILES", "16")
    for v in ("CAPF_C5_PROBE", "CAPF_C5_DIRECT", "CAPF_P3_SPLIT", "CAPF_C5_STEAL", "CAPF_C5_INDEX",
              "CAPF_C5_HOTCAP"):
        monkeypatch.delenv(v, raising=False)


@pytest.fixture(scope="module")
def _mix():
    """(bucket, key) of every id below 2^24 under the node mix."""
    h = nodemix.node_mix(np.arange(N, dtype=np.int64), BITS)
    return h >> 16, h & 0xFFFF


def _ids_in_bucket(mix, bucket):
    return np.nonzero(mix[0] == bucket)[0].astype(np.int64)


def _graph(session, src, dst, compact):
    m = len(src)
    rels = session.table([("id", T_INT, np.arange(m), None), ("source", T_INT, src, None),
                          ("target", T_INT, dst, None)])
    nodes = session.range_nodes(0, N, id_col="id")
    rels, nodes = compact_as(rels, compact), compact_as(nodes, compact)
    return ScanGraph(session, [ElementTable("node", frozenset(["V"]), nodes, {})],
                     [ElementTable("rel", frozenset(["E"]), rels, {})])


def _expect(src, dst):
    return cmodel.count_2hop(np.ascontiguousarray(src, dtype=np.int64), np.ascontiguousarray(dst, dtype=np.int64), N)


def _count(session, g):
    got = run(g, TWO_HOP)[0]["count"]
    assert session.last_plan() == "fused_chain2"
    return got


class _Profiled:
    """Profiling on for the test; counters and c5_partition bytes as
    differences from the last look."""

    def __init__(self, session):
        self.s = session
        session.reset_profile()
        session.set_profiling(True)
        self.last = self._read()

    def _read(self):
        prof = self.s.profile()
        out = {k: prof.get(k, {"bytes": 0.0})["bytes"] for k in COUNTERS + ("c5_partition", "c5_steals")}
        out["launches"] = {k: prof.get(k, {"launches": 0})["launches"] for k in ("c5_partition", "c5_gather", "chain2_dot")}
        return out

    def step(self):
        now = self._read()
        d = {k: now[k] - self.last[k] for k in now if k != "launches"}
        d["launches"] = {k: now["launches"][k] - self.last["launches"][k] for k in now["launches"]}
        self.last = now
        return d

    def close(self):
        self.s.set_profiling(False)


@pytest.fixture
def profiled(gpu_session):
    p = _Profiled(gpu_session)
    yield p
    p.close()


def _three_queries(session, profiled, g, expect, n, w):
    """Query 1 builds, queries 2 and 3 probe: counts, counters, P1 bytes."""
    seen = []
    for _ in range(3):
        assert _count(session, g) == expect
        seen.append(profiled.step())
    assert [d["c5_partition"] for d in seen] == [(2 * w + 4) * n, (w + 2) * n, (w + 2) * n]
    assert sum(d["c5_index_builds"] for d in seen) == 1
    assert sum(d["c5_index_queries"] for d in seen) == 2
    assert sum(d["c5_index_refused"] for d in seen) == 0
    assert all(d["launches"]["chain2_dot"] == 0 for d in seen)
    return seen


@pytest.fixture(scope="module")
def _uniform():
    rng = np.random.default_rng(101)
    m = (1 << 20) + 4321
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    dst[:200000] = src[200000:400000]  # paths
    return src, dst, _expect(src, dst)


@pytest.mark.parametrize("compact", [False, 4, 3], ids=["int64", "for32", "for24"])
def test_index_three_queries(gpu_session, profiled, _uniform, compact):
    src, dst, expect = _uniform
    assert expect > 0
    g = _graph(gpu_session, src, dst, compact)
    _three_queries(gpu_session, profiled, g, expect, len(src), WIDTH[compact])


@pytest.fixture(scope="module")
def _specials(_mix):
    """In-degrees exactly 2^16 − 1, 2^16, 2^16 + 1 and 2^17 + 3; the last three
    (specials: in-degree ≥ 2^16) share bucket 33 — one more than the two held
    in scalars — and the 2^17 + 3 one sources 60,000 rels."""
    rng = np.random.default_rng(7)
    m = 1 << 20
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    ids = _ids_in_bucket(_mix, 33)
    hubs = [int(_ids_in_bucket(_mix, 120)[5]), int(ids[10]), int(ids[2000]), int(ids[40000])]
    degs = [(1 << 16) - 1, 1 << 16, (1 << 16) + 1, (1 << 17) + 3]
    spare = int(_ids_in_bucket(_mix, 200)[0])
    dst[np.isin(dst, hubs)] = spare
    pos = 0
    for h, d in zip(hubs, degs):
        dst[pos:pos + d] = h
        pos += d
    src[pos:pos + 60000] = hubs[3]
    src[pos + 60000:pos + 61000] = hubs[0]
    src[pos + 61000:pos + 62000] = hubs[1]
    indeg = np.bincount(dst, minlength=N)
    assert [int(indeg[h]) for h in hubs] == degs
    return src, dst, _expect(src, dst)


@pytest.mark.parametrize("compact", [False, 3], ids=["int64", "for24"])
def test_index_special_keys(gpu_session, profiled, _specials, compact):
    src, dst, expect = _specials
    g = _graph(gpu_session, src, dst, compact)
    _three_queries(gpu_session, profiled, g, expect, len(src), WIDTH[compact])


def test_index_self_loops(gpu_session, profiled, _mix):
    """Self-loops on a special key, on ordinary keys and in the ragged tile:
    queries 2 and 3 subtract the index's loop count."""
    rng = np.random.default_rng(19)
    m = 20 * TILE + 777
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    hub = int(_ids_in_bucket(_mix, 64)[123])
    dst[1000:1000 + 70000] = hub
    src[50000:50000 + 30000] = hub       # [50000, 71000): loops on the special key
    dst[300000:300500] = src[300000:300500]
    dst[m - 300:] = src[m - 300:]        # loops in the ragged tile
    loops = int((src == dst).sum())
    assert loops >= 21000 + 500 + 300
    g = _graph(gpu_session, src, dst, 3)
    _three_queries(gpu_session, profiled, g, _expect(src, dst), m, 3)


@pytest.mark.parametrize("m", [TILE + 12345, TILE // 2 + 12345, 1000, 4 * TILE],
                         ids=["tile+12345", "halftile+12345", "1000", "4tiles"])
def test_index_ragged_and_tiny(gpu_session, profiled, m):
    """One tile and a ragged one; a ragged tile whose second half is partly
    filled; the ragged tile alone; whole tiles only."""
    rng = np.random.default_rng(m)
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    k = m // 5
    dst[:k] = src[k:2 * k]
    dst[m - 10:] = src[m - 10:]
    expect = _expect(src, dst)
    assert expect > 0
    g = _graph(gpu_session, src, dst, 3)
    _three_queries(gpu_session, profiled, g, expect, m, 3)


def test_index_skewed_out_run(gpu_session, profiled, _mix):
    """60 % of the sources in bucket 77 (≈150 × the mean out-run): its jobs of
    16 tiles are drawn by many units.  Whether another unit helps is timing:
    the count only."""
    rng = np.random.default_rng(41)
    m = 1 << 22
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    pool = _ids_in_bucket(_mix, 77)[:40000]
    heavy = rng.random(m) < 0.6
    src[heavy] = pool[rng.integers(0, len(pool), int(heavy.sum()))]
    dst[:5000] = src[5000:10000]
    g = _graph(gpu_session, src, dst, 3)
    _three_queries(gpu_session, profiled, g, _expect(src, dst), m, 3)


def test_index_empty_buckets(gpu_session, profiled, _mix):
    """All targets in 3 buckets, sources uniform: 253 all-zero images, and
    out keys that probe them."""
    rng = np.random.default_rng(3)
    m = 1 << 18
    src = rng.integers(0, N, m)
    pool = np.concatenate([_ids_in_bucket(_mix, b) for b in (5, 100, 255)])
    dst = pool[rng.integers(0, len(pool), m)]
    src[:20000] = dst[20000:40000]
    expect = _expect(src, dst)
    assert expect > 0
    g = _graph(gpu_session, src, dst, 3)
    _three_queries(gpu_session, profiled, g, expect, m, 3)


def test_index_two_tables(gpu_session, profiled):
    """Two rel tables in one session: each its own index, interleaved queries
    each its own count; a re-encoded copy of a table is a new column pair."""
    rng = np.random.default_rng(77)
    m = 3 * TILE + 99
    xs, xd = rng.integers(0, N, m), rng.integers(0, N, m)
    xd[:9000] = xs[9000:18000]
    ys, yd = xs[rng.permutation(m)], rng.integers(0, N, m)
    yd[:5000] = ys[5000:10000]
    xe, ye = _expect(xs, xd), _expect(ys, yd)
    assert xe != ye
    gx = _graph(gpu_session, xs, xd, 3)
    gy = _graph(gpu_session, ys, yd, 3)
    for g, e in [(gx, xe), (gy, ye), (gx, xe), (gy, ye), (gx, xe), (gy, ye)]:
        assert _count(gpu_session, g) == e
    d = profiled.step()
    assert d["c5_index_builds"] == 2
    assert d["c5_index_queries"] == 4
    gx32 = _graph(gpu_session, xs, xd, 4)
    for _ in range(2):
        assert _count(gpu_session, gx32) == xe
    assert _count(gpu_session, gx) == xe
    d = profiled.step()
    assert d["c5_index_builds"] == 1
    assert d["c5_index_queries"] == 2


def test_index_off_switch(gpu_session, profiled, monkeypatch, _uniform):
    monkeypatch.setenv("CAPF_C5_INDEX", "0")
    src, dst, expect = _uniform
    g = _graph(gpu_session, src, dst, 3)
    for _ in range(3):
        assert _count(gpu_session, g) == expect
        d = profiled.step()
        assert d["c5_partition"] == (2 * 3 + 4) * len(src)
        assert d["c5_index_builds"] == 0 and d["c5_index_queries"] == 0


def test_index_refused(gpu_session, profiled, monkeypatch, _mix):
    """One hot-table slot and two hot keys (in-degree ≥ 2^15) in one bucket:
    the build query's units log, the images are not self-contained, and every
    query keeps the unindexed pipeline."""
    monkeypatch.setenv("CAPF_C5_HOTCAP", "1")
    rng = np.random.default_rng(29)
    m = 1 << 19
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    ids = _ids_in_bucket(_mix, 150)
    h1, h2 = int(ids[100]), int(ids[30000])
    dst[0:40000] = h1
    dst[40000:75000] = h2
    src[80000:82000] = h1
    src[82000:83000] = h2
    expect = _expect(src, dst)
    g = _graph(gpu_session, src, dst, 3)
    seen = []
    for _ in range(3):
        assert _count(gpu_session, g) == expect
        seen.append(profiled.step())
    assert sum(d["c5_index_refused"] for d in seen) >= 1
    assert sum(d["c5_index_queries"] for d in seen) == 0
    assert sum(d["c5_index_builds"] for d in seen) == 0
    assert [d["c5_partition"] for d in seen] == [(2 * 3 + 4) * m] * 3


def test_index_async(gpu_session, _uniform):
    """count_async into a device slot as query 2; then four count_async calls
    on a fresh graph without a sync between them: the first builds, the rest
    probe, in stream order."""
    import torch
    src, dst, expect = _uniform
    g = _graph(gpu_session, src, dst, 3)
    assert _count(gpu_session, g) == expect
    slots = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    plan_query(g, TWO_HOP).table.count_async(slots.data_ptr())
    gpu_session.sync()
    assert slots[0].item() == expect
    g2 = _graph(gpu_session, src, dst, 3)
    for i in range(1, 5):
        plan_query(g2, TWO_HOP).table.count_async(slots.data_ptr() + 8 * i)
    gpu_session.sync()
    assert slots.cpu().tolist() == [expect] * 5
