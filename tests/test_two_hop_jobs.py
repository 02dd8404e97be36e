"""Jobs of the indexed probe of the fused 2-hop count (csrc/chain2_partitioned.hip,
k_c5_gather<…, IDX>): a slot's cursor counts tiles, and an indexed unit sizes
the jobs of its slot by the work in the slot's out-run (C5Steal::job_pieces,
jobt[]) — a mean run is cut into CAPF_C5_JOB_SPLIT jobs, none shorter than
CAPF_C5_STEAL_TILES tiles.  Whatever lengths the takers use, the jobs of a
slot are disjoint tile ranges that cover the run, so every count is exact.

Shapes follow test_two_hop_index.py: ids below 2^24 (256 buckets),
CAPF_CHAIN2=partitioned, tiles of 32 Ki rows, three queries per graph (one
builds the index, two probe it).  Every count is compared for exact equality
with oracle.cmodel.count_2hop.  The profile counters are read as differences
within a test: the session is shared.  c5_steals is timing: nothing is
asserted on it.
"""
import numpy as np
import pytest

from capf_amd.expr import CountStar, T_INT
from capf_amd.graph import ElementTable, ScanGraph
from capf_amd.planner import Match, NodeP, Query, RelP, Stage, run
from capf_amd.table import compact_as
from oracle import cmodel, nodemix

pytestmark = pytest.mark.gpu

TWO_HOP = Query([Match([NodeP("a"), NodeP("b"), NodeP("c")], [RelP("r1", "a", "b"), RelP("r2", "b", "c")])],
                [Stage([("count", CountStar())])])
BITS = 24
N = 1 << BITS
NB = 256
TILE = 32768  # rows per tile of the one-sided P1
COUNTERS = ("c5_index_builds", "c5_index_refused", "c5_index_queries", "c5_jobs")
KNOBS = [(t, j) for t in (1, 3, 16) for j in (1, 8)]
KNOB_IDS = [f"tiles{t}-split{j}" for t, j in KNOBS]


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("CAPF_CHAIN2", "partitioned")
    for v in ("CAPF_C5_PROBE", "CAPF_C5_DIRECT", "CAPF_P3_SPLIT", "CAPF_C5_STEAL", "CAPF_C5_INDEX",
              "CAPF_C5_HOTCAP", "CAPF_C5_STEAL_TILES", "CAPF_C5_JOB_SPLIT"):
        monkeypatch.delenv(v, raising=False)


@pytest.fixture(scope="module")
def _mix():
    """(bucket, key) of every id below 2^24 under the node mix."""
    h = nodemix.node_mix(np.arange(N, dtype=np.int64), BITS)
    return h >> 16, h & 0xFFFF


def _ids_in_bucket(mix, bucket):
    return np.nonzero(mix[0] == bucket)[0].astype(np.int64)


def _graph(session, src, dst, compact=3):
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
    """Profiling on for the test; the counters as differences from the last look."""

    def __init__(self, session):
        self.s = session
        session.reset_profile()
        session.set_profiling(True)
        self.last = self._read()

    def _read(self):
        prof = self.s.profile()
        return {k: prof.get(k, {"bytes": 0.0})["bytes"] for k in COUNTERS}

    def step(self):
        now = self._read()
        d = {k: now[k] - self.last[k] for k in now}
        self.last = now
        return d

    def close(self):
        self.s.set_profiling(False)


@pytest.fixture
def profiled(gpu_session):
    p = _Profiled(gpu_session)
    yield p
    p.close()


def _three_queries(session, profiled, monkeypatch, graph, min_tiles, split):
    """Query 1 builds the index, queries 2 and 3 probe it with jobs of at least
    min_tiles tiles, `split` to a mean run: counts, counters, the jobs' bounds."""
    src, dst, expect = graph
    monkeypatch.setenv("CAPF_C5_STEAL_TILES", str(min_tiles))
    monkeypatch.setenv("CAPF_C5_JOB_SPLIT", str(split))
    g = _graph(session, src, dst)
    ntiles = -(-len(src) // TILE)
    seen = []
    for _ in range(3):
        assert _count(session, g) == expect
        seen.append(profiled.step())
    print("c5_jobs per query:", [d["c5_jobs"] for d in seen], "ntiles", ntiles)
    assert [d["c5_index_queries"] for d in seen] == [0, 1, 1]
    assert sum(d["c5_index_builds"] for d in seen) == 1
    assert sum(d["c5_index_refused"] for d in seen) == 0
    for d in seen[1:]:
        # every slot's first add succeeds: one job at least per slot; a job is
        # min_tiles long or ends its run
        assert d["c5_jobs"] >= NB
        assert d["c5_jobs"] <= NB * -(-ntiles // min_tiles) + NB


def _uniform_graph(seed, m):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    k = m // 5
    dst[:k] = src[k:2 * k]  # paths
    dst[m - 10:] = src[m - 10:]
    expect = _expect(src, dst)
    assert expect > 0
    return src, dst, expect


@pytest.fixture(scope="module")
def _five_tiles():
    """ntiles = 5 with a ragged last tile: a job is shorter than the 16 waves it is dealt to."""
    return _uniform_graph(11, 4 * TILE + 777)


@pytest.fixture(scope="module")
def _one_tile():
    """A single ragged tile: every job length is clamped to ntiles = 1."""
    return _uniform_graph(12, 1000)


@pytest.fixture(scope="module")
def _uniform_128():
    """128 tiles: at 3 tiles per job the lengths do not divide the run and a slot's last job is clipped."""
    return _uniform_graph(13, 1 << 22)


@pytest.fixture(scope="module")
def _skewed(_mix):
    """60 % of the sources in bucket 77 (≈150 × the mean out-run): its job
    length clamps to the minimum while the other runs take one job each."""
    rng = np.random.default_rng(41)
    m = 1 << 22
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    pool = _ids_in_bucket(_mix, 77)[:40000]
    heavy = rng.random(m) < 0.6
    src[heavy] = pool[rng.integers(0, len(pool), int(heavy.sum()))]
    dst[:5000] = src[5000:10000]
    return src, dst, _expect(src, dst)


@pytest.fixture(scope="module")
def _three_source_buckets(_mix):
    """Sources in 3 buckets: 253 out-runs hold no piece (their weight is 0)."""
    rng = np.random.default_rng(5)
    m = 1 << 18
    dst = rng.integers(0, N, m)
    pool = np.concatenate([_ids_in_bucket(_mix, b) for b in (5, 100, 255)])
    src = pool[rng.integers(0, len(pool), m)]
    dst[:20000] = src[20000:40000]
    expect = _expect(src, dst)
    assert expect > 0
    return src, dst, expect


@pytest.fixture(scope="module")
def _specials(_mix):
    """In-degrees exactly 2^16 − 1, 2^16, 2^16 + 1 and 2^17 + 3; the last three
    (specials: in-degree ≥ 2^16) share bucket 33, and the 2^17 + 3 one sources
    60,000 rels: its probes are folded per job."""
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
    # spread over every tile of the out-run, so every job of the run meets the special keys
    at = rng.choice(np.arange(pos, m), 62000, replace=False)
    src[at[:60000]] = hubs[3]
    src[at[60000:61000]] = hubs[0]
    src[at[61000:]] = hubs[1]
    indeg = np.bincount(dst, minlength=N)
    assert [int(indeg[h]) for h in hubs] == degs
    return src, dst, _expect(src, dst)


@pytest.mark.parametrize("min_tiles,split", KNOBS, ids=KNOB_IDS)
def test_jobs_five_tiles(gpu_session, profiled, monkeypatch, _five_tiles, min_tiles, split):
    _three_queries(gpu_session, profiled, monkeypatch, _five_tiles, min_tiles, split)


@pytest.mark.parametrize("min_tiles,split", KNOBS, ids=KNOB_IDS)
def test_jobs_single_ragged_tile(gpu_session, profiled, monkeypatch, _one_tile, min_tiles, split):
    _three_queries(gpu_session, profiled, monkeypatch, _one_tile, min_tiles, split)


@pytest.mark.parametrize("min_tiles,split", KNOBS, ids=KNOB_IDS)
def test_jobs_uniform_128_tiles(gpu_session, profiled, monkeypatch, _uniform_128, min_tiles, split):
    _three_queries(gpu_session, profiled, monkeypatch, _uniform_128, min_tiles, split)


@pytest.mark.parametrize("min_tiles,split", KNOBS, ids=KNOB_IDS)
def test_jobs_skewed_out_run(gpu_session, profiled, monkeypatch, _skewed, min_tiles, split):
    _three_queries(gpu_session, profiled, monkeypatch, _skewed, min_tiles, split)


@pytest.mark.parametrize("min_tiles,split", KNOBS, ids=KNOB_IDS)
def test_jobs_empty_out_runs(gpu_session, profiled, monkeypatch, _three_source_buckets, min_tiles, split):
    _three_queries(gpu_session, profiled, monkeypatch, _three_source_buckets, min_tiles, split)


@pytest.mark.parametrize("min_tiles,split", KNOBS, ids=KNOB_IDS)
def test_jobs_special_keys(gpu_session, profiled, monkeypatch, _specials, min_tiles, split):
    _three_queries(gpu_session, profiled, monkeypatch, _specials, min_tiles, split)


def test_jobs_mode_p_publishers(gpu_session, profiled, monkeypatch):
    """The unindexed pipeline with every unit publishing (CAPF_C5_STEAL=all,
    jobs of 16 tiles) over two rel tables, interleaved: the tile cursor with
    a fixed job length; no index is built or probed."""
    monkeypatch.setenv("CAPF_C5_STEAL", "all")
    monkeypatch.setenv("CAPF_C5_STEAL_TILES", "16")
    rng = np.random.default_rng(77)
    m = 3 * TILE + 99
    xs, xd = rng.integers(0, N, m), rng.integers(0, N, m)
    xd[:9000] = xs[9000:18000]
    ys, yd = xs[rng.permutation(m)], rng.integers(0, N, m)
    yd[:5000] = ys[5000:10000]
    xe, ye = _expect(xs, xd), _expect(ys, yd)
    assert xe != ye
    gx = _graph(gpu_session, xs, xd)
    gy = _graph(gpu_session, ys, yd)
    for g, e in [(gx, xe), (gy, ye), (gx, xe), (gy, ye)]:
        assert _count(gpu_session, g) == e
    d = profiled.step()
    assert d["c5_index_builds"] == 0 and d["c5_index_queries"] == 0
    assert d["c5_jobs"] >= 4 * NB  # a published bucket's run is drawn from its cursor: a job at least
