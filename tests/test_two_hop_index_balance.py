"""The indexed 2-hop count's work balance (csrc/chain2_partitioned.hip,
k_c5_gather<…, IDX>; csrc/c5_job_len.h): the two-zone job rule.  An out-run
above the mean by a crumb's weight or more is cut into CAPF_C5_JOB_SPLIT base
jobs over the tiles that hold a mean run's work and CAPF_C5_EXCESS_SPLIT times
finer crumbs over the rest; every other run keeps the one-zone rule.

Shapes follow test_two_hop_index.py: ids below 2^24 (256 buckets: mode P by
default), CAPF_CHAIN2=partitioned, jobs of at least 16 tiles, at most 2^22
rows (128 tiles of 32 Ki rows).  Every count is compared for exact equality
with oracle.cmodel.count_2hop; each graph runs three queries, the first
builds the index, the second and third probe it.  c5_jobs is asserted as
bounds (a taker that reads a slot's length while it is still 0 takes the
minimum), c5_steals never: it is timing.
"""
import numpy as np
import pytest

from capf_amd import _lib
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
MIN_TILES = 16
J, X = 4, 2  # the defaults of CAPF_C5_JOB_SPLIT and CAPF_C5_EXCESS_SPLIT
WIDTH = {False: 8, 4: 4, 3: 3}  # bytes per id: int64, FOR32, FOR24
COUNTERS = ("c5_index_builds", "c5_index_refused", "c5_index_queries", "c5_jobs", "c5_partition")


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("CAPF_CHAIN2", "partitioned")
    monkeypatch.setenv("CAPF_C5_STEAL_TILES", str(MIN_TILES))
    for v in ("CAPF_C5_PROBE", "CAPF_C5_DIRECT", "CAPF_P3_SPLIT", "CAPF_C5_STEAL", "CAPF_C5_INDEX",
              "CAPF_C5_HOTCAP", "CAPF_C5_JOB_SPLIT", "CAPF_C5_EXCESS_SPLIT"):
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


# ---------------------------------------------------------------- the rule, restated
def _run_pieces(mix, src):
    """T of every out-run: its 16-B pieces, ceil(keys / 8) per tile."""
    m = len(src)
    ntiles = -(-m // TILE)
    cnt = np.bincount((np.arange(m) // TILE) * NB + mix[0][src], minlength=ntiles * NB).reshape(ntiles, NB)
    return ((cnt + 7) // 8).sum(axis=0), ntiles


def _job_pieces(m, ntiles, split):
    """W: the pieces of a job, mean / split (keys + ~3.5 pad keys per tile, in eights)."""
    return max(1, int(((m / NB + 3.5 * ntiles) / 8) / split))


def _one_zone_jobs(T, m, ntiles, split=J, min_tiles=MIN_TILES):
    """Jobs of a probe query under the one-zone rule, when every taker reads the stored length."""
    W = _job_pieces(m, ntiles, split)
    k = np.maximum(1, (T + W // 2) // W)
    jt = np.minimum(ntiles, np.maximum(min_tiles, -(-ntiles // k)))
    return int((-(-ntiles // jt)).sum())


def _lens(T, m, ntiles):
    """(base, crumb) lengths of a run of T pieces under the defaults, from the library's own function."""
    W = _job_pieces(m, ntiles, J)
    f = _lib.load().capf_c5_job_len
    return int(f(int(T), W * J, J, X, ntiles, MIN_TILES, 0)), int(f(int(T), W * J, J, X, ntiles, MIN_TILES, ntiles - 1))


def _three_queries(session, profiled, g, expect, n, w, nonempty=NB):
    """Query 1 builds, queries 2 and 3 probe: counts, counters, P1 bytes, the jobs' bounds."""
    ntiles = -(-n // TILE)
    seen = []
    for _ in range(3):
        assert _count(session, g) == expect
        seen.append(profiled.step())
    print("c5_jobs per query:", [d["c5_jobs"] for d in seen], "ntiles", ntiles)
    assert [d["c5_partition"] for d in seen] == [(2 * w + 4) * n, (w + 2) * n, (w + 2) * n]
    assert [d["c5_index_queries"] for d in seen] == [0, 1, 1]
    assert sum(d["c5_index_builds"] for d in seen) == 1
    assert sum(d["c5_index_refused"] for d in seen) == 0
    for d in seen[1:]:
        assert nonempty <= d["c5_jobs"] <= NB * -(-ntiles // MIN_TILES)
    return seen


# ---------------------------------------------------------------- 1. every image differs
@pytest.fixture(scope="module")
def _uniform():
    """Uniform sources and targets: all 256 images differ, so a unit that probed
    an out-run against another bucket's image would give a wrong count."""
    rng = np.random.default_rng(101)
    m = (1 << 20) + 4321
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    dst[:200000] = src[200000:400000]  # paths
    return src, dst, _expect(src, dst)


@pytest.mark.parametrize("compact", [False, 4, 3], ids=["int64", "for32", "for24"])
def test_balance_uniform_all_images_differ(gpu_session, profiled, _uniform, compact):
    src, dst, expect = _uniform
    assert expect > 0
    g = _graph(gpu_session, src, dst, compact)
    _three_queries(gpu_session, profiled, g, expect, len(src), WIDTH[compact])


# ---------------------------------------------------------------- 2. – 4. heavy out-runs
def _heavy_graph(mix, seed, extra, sort_heavy=False):
    """Uniform rels, m = 2^22, plus for every (bucket, x) of `extra` x mean runs' worth
    of rows whose sources are redrawn from the bucket's ids."""
    rng = np.random.default_rng(seed)
    m = 1 << 22
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    rows = rng.permutation(m)
    at = 0
    for bucket, x in extra:
        e = int(round(x * m / NB))
        pool = _ids_in_bucket(mix, bucket)[:40000]
        ids = pool[rng.integers(0, len(pool), e)]
        if sort_heavy:  # the run's work sits in its first tiles, in source order
            src[at:at + e] = np.sort(ids)
        else:
            src[rows[at:at + e]] = ids
        at += e
    dst[m - 5000:] = src[m - 10000:m - 5000]  # paths
    return src, dst, _expect(src, dst)


@pytest.fixture(scope="module")
def _heavy_13(_mix):
    return _heavy_graph(_mix, 201, [(77, 0.3)])


@pytest.mark.parametrize("x", [0.3, 2.0], ids=["1.3x", "3x"])
def test_balance_one_heavy_run(gpu_session, profiled, _mix, _heavy_13, x):
    """Bucket 77's out-run holds ≈1.3 × (≈3 ×) the mean: a base zone of 4 jobs and
    crumbs of at least 16 tiles behind it."""
    src, dst, expect = _heavy_13 if x == 0.3 else _heavy_graph(_mix, 202, [(77, x)])
    T, ntiles = _run_pieces(_mix, src)
    base, crumb = _lens(T[77], len(src), ntiles)
    print("bucket 77: T / mean", T[77] / T.mean(), "base", base, "crumb", crumb)
    assert J * base < ntiles and (ntiles - J * base) // crumb >= 1  # both zones exist
    if x == 0.3:
        assert MIN_TILES <= crumb < base
    else:  # 128 tiles: at 3 × the mean both lengths clamp to the minimum
        assert crumb == base == MIN_TILES
    others = [_lens(T[b], len(src), ntiles) for b in (0, 76, 78, 255)]
    assert all(b == c for b, c in others), others  # the runs near the mean keep one length
    g = _graph(gpu_session, src, dst)
    _three_queries(gpu_session, profiled, g, expect, len(src), 3, int((T > 0).sum()))


def test_balance_skewed_out_run(gpu_session, profiled, _mix):
    """60 % of the sources in bucket 77 (≈150 × the mean out-run): both its
    lengths clamp to the minimum, the other runs are below the mean."""
    rng = np.random.default_rng(41)
    m = 1 << 22
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    pool = _ids_in_bucket(_mix, 77)[:40000]
    heavy = rng.random(m) < 0.6
    src[heavy] = pool[rng.integers(0, len(pool), int(heavy.sum()))]
    dst[:5000] = src[5000:10000]
    T, ntiles = _run_pieces(_mix, src)
    assert _lens(T[77], m, ntiles) == (MIN_TILES, MIN_TILES)
    g = _graph(gpu_session, src, dst)
    _three_queries(gpu_session, profiled, g, _expect(src, dst), m, 3, int((T > 0).sum()))


@pytest.mark.parametrize("buckets", [(76, 77), (0, 255)], ids=["adjacent", "xcd-group-edges"])
def test_balance_two_heavy_runs(gpu_session, profiled, _mix, buckets):
    """Two heavy out-runs: in adjacent buckets (their segments share lines), and
    in the first and the last bucket (the ends of the XCDs' groups of 32)."""
    src, dst, expect = _heavy_graph(_mix, 203 + buckets[0], [(buckets[0], 0.3), (buckets[1], 0.5)])
    T, ntiles = _run_pieces(_mix, src)
    for b in buckets:
        base, crumb = _lens(T[b], len(src), ntiles)
        assert MIN_TILES <= crumb < base
    g = _graph(gpu_session, src, dst)
    _three_queries(gpu_session, profiled, g, expect, len(src), 3, int((T > 0).sum()))


def test_balance_heavy_run_sorted_by_source(gpu_session, profiled, _mix):
    """The heavy run's rows lead the table in source order: its work per tile is
    far from uniform (the rule's documented limit).  The count only."""
    src, dst, expect = _heavy_graph(_mix, 207, [(77, 2.0)], sort_heavy=True)
    g = _graph(gpu_session, src, dst)
    for _ in range(3):
        assert _count(gpu_session, g) == expect


# ---------------------------------------------------------------- 5. empty and light runs
def test_balance_empty_and_light_runs(gpu_session, profiled, _mix):
    """Targets in 3 buckets, sources uniform but for bucket 9 (no source: T = 0,
    its rows moved to bucket 10) and bucket 20 (half its rows moved away: below
    the mean): the one-zone rule holds for them."""
    rng = np.random.default_rng(3)
    m = 1 << 20
    src = rng.integers(0, N, m)
    pool = np.concatenate([_ids_in_bucket(_mix, b) for b in (5, 100, 255)])
    dst = pool[rng.integers(0, len(pool), m)]
    b = _mix[0][src]
    to10 = _ids_in_bucket(_mix, 10)
    src[b == 9] = to10[rng.integers(0, len(to10), int((b == 9).sum()))]
    light = np.nonzero(b == 20)[0][::2]
    to30 = _ids_in_bucket(_mix, 30)
    src[light] = to30[rng.integers(0, len(to30), len(light))]
    src[:20000] = dst[20000:40000]
    src[_mix[0][src] == 9] = to10[0]
    T, ntiles = _run_pieces(_mix, src)
    assert T[9] == 0 and 0 < T[20] < 0.7 * T.mean()
    for r in (9, 20):
        base, crumb = _lens(T[r], m, ntiles)
        assert base == crumb
    assert _lens(0, m, ntiles) == (ntiles, ntiles)  # T = 0: one job that walks nothing
    expect = _expect(src, dst)
    assert expect > 0
    g = _graph(gpu_session, src, dst)
    _three_queries(gpu_session, profiled, g, expect, m, 3, int((T > 0).sum()))


# ---------------------------------------------------------------- 6. knobs
def test_balance_knobs(gpu_session, profiled, monkeypatch, _mix, _heavy_13):
    """The knobs are read per query.  Excess split off: the count is the
    default's and the jobs are the one-zone rule's for this graph; job split
    off: the count again, every job MIN_TILES long."""
    src, dst, expect = _heavy_13
    m = len(src)
    T, ntiles = _run_pieces(_mix, src)
    g = _graph(gpu_session, src, dst)
    assert _count(gpu_session, g) == expect  # builds
    profiled.step()
    assert _count(gpu_session, g) == expect  # the defaults
    d = profiled.step()
    print("c5_jobs, defaults:", d["c5_jobs"])
    assert d["c5_index_queries"] == 1
    monkeypatch.setenv("CAPF_C5_EXCESS_SPLIT", "0")
    for _ in range(2):
        assert _count(gpu_session, g) == expect
        d = profiled.step()
        print("c5_jobs, excess split off:", d["c5_jobs"], "one-zone rule:", _one_zone_jobs(T, m, ntiles))
        assert d["c5_index_queries"] == 1
        assert d["c5_jobs"] == _one_zone_jobs(T, m, ntiles)
    monkeypatch.delenv("CAPF_C5_EXCESS_SPLIT")
    monkeypatch.setenv("CAPF_C5_JOB_SPLIT", "0")
    assert _count(gpu_session, g) == expect
    d = profiled.step()
    assert d["c5_index_queries"] == 1
    assert d["c5_jobs"] == NB * -(-ntiles // MIN_TILES)
