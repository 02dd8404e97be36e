"""Mode P with phase 2 shared between units (csrc/chain2_partitioned.hip): a
unit that publishes copies its bucket's image (the 2^16 halves, the special
keys, the bucket id) into a slot of the work area and hands its out-run out
as jobs of CAPF_C5_STEAL_TILES tiles; units that have finished their own
bucket load a ready image and take jobs.

Every assertion on a count is exact equality with oracle.cmodel.count_2hop.
CAPF_C5_STEAL: 0 = off, unset = heavy units publish, all = every unit
publishes, reload = every unit publishes and re-reads its own image from the
slot before its first job — the helper's path (publish, acquire, load, job
loop, per-job correction) run deterministically.  Whether another unit really
helps is timing, so nothing here asserts c5_steals > 0.  Job size 16 tiles
throughout: 2^22 rels (256 tiles) are 16 jobs per bucket.
"""
import numpy as np
import pytest

from capf_amd.expr import CountStar, T_INT
from capf_amd.graph import ElementTable, ScanGraph
from capf_amd.planner import Match, NodeP, Query, RelP, Stage, plan_query, run
from capf_amd.synthetic import rmat_graph
from capf_amd.table import compact_as
from oracle import cmodel, nodemix

pytestmark = pytest.mark.gpu

TWO_HOP = Query([Match([NodeP("a"), NodeP("b"), NodeP("c")], [RelP("r1", "a", "b"), RelP("r2", "b", "c")])],
                [Stage([("count", CountStar())])])
BITS = 24  # ids of the hand-built graphs: 256 buckets, mode P by default
N = 1 << BITS
TILE = 16384  # rels per P1 tile at ≤ 2^24 ids


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("CAPF_CHAIN2", "partitioned")
    monkeypatch.setenv("CAPF_C5_STEAL_TILES", "16")
    monkeypatch.delenv("CAPF_C5_PROBE", raising=False)
    monkeypatch.delenv("CAPF_C5_STEAL", raising=False)


def _steal(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("CAPF_C5_STEAL", raising=False)
    else:
        monkeypatch.setenv("CAPF_C5_STEAL", mode)


def _graph(session, src, dst, n, compact):
    m = len(src)
    rels = session.table([("id", T_INT, np.arange(m), None), ("source", T_INT, src, None),
                          ("target", T_INT, dst, None)])
    nodes = session.range_nodes(0, n, id_col="id")
    rels, nodes = compact_as(rels, compact), compact_as(nodes, compact)
    return ScanGraph(session, [ElementTable("node", frozenset(["V"]), nodes, {})],
                     [ElementTable("rel", frozenset(["E"]), rels, {})])


def _count(session, g):
    got = run(g, TWO_HOP)[0]["count"]
    assert session.last_plan() == "fused_chain2"
    return got


def _profiled_count(session, g):
    session.set_profiling(True)
    try:
        session.reset_profile()
        got = run(g, TWO_HOP)[0]["count"]
        prof = session.profile()
    finally:
        session.set_profiling(False)
    assert session.last_plan() == "fused_chain2"
    return got, prof


def _async_count(session, g):
    import torch
    slot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    plan_query(g, TWO_HOP).table.count_async(slot.data_ptr())
    session.sync()
    return slot.item()


def _expect(src, dst, n=N):
    return cmodel.count_2hop(np.ascontiguousarray(src, dtype=np.int64), np.ascontiguousarray(dst, dtype=np.int64), n)


def _bucket_keys():
    """(bucket, key) of every id below 2^24 under the node mix."""
    h = nodemix.node_mix(np.arange(N, dtype=np.int64), BITS)
    return h >> 16, h & 0xFFFF


@pytest.fixture(scope="module")
def _mix():
    return _bucket_keys()


def _ids_in_bucket(mix, bucket, want_low=None):
    b, k = mix
    ok = b == bucket
    if want_low is not None:
        ok &= k < want_low
    ids = np.nonzero(ok)[0].astype(np.int64)
    return ids, k[ids]


@pytest.fixture(scope="module")
def _skewed(_mix):
    """2^22 rels: 60 % of the sources are drawn from 40,000 distinct ids of
    bucket 77 (its out-run holds ~150 × the mean), targets uniform."""
    rng = np.random.default_rng(41)
    m = 1 << 22
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    ids, _ = _ids_in_bucket(_mix, 77)
    pool = ids[:40000]
    heavy = rng.random(m) < 0.6
    src[heavy] = pool[rng.integers(0, len(pool), int(heavy.sum()))]
    dst[:5000] = src[5000:10000]  # paths through the heavy bucket's sources too
    return src, dst, _expect(src, dst)


@pytest.mark.parametrize("compact", [False, 3], ids=["int64", "for24"])
@pytest.mark.parametrize("mode", ["0", None, "all", "reload"], ids=["off", "default", "all", "reload"])
def test_steal_skewed_out_run(gpu_session, monkeypatch, _skewed, mode, compact):
    """One bucket's out-run dwarfs the others: its unit publishes in every
    mode but off.  Two queries back to back (the second meets the work area
    as the first left it), then the asynchronous count."""
    _steal(monkeypatch, mode)
    src, dst, expect = _skewed
    g = _graph(gpu_session, src, dst, N, compact)
    for _ in range(2):
        assert _count(gpu_session, g) == expect
    assert _async_count(gpu_session, g) == expect


@pytest.fixture(scope="module")
def _hot(_mix):
    """The hot-key shape of test_two_hop_probe at 2^22 rels (16 jobs per
    bucket): an in-hub of degree 300,000 sourcing 200,000 rels with 50,000
    self-loops, a second in-hub in another bucket, an in-hub of degree 45,000
    whose mixed key is below 64 (a hot pad-corrected bin), and an in-hub of
    degree 70,000 in a fourth bucket (a special key: in-degree ≥ 2^16)
    sourcing 20,000 rels."""
    rng = np.random.default_rng(17)
    m = 1 << 22
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    b, _ = _mix
    hub = 9
    hub_bucket = int(b[hub])
    hub2 = next(i for i in range(4_500_000, 4_600_000) if int(b[i]) != hub_bucket)
    pad_ids, pad_keys = _ids_in_bucket(_mix, (hub_bucket + 7) % 256, want_low=64)
    hubp = int(pad_ids[0])
    assert pad_keys[0] < 64
    hub3 = next(i for i in range(9_000_000, 9_100_000)
                if int(b[i]) not in (hub_bucket, int(b[hub2]), (hub_bucket + 7) % 256))
    dst[100000:400000] = hub
    src[350000:550000] = hub      # [350000, 400000): self-loops on the hub
    dst[600000:700000] = hub2
    src[690000:720000] = hub2
    dst[750000:795000] = hubp
    src[800000:803000] = hubp
    dst[900000:900100] = src[900000:900100]
    dst[1000000:1070000] = hub3
    src[1100000:1120000] = hub3
    return src, dst, _expect(src, dst)


@pytest.mark.parametrize("compact", [False, 3], ids=["int64", "for24"])
@pytest.mark.parametrize("mode", ["reload", "all"])
def test_steal_hot_special_and_pad_keys(gpu_session, monkeypatch, _hot, mode, compact):
    """Specials, hot pad bins and the per-job correction stay exact when a
    bucket's out-run is cut into 16 jobs against a re-read (or helped) image."""
    _steal(monkeypatch, mode)
    src, dst, expect = _hot
    g = _graph(gpu_session, src, dst, N, compact)
    got, prof = _profiled_count(gpu_session, g)
    assert got == expect
    assert "chain2_dot" not in prof
    assert prof.get("c3_handoffs", {"bytes": 0})["bytes"] == 0
    assert _async_count(gpu_session, g) == expect


@pytest.fixture(scope="module")
def _full_table(_mix):
    """Six in-hubs of degree ≥ 33,000 in one bucket (one of degree 70,000; one
    with a mixed key below 64; two sharing an LDS word), each sourcing 1,000 rels."""
    rng = np.random.default_rng(23)
    m = 1 << 20
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    ids, keys = _ids_in_bucket(_mix, 101)
    by_key = {int(k): int(i) for i, k in zip(ids, keys)}
    pair = next(k for k in range(64, 1 << 15) if k in by_key and k + (1 << 15) in by_key)
    low = next(k for k in range(64) if k in by_key)
    others = [k for k in sorted(by_key) if k not in (pair, pair + (1 << 15), low)][1000:1003]
    hubs = [by_key[k] for k in (pair, pair + (1 << 15), low, *others)]
    assert len(set(hubs)) == 6
    pos = 0
    for h, d in zip(hubs, [33000, 34000, 35000, 70000, 33500, 36000]):
        dst[pos:pos + d] = h
        pos += d
    for i, h in enumerate(hubs):
        src[pos + 1000 * i:pos + 1000 * (i + 1)] = h
    src[0:500] = hubs[0]  # self-loops on a hub
    return src, dst, _expect(src, dst)


@pytest.mark.parametrize("compact", [False, 3], ids=["int64", "for24"])
def test_steal_hot_table_full(gpu_session, monkeypatch, _full_table, compact):
    """CAPF_C5_HOTCAP=2: four hubs' counts go to the global log, their halves
    become 0xFFFF, and the jobs resolve them from the log through the re-read image."""
    _steal(monkeypatch, "reload")
    monkeypatch.setenv("CAPF_C5_HOTCAP", "2")
    src, dst, expect = _full_table
    g = _graph(gpu_session, src, dst, N, compact)
    got, prof = _profiled_count(gpu_session, g)
    assert got == expect
    assert "chain2_dot" not in prof
    assert prof["c3_handoffs"]["bytes"] >= 8
    assert _async_count(gpu_session, g) == expect


@pytest.mark.parametrize("mode", ["all", "reload"])
def test_steal_nearly_empty_buckets(gpu_session, monkeypatch, mode):
    """1000 rels over 2^24 ids (one ragged tile, one job): most buckets are
    empty on one or both sides."""
    _steal(monkeypatch, mode)
    rng = np.random.default_rng(5)
    src = rng.integers(0, N, 1000)
    dst = rng.integers(0, N, 1000)
    dst[:200] = src[200:400]
    dst[990:] = src[990:]
    g = _graph(gpu_session, src, dst, N, 3)
    expect = _expect(src, dst)
    assert expect > 0
    for _ in range(2):
        assert _count(gpu_session, g) == expect


@pytest.mark.parametrize("mode", [None, "all", "reload"], ids=["default", "all", "reload"])
def test_steal_ragged_jobs(gpu_session, monkeypatch, mode):
    """37 full tiles and a partial one: jobs of 16, 16 and 6 tiles, the last
    tile ragged; half the sources in one bucket so the default publishes too."""
    _steal(monkeypatch, mode)
    rng = np.random.default_rng(59)
    m = 37 * TILE + 1234
    src = rng.integers(0, N, m)
    dst = rng.integers(0, N, m)
    ids, _ = _ids_in_bucket(_bucket_keys(), 200)
    half = rng.random(m) < 0.5
    src[half] = ids[rng.integers(0, 30000, int(half.sum()))]
    dst[:3000] = src[3000:6000]
    g = _graph(gpu_session, src, dst, N, 3)
    expect = _expect(src, dst)
    for _ in range(2):
        assert _count(gpu_session, g) == expect


def test_steal_no_stale_image(gpu_session, monkeypatch, _skewed):
    """Graph X, then Y (same shape, other data: the same slots carry other
    images), then X again in one session under `all`."""
    _steal(monkeypatch, "all")
    xs, xd, xe = _skewed
    rng = np.random.default_rng(43)
    perm = rng.permutation(len(xs))
    ys, yd = xs[perm], rng.integers(0, N, len(xs))
    ye = _expect(ys, yd)
    assert ye != xe
    gx = _graph(gpu_session, xs, xd, N, 3)
    gy = _graph(gpu_session, ys, yd, N, 3)
    assert _count(gpu_session, gx) == xe
    assert _count(gpu_session, gy) == ye
    assert _count(gpu_session, gx) == xe


@pytest.mark.parametrize("scale,nodes,mode", [(24, 12_000_001, "reload"), (25, None, "reload"), (25, None, "all")])
def test_steal_clipped_and_big_p1(gpu_session, monkeypatch, scale, nodes, mode):
    """12,000,001 nodes: the range-checked P1 and the dummy run; scale 25: the
    big P1 shape, 512 buckets — more units than CUs."""
    _steal(monkeypatch, mode)
    g = rmat_graph(gpu_session, scale, compact=True, count=300001, n_nodes=nodes)
    src, dst = cmodel.rmat(scale, count=300001)
    expect = cmodel.count_2hop(src, dst, nodes or 1 << scale)
    for _ in range(2):
        assert _count(gpu_session, g) == expect


def test_steal_off_switch(gpu_session, monkeypatch, _skewed):
    """CAPF_C5_STEAL=0 launches what the mode launched before: c5_gather, no dot;
    nothing is stolen."""
    _steal(monkeypatch, "0")
    src, dst, expect = _skewed
    g = _graph(gpu_session, src, dst, N, 3)
    got, prof = _profiled_count(gpu_session, g)
    assert got == expect
    assert "c5_gather" in prof
    assert "chain2_dot" not in prof
    assert prof.get("c5_steals", {"bytes": 0})["bytes"] == 0
