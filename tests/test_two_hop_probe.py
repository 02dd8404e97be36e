"""Mode P of the partitioned 2-hop count (csrc/chain2_partitioned.hip): one P3
unit per bucket counts the in-run into LDS, then probes those counters with
the out-run's keys — no out histogram, no counter flush, no dot kernel; the
last unit writes the count.

Every assertion is exact equality with oracle.cmodel.count_2hop.  The bucket
count comes from the node-id range, not the rel count, so small rel tables
with CAPF_CHAIN2=partitioned reach the mode: ≥ 2^24 ids take it by default,
2^23 ids (128 buckets) with CAPF_C5_PROBE=1; CAPF_C5_PROBE=0 is mode A (both
sides counted, k_chain2_dot_pairs).
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


def _graph(session, src, dst, n, compact):
    m = len(src)
    rels = session.table([("id", T_INT, np.arange(m), None), ("source", T_INT, src, None),
                          ("target", T_INT, dst, None)])
    nodes = session.range_nodes(0, n, id_col="id")
    rels, nodes = compact_as(rels, compact), compact_as(nodes, compact)
    return ScanGraph(session, [ElementTable("node", frozenset(["V"]), nodes, {})],
                     [ElementTable("rel", frozenset(["E"]), rels, {})])


def _profiled_count(session, g):
    """(count, profile) of one synchronous 2-hop count with kernel timers on."""
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


@pytest.fixture(scope="module")
def _sparse_expect():
    """Closed-form counts of the 300001-rel R-MAT prefixes, once per (scale, nodes)."""
    memo = {}

    def expect(scale, nodes):
        if (scale, nodes) not in memo:
            src, dst = cmodel.rmat(scale, count=300001)
            memo[scale, nodes] = cmodel.count_2hop(src, dst, nodes or 1 << scale)
        return memo[scale, nodes]
    return expect


@pytest.mark.parametrize("probe", ["1", "0"], ids=["probe", "mode_a"])
@pytest.mark.parametrize("compact", [False, True, 3], ids=["int64", "for32", "for24"])
@pytest.mark.parametrize("scale,nodes", [(24, None), (24, 12_000_001), (25, None), (25, 20_000_003), (23, None)])
def test_probe_parity_with_mode_a(gpu_session, monkeypatch, _sparse_expect, probe, compact, scale, nodes):
    """Scale 24: 256 buckets, the small P1 shape; scale 25: the big P1 shape
    with the 32-bit mix; the clipped node tables take the range-checked P1 and
    the dummy run; scale 23: 128 buckets, mode P only when forced.  Two queries
    back to back: the second reuses the session's scratch as the first left it."""
    monkeypatch.setenv("CAPF_CHAIN2", "partitioned")
    monkeypatch.setenv("CAPF_C5_PROBE", probe)
    g = rmat_graph(gpu_session, scale, compact=compact, count=300001, n_nodes=nodes)
    expect = _sparse_expect(scale, nodes)
    for _ in range(2):
        got = run(g, TWO_HOP)[0]["count"]
        assert gpu_session.last_plan() == "fused_chain2"
        assert got == expect


@pytest.mark.parametrize("scale,probe,dot", [(24, None, False), (24, "0", True), (23, None, True), (23, "1", False)])
def test_probe_mode_selection(gpu_session, monkeypatch, _sparse_expect, scale, probe, dot):
    """Mode P launches no dot kernel: the default from 256 buckets, forced by
    CAPF_C5_PROBE at 128."""
    monkeypatch.setenv("CAPF_CHAIN2", "partitioned")
    if probe is None:
        monkeypatch.delenv("CAPF_C5_PROBE", raising=False)
    else:
        monkeypatch.setenv("CAPF_C5_PROBE", probe)
    g = rmat_graph(gpu_session, scale, compact=True, count=300001)
    got, prof = _profiled_count(gpu_session, g)
    assert got == _sparse_expect(scale, None)
    assert "c5_gather" in prof
    assert ("chain2_dot" in prof) == dot


@pytest.mark.parametrize("compact", [False, 3], ids=["int64", "for24"])
def test_probe_nearly_empty_buckets(gpu_session, monkeypatch, compact):
    """1000 rels over 2^24 ids: most buckets have no keys on one or both sides
    (the walker's empty-batch and empty-run paths)."""
    monkeypatch.setenv("CAPF_CHAIN2", "partitioned")
    rng = np.random.default_rng(5)
    n = 1 << BITS
    src = rng.integers(0, n, 1000)
    dst = rng.integers(0, n, 1000)
    dst[:200] = src[200:400]  # some real 2-hop paths
    dst[990:] = src[990:]     # self-loops
    g = _graph(gpu_session, src, dst, n, compact)
    expect = cmodel.count_2hop(src.astype(np.int64), dst.astype(np.int64), n)
    assert expect > 0
    for _ in range(2):
        assert run(g, TWO_HOP)[0]["count"] == expect
        assert gpu_session.last_plan() == "fused_chain2"


def _ids_in_bucket(bucket, want_low=None):
    """Node ids whose mixed key lies in `bucket` (optionally with key < want_low), ascending."""
    ids = np.arange(1 << BITS, dtype=np.int64)
    h = nodemix.node_mix(ids, BITS)
    ok = (h >> 16) == bucket
    if want_low is not None:
        ok &= (h & 0xFFFF) < want_low
    return ids[ok], h[ok] & 0xFFFF


@pytest.fixture(scope="module")
def _hot_graph():
    """2^20 rels over 2^24 ids: an in-hub of degree 300,000 (nine hand-offs)
    that also sources 200,000 rels (its hot half is probed constantly) with
    50,000 self-loops, a second in-hub in another bucket, and an in-hub of
    degree 45,000 sourcing 3,000 rels whose mixed key is below 64 (a hot
    pad-corrected bin)."""
    rng = np.random.default_rng(17)
    n, m = 1 << BITS, 1 << 20
    src = rng.integers(0, n, m)
    dst = rng.integers(0, n, m)
    hub = 9
    hub_bucket = int(nodemix.node_mix([hub], BITS)[0]) >> 16
    hub2 = next(int(i) for i in range(4_500_000, 4_600_000)
                if int(nodemix.node_mix([i], BITS)[0]) >> 16 != hub_bucket)
    pad_ids, pad_keys = _ids_in_bucket((hub_bucket + 7) % 256, want_low=64)
    hubp = int(pad_ids[0])
    assert pad_keys[0] < 64
    dst[100000:400000] = hub
    src[350000:550000] = hub      # [350000, 400000): self-loops on the hub
    dst[600000:700000] = hub2
    src[690000:720000] = hub2
    dst[750000:795000] = hubp
    src[800000:803000] = hubp
    dst[900000:900100] = src[900000:900100]
    expect = cmodel.count_2hop(src.astype(np.int64), dst.astype(np.int64), n)
    return src, dst, n, expect


@pytest.mark.parametrize("compact", [False, True, 3], ids=["int64", "for32", "for24"])
def test_probe_hot_keys(gpu_session, monkeypatch, _hot_graph, compact):
    """Counters past 2^15 live in the unit's LDS hot table (nothing reaches
    the global log); synchronous and asynchronous counts."""
    monkeypatch.setenv("CAPF_CHAIN2", "partitioned")
    monkeypatch.delenv("CAPF_C5_PROBE", raising=False)
    src, dst, n, expect = _hot_graph
    g = _graph(gpu_session, src, dst, n, compact)
    got, prof = _profiled_count(gpu_session, g)
    assert got == expect
    assert "chain2_dot" not in prof
    assert prof.get("c3_handoffs", {"bytes": 0})["bytes"] == 0
    assert _async_count(gpu_session, g) == expect
    assert run(g, TWO_HOP)[0]["count"] == expect


@pytest.fixture(scope="module")
def _full_table_graph():
    """Six in-hubs of degree ≥ 33,000 in one bucket (one of degree 70,000: two
    hand-offs; one with a mixed key below 64: a pad-corrected bin; two sharing
    an LDS word: keys k and k + 2^15), each sourcing 1,000 rels."""
    rng = np.random.default_rng(23)
    n, m = 1 << BITS, 1 << 20
    src = rng.integers(0, n, m)
    dst = rng.integers(0, n, m)
    bucket = 101
    ids, keys = _ids_in_bucket(bucket)
    by_key = {int(k): int(i) for i, k in zip(ids, keys)}
    pair = next(k for k in range(64, 1 << 15) if k in by_key and k + (1 << 15) in by_key)
    low = next(k for k in range(64) if k in by_key)
    others = [k for k in sorted(by_key) if k not in (pair, pair + (1 << 15), low)][1000:1003]
    hubs = [by_key[k] for k in (pair, pair + (1 << 15), low, *others)]
    assert len(set(hubs)) == 6
    degs = [33000, 34000, 35000, 70000, 33500, 36000]
    pos = 0
    for h, d in zip(hubs, degs):
        dst[pos:pos + d] = h
        pos += d
    for i, h in enumerate(hubs):
        src[pos + 1000 * i:pos + 1000 * (i + 1)] = h
    src[0:500] = hubs[0]  # self-loops on a hub
    expect = cmodel.count_2hop(src.astype(np.int64), dst.astype(np.int64), n)
    return src, dst, n, expect


@pytest.mark.parametrize("compact", [False, 3], ids=["int64", "for24"])
def test_probe_hot_table_full(gpu_session, monkeypatch, _full_table_graph, compact):
    """CAPF_C5_HOTCAP=2: four of the six hubs overflow the hot table into the
    global log (≥ one hand-off + one remainder entry each); the count is exact."""
    monkeypatch.setenv("CAPF_CHAIN2", "partitioned")
    monkeypatch.setenv("CAPF_C5_HOTCAP", "2")
    monkeypatch.delenv("CAPF_C5_PROBE", raising=False)
    src, dst, n, expect = _full_table_graph
    g = _graph(gpu_session, src, dst, n, compact)
    got, prof = _profiled_count(gpu_session, g)
    assert got == expect
    assert "chain2_dot" not in prof
    assert prof["c3_handoffs"]["bytes"] >= 8
    assert _async_count(gpu_session, g) == expect
