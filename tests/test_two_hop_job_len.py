"""The job-length rule of the indexed 2-hop count (csrc/c5_job_len.h), checked
on the host through capf_c5_job_len: no GPU.

A slot's cursor counts tiles; a taker looks at where it last saw the cursor
(possibly stale), picks a length by that position and adds the length to the
cursor.  Whatever the takers read, the ranges they claim must be disjoint and
cover [0, ntiles), no length may be 0, a run is never cut into more than
ceil(ntiles / min_tiles) jobs, and a run at or below the mean (and every run
with the excess split off) gets exactly the lengths of the one-zone rule:
k = round(T / W) ranges of ceil(ntiles / k) tiles, W = M / J, not below
min_tiles.
"""
import itertools

import numpy as np
import pytest

from capf_amd import _lib


@pytest.fixture(scope="module")
def job_len():
    f = _lib.load().capf_c5_job_len
    return lambda T, M, J, X, nt, mn, pos: int(f(T, M, J, X, nt, mn, pos))


def one_zone(T, M, J, nt, mn):
    W = max(1, M // J)
    k = max(1, (T + W // 2) // W)
    return min(nt, max(mn, -(-nt // k)))


GRID = [(T, M, nt, mn, J, X)
        for M in (1, 1000, 268435)
        for T in sorted({0, 1, M // 2, M, M + 1, M + max(1, M // 16), int(1.05 * M), int(1.27 * M), int(1.3 * M), 3 * M,
                         150 * M, 4000000000})
        for nt in (1, 2, 31, 128, 129, 8192, 70000)
        for mn in (1, 16, 32)
        for J, X in ((4, 4), (4, 1), (4, 2), (1, 4), (8, 64), (3, 5))
        if mn >= 16 or nt <= 129]  # (jobs of one tile: the short runs show all there is to them)


def test_grid_is_what_it_says():
    assert any(nt > 65536 for _, _, nt, _, _, _ in GRID)  # two lengths do not fit 16 bits each
    assert len(GRID) > 2000


def drain(job_len, T, M, nt, mn, J, X, rng, mode):
    """Takers draw until the cursor passes nt.  mode: how stale the position a
    taker picks by is — 'fresh' (the cursor itself), 'zero' (always 0), 'random'
    (any earlier cursor value), 'unset' mixes in takers that found no length
    stored yet and claim min_tiles."""
    cursor, seen, jobs = 0, [0], []
    while cursor < nt:
        if mode == "fresh":
            pos = cursor
        elif mode == "zero":
            pos = 0
        else:
            pos = seen[int(rng.integers(0, len(seen)))]
        ln = job_len(T, M, J, X, nt, mn, pos)
        if mode == "unset" and rng.random() < 0.3:
            ln = mn
        assert ln > 0
        jobs.append((cursor, min(cursor + ln, nt), ln))
        cursor += ln
        seen.append(min(cursor, nt - 1))
    return jobs


@pytest.mark.parametrize("mode", ["fresh", "zero", "random", "unset"])
def test_claims_partition_the_run(job_len, mode):
    rng = np.random.default_rng(5)
    for T, M, nt, mn, J, X in GRID:
        jobs = drain(job_len, T, M, nt, mn, J, X, rng, mode)
        # disjoint, covering: each job starts where the last ended
        assert jobs[0][0] == 0 and jobs[-1][1] == nt, (T, M, nt, mn, J, X)
        assert all(a[1] == b[0] for a, b in zip(jobs, jobs[1:])), (T, M, nt, mn, J, X)
        assert all(j[0] < j[1] for j in jobs)
        assert len(jobs) <= -(-nt // mn), (T, M, nt, mn, J, X, len(jobs))
        assert all(j[2] >= min(mn, nt) for j in jobs)


def test_at_or_below_the_mean_is_the_one_zone_rule(job_len):
    for T, M, nt, mn, J, X in GRID:
        W = max(1, M // J)
        if T > W * J and X:
            continue
        want = one_zone(T, M, J, nt, mn)
        for pos in (0, nt // 2, nt - 1):
            assert job_len(T, M, J, X, nt, mn, pos) == want, (T, M, nt, mn, J, X, pos)


def test_excess_split_off_is_the_one_zone_rule(job_len):
    for T, M, nt, mn, J, _ in GRID:
        want = one_zone(T, M, J, nt, mn)
        for pos in (0, nt // 2, nt - 1):
            assert job_len(T, M, J, 0, nt, mn, pos) == want, (T, M, nt, mn, J, pos)


def test_excess_below_one_crumb_is_the_one_zone_rule(job_len):
    M, J, X, nt, mn = 16000, 4, 4, 8192, 32
    W = M // J
    T = M + W // X - 1
    assert all(job_len(T, M, J, X, nt, mn, p) == one_zone(T, M, J, nt, mn) for p in (0, 4000, nt - 1))


def test_two_zones_of_a_heavy_run(job_len):
    """T = 1.27 M over 8192 tiles, J = 4, X = 4: the first ceil(8192 / 1.27) tiles
    in 4 base jobs, the rest in round(0.27 · 16) = 4 crumbs."""
    M, J, X, nt, mn = 100000, 4, 4, 8192, 32
    T = 127000
    B = -(-nt * M // T)
    base = -(-B // J)
    assert job_len(T, M, J, X, nt, mn, 0) == base
    assert job_len(T, M, J, X, nt, mn, J * base - 1) == base
    crumb = job_len(T, M, J, X, nt, mn, J * base)
    assert crumb == -(-(nt - J * base) // 4) and mn <= crumb < base
    assert job_len(T, M, J, X, nt, mn, nt - 1) == crumb
    jobs = drain(job_len, T, M, nt, mn, J, X, None, "fresh")
    assert [j[2] for j in jobs] == [base] * 4 + [crumb] * 4


def test_no_length_below_min_tiles_in_either_zone(job_len):
    for (T, M, nt, mn, J, X), pos in itertools.product(GRID[::7], (0, 1, 100, 5000, 69999)):
        if pos < nt:
            assert job_len(T, M, J, X, nt, mn, pos) >= min(mn, nt)
