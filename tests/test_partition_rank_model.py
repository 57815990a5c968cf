"""The row rule of the rasterizer's fused digit partition (csrc/lines.hip, ras_partition), stated in numpy.

A row is 64 consecutive keys of the stream.  Its keys are ranked stably by their digit on top of the wave's per-digit
counters.  The kernel has two forms of that rank:

* the fallback (the 8-ballot match-any form): the lanes of one digit form a class; rank = counter + lanes of my class below me,
  and the counter grows by the class size;
* the fast path, by RUNS of equal digit: a lane is a head if it is lane 0 or its digit differs from lane - 1's; a lane's run
  starts at the highest head at or below it and ends in front of the lowest head above it (or at 64).  It is taken only when
  every digit of the row owns ONE run and the row has at most RAS_RUNS_MAX heads — an exact test, not an approximation.  Then
  rank = counter + place in the run (= counter after the run's length was added - run length + place), and the counter grows by
  the run length.

Both are checked against a stable argsort by digit, row after row on shared counters, on random rows, A,B,A rows, rows of 5 to
64 heads, rows of one digit and rows whose tail is the last block's padding (digit `mask`, behind every key).  The adversarial
rows must take the fallback, the plain rows must not."""
import numpy as np
import pytest

RAS_RUNS_MAX = 4          # csrc/lines.hip
LANES = 64


def heads_and_runs(d):
    """(head flags, place of every lane in its run, length of every lane's run)"""
    d = np.asarray(d)
    head = np.ones(LANES, bool)
    head[1:] = d[1:] != d[:-1]
    H = sum(1 << i for i in range(LANES) if head[i])
    pos, length = np.zeros(LANES, int), np.zeros(LANES, int)
    for lane in range(LANES):
        le = H & ((2 << lane) - 1)                       # heads at or below me: bit 0 is always set
        start = le.bit_length() - 1                      # 63 - clz
        gt = H >> (lane + 1)                             # heads above me
        end = lane + 1 + ((gt & -gt).bit_length() - 1) if gt else LANES
        pos[lane], length[lane] = lane - start, end - start
    return head, pos, length


def row_is_fast(d):
    """every digit owns at most one run, and there are at most RAS_RUNS_MAX heads"""
    head, _, _ = heads_and_runs(d)
    hd = np.asarray(d)[head]
    return len(hd) <= RAS_RUNS_MAX and len(set(hd.tolist())) == len(hd)


def rank_fast(d, counters):
    """the kernel's fast path: every lane reads its digit's counter, the run's last lane adds the run's length"""
    d = np.asarray(d)
    _, pos, length = heads_and_runs(d)
    before = counters[d].copy()
    tail = np.ones(LANES, bool)
    tail[:-1] = d[:-1] != d[1:]
    for lane in np.flatnonzero(tail):
        assert pos[lane] + 1 == length[lane]
        counters[d[lane]] += pos[lane] + 1
    r = before + pos
    assert np.array_equal(r, counters[d] - length + pos)        # the issue's form: counter after the add - run length + place
    return r


def rank_fallback(d, counters):
    """the 8-ballot form: the class leader (no lane of the class below it) adds the class size; every lane reads it back"""
    d = np.asarray(d)
    same = d[:, None] == d[None, :]
    below = np.tril(same, -1).sum(1)
    cnt = same.sum(1)
    for lane in np.flatnonzero(below == 0):
        counters[d[lane]] += cnt[lane]
    return counters[d] - cnt + below


def rank_rows(rows, force_fallback=False):
    """ranks of a wave's rows on shared counters, and which rows took the fast path"""
    counters = np.zeros(256, int)
    out, fast = [], []
    for d in rows:
        f = row_is_fast(d) and not force_fallback
        out.append(rank_fast(d, counters) if f else rank_fallback(d, counters))
        fast.append(f)
    return np.concatenate(out), fast, counters


def reference(rows):
    """place of every key among the keys of its digit, in stream order: what a stable sort by digit gives"""
    d = np.concatenate(rows)
    order = np.argsort(d, kind="stable")
    place = np.empty(len(d), int)
    first = np.searchsorted(d[order], d[order], side="left")
    place[order] = np.arange(len(d)) - first
    return place


def runs_row(digits, lengths):
    d = np.repeat(np.asarray(digits), np.asarray(lengths))
    assert len(d) == LANES
    return d


def _check(rows, expect_fast=None):
    want = reference(rows)
    got, fast, counters = rank_rows(rows)
    assert np.array_equal(got, want)
    assert np.array_equal(counters, np.bincount(np.concatenate(rows), minlength=256))
    forced, fast2, _ = rank_rows(rows, force_fallback=True)          # ras_rank=0 / 2
    assert np.array_equal(forced, want) and not any(fast2)
    if expect_fast is not None:
        assert fast == list(expect_fast), fast
    return fast


def test_heads_and_run_lengths():
    d = runs_row([7, 3, 9], [10, 33, 21])
    head, pos, length = heads_and_runs(d)
    assert np.flatnonzero(head).tolist() == [0, 10, 43]
    assert pos.tolist() == list(range(10)) + list(range(33)) + list(range(21))
    assert length.tolist() == [10] * 10 + [33] * 33 + [21] * 21
    head, pos, length = heads_and_runs(np.full(LANES, 5))
    assert head.sum() == 1 and pos.tolist() == list(range(64)) and set(length.tolist()) == {64}
    head, pos, length = heads_and_runs(np.arange(LANES))
    assert head.all() and not pos.any() and set(length.tolist()) == {1}


def test_random_rows():
    rng = np.random.default_rng(1)
    for bins in (2, 3, 16, 256):
        rows = [rng.integers(0, bins, LANES) for _ in range(8)]
        _check(rows)


def test_random_runs_share_counters_across_rows():
    """a wave's eight rows: the same digits come back row after row, fast and fallback rows mixed"""
    rng = np.random.default_rng(2)
    for _ in range(50):
        rows = []
        for _j in range(8):
            n = int(rng.integers(1, 9))
            cuts = np.sort(rng.choice(np.arange(1, LANES), n - 1, replace=False)) if n > 1 else np.zeros(0, int)
            lengths = np.diff(np.concatenate([[0], cuts, [LANES]]))
            rows.append(runs_row(rng.integers(0, 6, n), lengths))
        _check(rows)


def test_aba_rows_take_the_fallback():
    aba = runs_row([4, 5, 4], [20, 20, 24])
    abab = runs_row([4, 5, 4, 5], [16, 16, 16, 16])
    abca = runs_row([1, 2, 3, 1], [1, 31, 31, 1])
    plain = runs_row([4, 5], [40, 24])
    assert _check([aba, abab, abca, plain, aba]) == [False, False, False, True, False]


@pytest.mark.parametrize("n_heads", [1, 2, 3, 4, 5, 6, 17, 63, 64])
def test_rows_by_head_count(n_heads):
    """distinct digits, so that only the count decides: up to RAS_RUNS_MAX heads are fast, 5 to 64 fall back"""
    lengths = [1] * (n_heads - 1) + [LANES - (n_heads - 1)]
    row = runs_row(np.arange(n_heads) + 100, lengths)
    fast = _check([row, row[::-1].copy(), row])
    assert fast == [n_heads <= RAS_RUNS_MAX] * 3


def test_rows_of_one_digit():
    rows = [np.full(LANES, 200)] * 8
    assert _check(rows) == [True] * 8
    got, _, counters = rank_rows(rows)
    assert np.array_equal(got, np.arange(512)) and counters[200] == 512


@pytest.mark.parametrize("n_keys", [0, 1, 63])
@pytest.mark.parametrize("mask", [63, 255])
def test_padding_tail(n_keys, mask):
    """the last block's positions beyond its keys carry digit `mask`: one run at the end of the row, behind every key — a real
    key of digit `mask` in front of other digits makes that digit come back, and the row falls back"""
    rng = np.random.default_rng(n_keys + mask)
    keys = np.full(n_keys, 9)
    row = np.concatenate([keys, np.full(LANES - n_keys, mask)])
    assert _check([row, np.full(LANES, mask)]) == [True, True]
    if n_keys >= 2:
        row2 = row.copy(); row2[0] = mask                              # mask, 9 .. 9, padding
        assert _check([row2]) == [False]
        row3 = row.copy(); row3[n_keys - 1] = mask                     # 9 .. 9, mask, padding: one run of `mask`
        assert _check([row3]) == [True]
        noisy = np.concatenate([rng.integers(0, mask + 1, n_keys), np.full(LANES - n_keys, mask)])
        _check([noisy])
    # the keys of the padded row rank in front of the padding within digit `mask`
    got, _, _ = rank_rows([np.concatenate([np.full(n_keys, mask), np.full(LANES - n_keys, mask)])])
    assert np.array_equal(got, np.arange(LANES))
