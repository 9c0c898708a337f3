"""GPU tests of the k-NN search and vote (lafs_knn_search / lafs_knn_vote, csrc/knn.hip) through the C entry points, against
tests/knn_oracle.py: scores in float64, the ranking order as a Python sort, votes in float64.

Score bound (fixed, derivable): any order of D float32 products and additions, fused or not, is within
b = (D + 2) 2^-24 sum_d |a_d b_d| of the float64 value.  Every returned score is held to b against the oracle's score of the pair the
device names.  Selection is checked so that near-ties cannot fail: with B the largest b of the query's row and s_k the oracle's k-th
score, every returned position has a float64 score >= s_k - 2B and every position left out one <= s_k + 2B (the device orders by
scores that are within b of the float64 ones, and at most k - 1 positions lie above s_k, at least k at or above it).

Boundaries of the kernel: 64 queries per workgroup, 32 per MFMA block, 16 per selecting wave; 128 bank rows per tile, 64 per wave,
32 per MFMA block; 32 columns of D per LDS chunk, 4 per load; list entries 64 per lane slot (k = 64 | 65, 128 | 129, 192 | 193).

Vote bound: each vote within g * vote64, g = (ks + 32) 2^-23 (the exponent's rounding, expf, ks - 1 additions of positive terms).
The oracle takes the temperature as the float32 the entry point receives."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu

import knn_oracle as KO  # noqa: E402
from lafs_cvpr2024_amd import _lib  # noqa: E402
from lafs_cvpr2024_amd.ops import _p  # noqa: E402

DEV = "cuda"
GUARD, SENTINEL = 3, 1.0e30


def rows(seed, n, D, unit=True):
    x = np.random.RandomState(seed).randn(n, D).astype(np.float32)
    if unit and D > 4:
        x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return x


def guarded(x, extra_ld=0):
    """x between guard rows and guard columns of a sentinel that would wreck any score it entered; the view is 16-byte aligned."""
    n, D = x.shape
    ld = 4 + (D + 3) // 4 * 4 + 4 + extra_ld
    big = torch.full((n + 2 * GUARD, ld), SENTINEL, device=DEV, dtype=torch.float32)
    big[GUARD:GUARD + n, 4:4 + D] = torch.from_numpy(x).to(DEV)
    return big, big[GUARD:GUARD + n, 4:4 + D]


def guards_intact(big, x):
    n, D = x.shape
    g = big.cpu().numpy()
    m = np.ones(g.shape, bool)
    m[GUARD:GUARD + n, 4:4 + D] = False
    return bool(np.all(g[m] == np.float32(SENTINEL))) and np.array_equal(g[GUARD:GUARD + n, 4:4 + D], x, equal_nan=True)


def raw_search(bank_v, query_v, k, pos0=0, exclude=None, merge=False, splits=0, out=None, ws_bytes=None, D=None):
    """The C entry point itself -> (status, top_score, top_idx) with the outputs between guard rows of their own."""
    h = _lib.lib()
    (N, Dv), Q = bank_v.shape, query_v.shape[0]
    D = Dv if D is None else D
    if out is None:
        bs = torch.full((Q + 2 * GUARD, k), -7.0, device=DEV, dtype=torch.float32)
        bi = torch.full((Q + 2 * GUARD, k), -7, device=DEV, dtype=torch.int32)
    else:
        bs, bi = out
    ts, ti = bs[GUARD:GUARD + Q], bi[GUARD:GUARD + Q]
    need = int(h.lafs_knn_workspace(Q, N, k, splits))
    nb = need if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nb, 1), device=DEV, dtype=torch.uint8)
    ex = None if exclude is None else torch.tensor(np.asarray(exclude, np.int32), device=DEV)
    rc = h.lafs_knn_search(_p(bank_v), bank_v.stride(0), N, pos0, _p(query_v), query_v.stride(0), Q, D, k, _p(ex), 1 if merge else 0,
                           splits, _p(ts), _p(ti), _p(ws) if nb else None, nb, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    s, i = bs.cpu().numpy(), bi.cpu().numpy()
    assert np.all(s[:GUARD] == -7) and np.all(s[GUARD + Q:] == -7) and np.all(i[:GUARD] == -7) and np.all(i[GUARD + Q:] == -7)
    return rc, s[GUARD:GUARD + Q], i[GUARD:GUARD + Q], (bs, bi)


def check(bank, query, k, pos0=0, exclude=None, splits=0, extra_ld=0):
    """Everything the header promises about one search; -> (top_score, top_idx, worst error / bound)."""
    N, D = bank.shape
    Q = query.shape[0]
    bb, bv = guarded(bank, extra_ld)
    qb, qv = guarded(query, extra_ld)
    rc, ts, ti, _ = raw_search(bv, qv, k, pos0, exclude, splits=splits)
    assert rc == 0, _lib.lib().lafs_last_error()
    assert guards_intact(bb, bank) and guards_intact(qb, query)
    S, B = KO.scores(bank, query), KO.bound(bank, query)
    worst = 0.0
    for i in range(Q):
        ex = -1 if exclude is None else int(exclude[i])
        cand = [j for j in range(N) if pos0 + j != ex]
        n = min(k, len(cand))
        assert np.all(ti[i, n:] == -1) and np.isnan(ts[i, n:]).all(), (i, ti[i], ts[i])
        got = ti[i, :n].astype(np.int64) - pos0
        assert np.all((got >= 0) & (got < N)) and len(set(got.tolist())) == n and ex - pos0 not in got.tolist()
        for r in range(n):
            j, dev = int(got[r]), float(ts[i, r])
            if S[i, j] != S[i, j] or dev != dev:
                assert S[i, j] != S[i, j] and dev != dev, (i, j, dev, S[i, j])
            else:
                e = abs(dev - S[i, j])
                assert e <= B[i, j], (i, j, dev, S[i, j], e, B[i, j])
                if B[i, j] > 0:
                    worst = max(worst, e / B[i, j])
            assert r == 0 or KO.before(ts[i, r - 1], ti[i, r - 1], ts[i, r], ti[i, r]), (i, r, ts[i, :n], ti[i, :n])
        order = KO.rank(S[i, cand], cand)
        s_k = S[i, order[n - 1]] if n else float("nan")
        left = np.setdiff1d(np.asarray(cand, np.int64), got)
        if s_k == s_k:
            Bm = np.nanmax(B[i, cand])
            with np.errstate(invalid="ignore"):
                assert not (S[i, got] < s_k - 2 * Bm).any(), (i, "a returned position lies below the k-th score")
                assert not (S[i, left] > s_k + 2 * Bm).any(), (i, "a position left out lies above the k-th score")
        elif len(left):                                      # the k-th is a NaN: only later NaNs may be left out
            assert np.isnan(S[i, left]).all() and left.min() > got[n - 1]
    return ts, ti, worst


SHAPES = [  # (n_query, n_bank, D, k)
    (1, 1, 1, 1), (1, 37, 4, 10), (70, 1000, 48, 10), (130, 4500, 64, 200), (70, 1000, 100, 256), (3, 333, 384, 200),
    (5, 300, 1024, 10), (63, 127, 31, 64), (64, 128, 32, 65), (65, 129, 33, 128), (16, 257, 5, 129), (17, 256, 3, 192),
    (33, 255, 36, 193), (32, 64, 28, 1), (2, 65, 7, 63), (70, 37, 48, 200), (9, 100, 64, 256),
]


@pytest.mark.parametrize("Q,N,D,k", SHAPES)
def test_search_shapes(Q, N, D, k):
    bank, query = rows(1000 + N + D, N, D), rows(2000 + Q + D, Q, D)
    _, _, worst = check(bank, query, k)
    print(f"\nknn search Q={Q} N={N} D={D} k={k}: worst error/bound {worst:.3f}")


def test_search_wide_rows():
    """ldb > D and ldq > D by more than the guard columns (a feature slice of a wider table)."""
    _, _, worst = check(rows(1, 300, 48), rows(2, 20, 48), 10, extra_ld=64)
    print(f"\nknn search wide rows: worst error/bound {worst:.3f}")


def test_duplicates_resolve_by_position():
    bank = rows(3, 200, 48)
    bank[50:150] = bank[7]
    query = np.concatenate([bank[7:8], rows(4, 4, 48)])
    ts, ti, _ = check(bank, query, 64)
    assert ti[0, 0] == 7 and list(ti[0, 1:64]) == list(range(50, 113))
    for i in range(5):
        same = [p for p in ti[i] if 50 <= p < 150]
        assert same == sorted(same)


def test_nan_row_ranks_last():
    bank = rows(5, 140, 48)
    bank[3, 5] = np.nan
    bank[130, 0] = np.nan
    query = rows(6, 5, 48)
    ts, ti, _ = check(bank, query, 140)
    assert np.all(ti[:, 138] == 3) and np.all(ti[:, 139] == 130) and np.isnan(ts[:, 138:]).all() and not np.isnan(ts[:, :138]).any()
    ts, ti, _ = check(bank, query, 10)
    assert not np.isnan(ts).any()


def test_exclude_is_leave_one_out():
    x = rows(7, 150, 48)
    ts, ti, _ = check(x, x, 10, exclude=np.arange(150))
    assert not np.any(ti == np.arange(150)[:, None])
    ts2, ti2, _ = check(x, x, 10, exclude=np.full(150, -1))
    assert np.all(ti2[:, 0] == np.arange(150))


def test_bank_pos0():
    bank, query = rows(8, 300, 48), rows(9, 70, 48)
    ts0, ti0, _ = check(bank, query, 20)
    ts1, ti1, _ = check(bank, query, 20, pos0=1_000_000, exclude=np.full(70, 1_000_005))
    ts2, ti2, _ = check(bank, query, 20, exclude=np.full(70, 5))
    assert ts1.tobytes() == ts2.tobytes() and np.array_equal(ti1, ti2 + 1_000_000)
    big = (1 << 31) - 1 - 300
    ts3, ti3, _ = check(bank, query, 20, pos0=big)
    assert ts3.tobytes() == ts0.tobytes() and np.array_equal(ti3.astype(np.int64), ti0.astype(np.int64) + big)


@pytest.mark.parametrize("Q,N,D,k", [(70, 1000, 48, 200), (5, 4500, 100, 256), (130, 700, 64, 10)])
def test_bit_identity(Q, N, D, k):
    """One call, three uneven chunks in both orders with merge, and splits in {1, 2, 7, auto}: the same bytes."""
    bank, query = rows(10, N, D), rows(11, Q, D)
    bank[N // 2] = bank[3]                                  # an exact tie across chunks and splits
    ref_s, ref_i, _ = check(bank, query, k, splits=1)
    _, bv = guarded(bank)
    _, qv = guarded(query)
    for splits in (2, 7, 0, 32):
        rc, s, i, _ = raw_search(bv, qv, k, splits=splits)
        assert rc == 0 and s.tobytes() == ref_s.tobytes() and i.tobytes() == ref_i.tobytes(), splits
    cuts = [0, N // 7, N // 7 + N // 2 + 1, N]
    chunks = [(cuts[c], cuts[c + 1]) for c in range(3)]
    for order in (chunks, chunks[::-1]):
        for splits in (1, 3):
            out = None
            for n, (a, b) in enumerate(order):
                _, cv = guarded(bank[a:b])
                rc, s, i, out = raw_search(cv, qv, k, pos0=a, merge=n > 0, splits=splits, out=out)
                assert rc == 0
            assert s.tobytes() == ref_s.tobytes() and i.tobytes() == ref_i.tobytes(), (order, splits)


def test_refusals_write_nothing():
    bank, query = rows(12, 300, 48), rows(13, 10, 48)
    _, bv = guarded(bank)
    _, qv = guarded(query)

    def refused(**kw):
        a = dict(bank_v=bv, query_v=qv, k=10)
        a.update(kw)
        rc, s, i, _ = raw_search(**a)
        assert rc < 0 and np.all(s == -7) and np.all(i == -7), kw

    refused(k=257)
    refused(k=0)
    refused(splits=2, ws_bytes=int(_lib.lib().lafs_knn_workspace(10, 300, 10, 2)) - 4)
    flat = torch.zeros(400 * 1100, device=DEV)
    refused(bank_v=flat[:300 * 1028].view(300, 1028), query_v=flat[:10 * 1028].view(10, 1028), D=1025)
    refused(bank_v=flat[1:1 + 300 * 48].view(300, 48))                     # base not 16-byte aligned
    refused(query_v=flat[2:2 + 10 * 48].view(10, 48))
    refused(bank_v=flat[:300 * 50].view(300, 50)[:, :48])                   # ldb % 4 != 0
    refused(bank_v=flat[:300 * 52].view(300, 52), D=56)                     # ld < D
    assert int(_lib.lib().lafs_knn_workspace(10, 300, 10, 1)) == 0
    assert int(_lib.lib().lafs_knn_workspace(10, 300, 10, 2)) == 2 * 10 * 10 * 8


# ------------------------------------------------------------------------------------------------------------------ vote
def raw_vote(ts, ti, labels, ks, T):
    h = _lib.lib()
    Q, k = ts.shape
    d_s, d_i = torch.tensor(ts, device=DEV), torch.tensor(np.asarray(ti, np.int32), device=DEV)
    d_l = torch.tensor(np.asarray(labels, np.int32), device=DEV)
    pred = torch.full((len(ks), Q, 5), -9, device=DEV, dtype=torch.int32)
    vote = torch.full((len(ks), Q, 5), -9.0, device=DEV, dtype=torch.float32)
    rc = h.lafs_knn_vote(_p(d_s), _p(d_i), Q, k, _p(d_l), len(labels), (C.c_int32 * len(ks))(*ks), len(ks), C.c_float(T), _p(pred), _p(vote),
                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, pred.cpu().numpy(), vote.cpu().numpy()


def check_vote(ts, ti, labels, ks, T):
    """-> (cases, undecided cases, worst vote error / bound)."""
    rc, pred, vote = raw_vote(ts, ti, labels, ks, T)
    assert rc == 0, _lib.lib().lafs_last_error()
    ref = KO.vote(ts, ti, labels, ks, float(np.float32(T)))
    undecided, worst = 0, 0.0
    for n, kn in enumerate(ks):
        g = (kn + 32) * 2.0 ** -23
        for q in range(ts.shape[0]):
            o = ref[n][q]
            m = min(5, len(o))
            assert np.all(pred[n, q, m:] == -1) and np.all(vote[n, q, m:] == 0), (n, q, pred[n, q], vote[n, q])
            v64 = dict(o)
            for c, v in zip(pred[n, q, :m], vote[n, q, :m]):
                assert int(c) in v64, (n, q, c)
                e = abs(float(v) - v64[int(c)])
                assert e <= g * v64[int(c)], (n, q, c, v, v64[int(c)])
                worst = max(worst, e / (g * v64[int(c)]))
            first = [v for _, v in o[:6]]
            decided = all(first[i] - first[i + 1] > g * (first[i] + first[i + 1]) or first[i] == first[i + 1] == 0.0
                          for i in range(len(first) - 1))
            if decided:
                assert [int(c) for c in pred[n, q, :m]] == [c for c, _ in o[:m]], (n, q, pred[n, q], o[:6])
            else:
                undecided += 1
    return len(ks) * ts.shape[0], undecided, worst


clustered = KO.clustered


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_vote_on_searched_lists(seed):
    bank, yb, query, yq = clustered(seed, 25, 48, 1000, 70, 1.5)
    ts, ti, _ = check(bank, query, 200)
    cases, undecided, worst = check_vote(ts, ti, yb, (10, 20, 100, 200), 0.07)
    print(f"\nknn vote seed {seed}: {undecided} of {cases} undecided, worst error/bound {worst:.3f}")
    assert undecided <= 0.02 * cases


def test_vote_small_wide():
    bank, yb, query, yq = clustered(0, 7, 384, 333, 5, 4.0)
    ts, ti, _ = check(bank, query, 200)
    cases, undecided, worst = check_vote(ts, ti, yb, (10, 20, 100, 200), 0.07)
    print(f"\nknn vote D=384: {undecided} of {cases} undecided, worst error/bound {worst:.3f}")
    assert undecided <= 0.02 * cases


def test_vote_hand_made_lists():
    labels = np.array([4, 4, 4, 9, 8, 7, 6, 5, 3, 2, 1000000, 4], np.int32)
    nan = np.float32("nan")
    ts = np.array([[0.9, 0.8, 0.7, 0.6, nan, nan, nan, nan],             # one class only, a -1 tail
                   [0.9, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5],             # more than 5 classes, equal votes: smaller label first
                   [0.1, 0.9, 0.2, 0.3, 0.1, 0.2, 0.3, 0.4],
                   [nan] * 8], np.float32)                               # nothing retrieved
    ti = np.array([[0, 1, 2, 11, -1, -1, -1, -1], [3, 4, 5, 6, 7, 8, 9, 10], [10, 0, 3, 3, 1, 2, 9, 30], [-1] * 8], np.int32)
    ks = (1, 4, 8)
    cases, undecided, _ = check_vote(ts, ti, labels, ks, 0.07)
    rc, pred, vote = raw_vote(ts, ti, labels, ks, 0.07)
    assert list(pred[2, 0]) == [4, -1, -1, -1, -1] and list(pred[2, 3]) == [-1] * 5 and np.all(vote[2, 3] == 0)
    assert list(pred[2, 1]) == [9, 2, 3, 5, 6]                            # 0.9 first, then the equal 0.5 votes by smaller label
    assert list(pred[0, 2]) == [1000000, -1, -1, -1, -1]
    assert 30 >= len(labels) and 4 in pred[2, 2]                          # position 30 >= n_label is skipped
    for bad in ((4, 2), (0,), (9,), (2, 2)):
        rc, pred, vote = raw_vote(ts, ti, labels, bad, 0.07)
        assert rc < 0 and np.all(pred == -9) and np.all(vote == -9.0), bad
