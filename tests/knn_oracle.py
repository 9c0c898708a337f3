"""Host oracle of the weighted k-NN evaluation (csrc/knn.hip, lafs_cvpr2024_amd/knn.py); numpy only, no GPU code.

  scores / bound   float64 dot products, and the derivable bound (D + 2) 2^-24 sum_d |a_d b_d| on any float32 evaluation of them
  rank             the ranking order as a Python sort: larger score first, equal scores by position, NaN last (by position)
  search           the first k positions of that order per query (tail: idx -1, score NaN), with exclude and bank_pos0
  vote             DINO's knn_classifier formula in float64 on a given list: all classes in (larger vote, smaller label) order
  accuracies       top-1 / top-5 in percent from the votes
  holdout_split    the bank / query split of knn.holdout_split, restated independently
  clustered        the seeded clustered rows the vote and accuracy tests share
"""
import math

import numpy as np


def scores(bank, query):
    return np.asarray(query, np.float64) @ np.asarray(bank, np.float64).T


def bound(bank, query):
    D = np.asarray(bank).shape[1]
    return (D + 2) * 2.0 ** -24 * (np.abs(np.asarray(query, np.float64)) @ np.abs(np.asarray(bank, np.float64)).T)


def before(a, ia, b, ib):
    if a != a or b != b:
        return (b != b and ia < ib) if a != a else True
    return a > b or (a == b and ia < ib)


def rank(row_scores, positions):
    """Positions in ranking order."""
    key = lambda t: (1, 0.0, t[1]) if t[0] != t[0] else (0, -t[0], t[1])
    return [p for _, p in sorted(zip((float(s) for s in row_scores), (int(p) for p in positions)), key=key)]


def search(bank, query, k, bank_pos0=0, exclude=None):
    """-> (top_idx int64 [Q, k] positions, -1 tail; S float64 [Q, N] all scores by bank row)."""
    S = scores(bank, query)
    Q, N = S.shape
    top = np.full((Q, k), -1, dtype=np.int64)
    for i in range(Q):
        rows = [j for j in range(N) if exclude is None or bank_pos0 + j != int(exclude[i])]
        order = rank(S[i, rows], [bank_pos0 + j for j in rows])[:k]
        top[i, :len(order)] = order
    return top, S


def vote(top_score, top_idx, bank_label, ks, temperature):
    """-> out[n][q] = [(label, vote64), ...] every class among the first ks[n] entries, larger vote first, then smaller label."""
    out = []
    for kn in ks:
        per_q = []
        for s_row, i_row in zip(np.asarray(top_score), np.asarray(top_idx)):
            acc = {}
            for s, idx in zip(s_row[:kn], i_row[:kn]):
                if 0 <= idx < len(bank_label):
                    c = int(bank_label[idx])
                    acc[c] = acc.get(c, 0.0) + math.exp(float(s) / float(temperature))
            per_q.append(sorted(acc.items(), key=lambda t: (-t[1], t[0])))
        out.append(per_q)
    return out


def accuracies(votes, query_label):
    """votes: vote()'s output -> [(top1 %, top5 %)] per ks entry."""
    res = []
    for per_q in votes:
        t1 = sum(1 for v, y in zip(per_q, query_label) if v and v[0][0] == int(y))
        t5 = sum(1 for v, y in zip(per_q, query_label) if int(y) in [c for c, _ in v[:5]])
        res.append((100.0 * t1 / len(per_q), 100.0 * t5 / len(per_q)))
    return res


def holdout_split(labels, n_holdout=1, min_bank=1):
    """Per identity the last n_holdout records (record order) are queries, the rest bank; an identity left with fewer than min_bank
    bank records gives neither.  -> (bank record indices, query record indices), each ascending."""
    by_id = {}
    for i, y in enumerate(labels):
        by_id.setdefault(int(y), []).append(i)
    bank, query = [], []
    for recs in by_id.values():
        n_bank = len(recs) - n_holdout
        if n_bank < min_bank or n_bank < 0:
            continue
        bank += recs[:n_bank]
        query += recs[n_bank:]
    return sorted(bank), sorted(query)


def clustered(seed, n_class, D, n_bank, n_query, noise):
    """Rows normalize(center[label] + noise * randn) -> (bank f32, bank labels i32, query f32, query labels i32)."""
    r = np.random.RandomState(seed)
    centers = r.randn(n_class, D)
    yb, yq = r.randint(0, n_class, n_bank), r.randint(0, n_class, n_query)
    mk = lambda y: centers[y] + noise * r.randn(len(y), D)
    nrm = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return nrm(mk(yb)), yb.astype(np.int32), nrm(mk(yq)), yq.astype(np.int32)
