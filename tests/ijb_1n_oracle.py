"""Oracle of the IJB 1:N search and its metrics (lafs_ijb_search, lafs_cvpr2024_amd/ijb_evaluation.py), independent of the product:
scores in numpy.longdouble (or exactly, with fractions), the ranking order as a plain Python sort, the metrics as plain loops."""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53


def score_matrix(unit, probe_idx, gallery_idx):
    """-> (scores longdouble [Q, G], bound float64 [Q, G]).  bound = (D + 2) 2^-53 sum_d |a_d b_d|: what any order of D float64
    products and D - 1 float64 additions, fused or not, can differ from the exact value by.  A gallery index outside the table
    scores NaN; a probe index outside it makes its whole row NaN (the caller treats such a probe apart)."""
    unit = np.asarray(unit, dtype=np.float64)
    T, D = unit.shape
    pi, gi = np.asarray(probe_idx), np.asarray(gallery_idx)
    pok, gok = (pi >= 0) & (pi < T), (gi >= 0) & (gi < T)
    P = unit[np.where(pok, pi, 0)].astype(LD)
    Gm = unit[np.where(gok, gi, 0)].astype(LD)
    with np.errstate(invalid="ignore", over="ignore"):
        s = P @ Gm.T
        b = (np.abs(P) @ np.abs(Gm).T).astype(np.float64) * ((D + 2) * EPS)
    s[:, ~gok] = np.nan
    s[~pok, :] = np.nan
    return s, b


def exact_score(a, b):
    """The dot product of two float64 rows as a Fraction."""
    return sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)), Fraction(0))


def ranking(row):
    """Gallery positions in ranking order: larger score first, equal scores by position, NaN after every number (by position)."""
    def key(j):
        s = row[j]
        return (1, 0, j) if s != s else (0, -s, j)
    return sorted(range(len(row)), key=key)


def search(unit, probe_idx, gallery_idx, mate, k):
    """The outputs of lafs_ijb_search from the oracle's scores, plus nonmate_pos [Q] (the position behind best_nonmate, -1: none),
    plus the score matrix and its bound."""
    s, bound = score_matrix(unit, probe_idx, gallery_idx)
    T = np.asarray(unit).shape[0]
    Q, G = s.shape
    top_score = np.full((Q, k), np.nan, dtype=LD)
    top_idx = np.full((Q, k), -1, dtype=np.int32)
    mate_score = np.full(Q, np.nan, dtype=LD)
    mate_rank = np.full(Q, -1, dtype=np.int32)
    best_nonmate = np.full(Q, np.nan, dtype=LD)
    nonmate_pos = np.full(Q, -1, dtype=np.int32)
    for i in range(Q):
        if not 0 <= probe_idx[i] < T:
            continue
        order = ranking(s[i])
        m = int(mate[i]) if 0 <= mate[i] < G else -1
        for r, j in enumerate(order[:k]):
            top_score[i, r], top_idx[i, r] = s[i, j], j
        if m >= 0:
            mate_score[i], mate_rank[i] = s[i, m], order.index(m)
        rest = [j for j in order if j != m]
        if rest:
            best_nonmate[i], nonmate_pos[i] = s[i, rest[0]], rest[0]
    return dict(top_score=top_score, top_idx=top_idx, mate_score=mate_score, mate_rank=mate_rank, best_nonmate=best_nonmate,
                nonmate_pos=nonmate_pos, scores=s, bound=bound)


def min_gap_ratio(s, bound):
    """min over the rows of (smallest difference between two scores of the row) / (the larger of their two bounds): > 2 means no two
    scores of a row can change places within the bound."""
    worst = np.inf
    for row, b in zip(s, bound):
        if len(row) < 2:
            continue
        o = np.argsort(row, kind="mergesort")
        d = np.diff(row[o]).astype(np.float64)
        worst = min(worst, float(np.min(d / np.maximum(b[o][1:], b[o][:-1]))))
    return worst


# ----------------------------------------------------------------------------------------------------------------- metrics
def cmc(mate_rank, ranks=(1, 5, 10)):
    mated = [int(r) for r in mate_rank if r >= 0]
    if not mated:
        raise ValueError("no mated searches")
    return [sum(1 for r in mated if r < R) / len(mated) for R in ranks]


def tpir_at_fpir(mate_score, mate_rank, nonmated_top, fpirs=(0.01, 0.1), rank=1):
    """-> (tpir per FPIR, tau per FPIR).  tau = the (floor(f |N|) + 1)-th largest non-mated top score, NaN tops counted as -inf, and
    -inf when there are fewer; an alarm is a top score > tau."""
    if len(mate_score) == 0 or len(nonmated_top) == 0:
        raise ValueError("needs mated and non-mated searches")
    tops = sorted((-math.inf if t != t else float(t) for t in nonmated_top), reverse=True)
    out, taus = [], []
    for f in fpirs:
        allowed = math.floor(Fraction(repr(float(f))) * len(tops))
        tau = tops[allowed] if allowed < len(tops) else -math.inf
        assert sum(1 for t in tops if t > tau) <= f * len(tops) + 1e-9
        hits = sum(1 for s, r in zip(mate_score, mate_rank) if r < rank and s == s and s > tau)
        out.append(hits / len(mate_score))
        taus.append(tau)
    return out, taus


def mates(gallery_sids, probe_sids):
    gs = [int(x) for x in gallery_sids]
    if len(set(gs)) != len(gs):
        raise ValueError("a subject with two gallery templates")
    return np.array([gs.index(int(p)) if int(p) in gs else -1 for p in probe_sids], dtype=np.int32)


def gallery_metrics(res, mate, ranks=(1, 5, 10), fpirs=(0.01, 0.1)):
    mated = np.asarray(mate) >= 0
    tp, tau = tpir_at_fpir(res["mate_score"][mated], res["mate_rank"][mated], res["top_score"][~mated, 0], fpirs)
    return dict(cmc=cmc(res["mate_rank"][mated], ranks), tpir=tp, tau=tau)
