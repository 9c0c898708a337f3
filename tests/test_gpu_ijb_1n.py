"""GPU tests of the IJB 1:N search (lafs_ijb_search, csrc/ijb.hip) and the identification protocol on it
(lafs_cvpr2024_amd/ijb_evaluation.py) against the oracle of tests/ijb_1n_oracle.py: scores in numpy.longdouble, the ranking order as
a Python sort.

Per-element bound (fixed, derivable): any order of D float64 products and D - 1 additions, fused or not, differs from the exact value
by at most (D + 2) 2^-53 sum_d |a_d b_d|.  Every score the device returns is held to it against the oracle's score of the pair the
device names.  Selection is checked in a way that near-ties cannot fail, and exactly where the oracle's scores of a row lie more than
twice the bound apart (asserted for every row that is used so).

The design has no gallery split and needs no workspace (lafs_ijb_search_workspace returns 0), so there is no split-gallery merge and
no short workspace to refuse; G = 5000 with Q = 3 runs the one path there is.  Its boundaries: 16 gallery positions per MFMA block,
64 per tile; 16 probes per wave, 64 per workgroup; 32 columns of D per LDS chunk."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ijb_1n_oracle as NO  # noqa: E402
import ijb_oracle as IO  # noqa: E402
import make_synthetic_ijb as syn  # noqa: E402
from lafs_cvpr2024_amd import _lib  # noqa: E402
from lafs_cvpr2024_amd import ijb_evaluation as J  # noqa: E402
from lafs_cvpr2024_amd.ops import _p, call  # noqa: E402

DEV = "cuda"
GUARD, SENTINEL = 4, 1.0e300
WORST = {"ratio": 0.0}


def table(seed, T, D, unit=True):
    """Seeded Gaussian rows; unit rows where D allows distinct scores (D = 1 unit rows are all +-1)."""
    x = np.random.RandomState(seed).randn(T, D)
    return x / np.linalg.norm(x, axis=1, keepdims=True) if unit and D > 4 else x


def device_search(unit, probe, gallery, mate, k):
    """The table sits between guard rows of a sentinel that would wreck any score it entered."""
    T, D = unit.shape
    big = torch.full((T + 2 * GUARD, D), SENTINEL, device=DEV, dtype=torch.float64)
    big[GUARD:GUARD + T] = torch.from_numpy(unit)
    out = J.search(big[GUARD:GUARD + T], np.asarray(probe, np.int32), np.asarray(gallery, np.int32), np.asarray(mate, np.int32), k)
    torch.cuda.synchronize()
    g = big.cpu().numpy()
    assert np.all(g[:GUARD] == SENTINEL) and np.all(g[GUARD + T:] == SENTINEL)
    return out


def before(a, ia, b, ib):
    if a != a or b != b:
        return (b != b and ia < ib) if a != a else True
    return a > b or (a == b and ia < ib)


def check(unit, probe, gallery, mate, k, exact):
    """Everything the header promises about one search.  exact: the oracle's scores of every row lie more than twice the bound apart
    (asserted), so indices and ranks must equal the oracle's."""
    probe, gallery, mate = np.asarray(probe), np.asarray(gallery), np.asarray(mate)
    T, G, Q = unit.shape[0], len(gallery), len(probe)
    o = NO.search(unit, probe, gallery, mate, k)
    d = device_search(unit, probe, gallery, mate, k)
    S, B = o["scores"], o["bound"]
    if exact:
        ok = (probe >= 0) & (probe < T)
        assert NO.min_gap_ratio(S[ok], B[ok]) > 2.0
    assert d["top_score"].shape == (Q, k) and d["top_idx"].shape == (Q, k) and d["top_idx"].dtype == np.int32
    worst = 0.0

    def err(dev, i, j):                                  # |device score - oracle score of pair (i, j)| / bound, NaN <-> NaN
        nonlocal worst
        if S[i, j] != S[i, j] or dev != dev:
            assert S[i, j] != S[i, j] and dev != dev, (i, j, dev, S[i, j])
            return
        e = abs(float(np.longdouble(dev) - S[i, j]))
        assert e <= B[i, j], (i, j, dev, S[i, j], e, B[i, j])
        if B[i, j] > 0:
            worst = max(worst, e / B[i, j])

    for i in range(Q):
        ts, ti, m = d["top_score"][i], d["top_idx"][i], int(mate[i])
        if not 0 <= probe[i] < T:
            assert np.all(ti == -1) and np.isnan(ts).all() and np.isnan(d["mate_score"][i]) and d["mate_rank"][i] == -1
            assert np.isnan(d["best_nonmate"][i])
            continue
        n = min(k, G)
        assert np.all(ti[n:] == -1) and np.isnan(ts[n:]).all()
        assert np.all((ti[:n] >= 0) & (ti[:n] < G)) and len(set(ti[:n].tolist())) == n
        for r in range(n):
            err(ts[r], i, ti[r])
            assert r == 0 or before(ts[r - 1], ti[r - 1], ts[r], ti[r]), (i, r, ts[:n], ti[:n])
        out = np.setdiff1d(np.arange(G), ti[:n])
        if len(out) and ts[n - 1] == ts[n - 1]:          # nothing left out beats the k-th score by more than twice the bound
            with np.errstate(invalid="ignore"):
                over = (S[i, out] - np.longdouble(ts[n - 1])).astype(np.float64) > 2 * np.maximum(B[i, out], B[i, ti[n - 1]])
            assert not over.any(), (i, out[over])
        elif len(out):                                   # the k-th is a NaN: only later NaNs may be left out
            assert np.isnan(S[i, out].astype(np.float64)).all() and out.min() > ti[n - 1]
        # the mate
        if m < 0:
            assert np.isnan(d["mate_score"][i]) and d["mate_rank"][i] == -1
        else:
            err(d["mate_score"][i], i, m)
            others = np.arange(G) != m
            sm, bm = S[i, m], B[i, m]
            with np.errstate(invalid="ignore"):
                gap = (S[i] - sm).astype(np.float64)
                sure = others & (gap > 2 * np.maximum(B[i], bm))
                maybe = others & (gap >= -2 * np.maximum(B[i], bm))
            if sm != sm:                                 # a NaN mate: every number precedes it, and the NaNs in front of it
                nan_s = np.isnan(S[i].astype(np.float64))
                assert d["mate_rank"][i] == int((~nan_s).sum() + (nan_s[:m]).sum())
            else:
                assert int(sure.sum()) <= d["mate_rank"][i] <= int(maybe.sum()), (i, d["mate_rank"][i], sure.sum(), maybe.sum())
        # the best non-mate: the score of some position other than the mate, and none of them beats it beyond the bound
        bn = d["best_nonmate"][i]
        rest = np.flatnonzero(np.arange(G) != m)
        if len(rest) == 0:
            assert bn != bn
        elif bn != bn:
            assert np.isnan(S[i, rest].astype(np.float64)).all()
        else:
            with np.errstate(invalid="ignore"):
                diff = (S[i, rest] - np.longdouble(bn)).astype(np.float64)
            j = rest[int(np.nanargmin(np.abs(diff)))]
            err(bn, i, j)
            assert not (diff > 2 * np.maximum(B[i, rest], B[i, j])).any()
            if exact:
                assert j == o["nonmate_pos"][i]
        if exact:
            assert np.array_equal(ti, o["top_idx"][i]), (i, ti, o["top_idx"][i])
            assert d["mate_rank"][i] == o["mate_rank"][i]
    WORST["ratio"] = max(WORST["ratio"], worst)
    print(f"[1:N] Q {Q} G {G} D {unit.shape[1]} k {k}: worst error / bound {worst:.3f}")
    return d, o


def cycle_mates(Q, G):
    return np.array([[0, G - 1, -1][i % 3] for i in range(Q)], dtype=np.int32)


# ----------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("D", [1, 5, 7, 384, 768, 1024])
def test_every_shape_against_the_oracle(D):
    """Q in {1, 17, 65} x G in {1, 15, 17, 33, 257}, k in {1, 5, 10, 64} in turn (k > G gives the -1 / NaN tail), mates at position 0,
    at G - 1 and absent, unsorted index lists without repeats: indices and ranks equal the oracle's exactly."""
    unit = table(100 + D, 330, D)
    rng = np.random.RandomState(D)
    ks, n = [1, 5, 10, 64], 0
    for Q in (1, 17, 65):
        for G in (1, 15, 17, 33, 257):
            rows = rng.permutation(330)
            check(unit, rows[:Q], rows[Q:Q + G], cycle_mates(Q, G), ks[n % 4], exact=True)
            n += 1
    check(unit, rows[:17], rows[17:17 + 33], cycle_mates(17, 33), 64, exact=True)          # k > G at a G past one MFMA block
    print(f"[1:N] D {D}: worst error / bound so far {WORST['ratio']:.3f}")


def test_large_gallery_few_probes():
    """G = 5000 (79 tiles) with Q = 3: the shape a split-gallery design would treat apart; here the one path."""
    unit = table(7, 5003, 384)
    rows = np.random.RandomState(8).permutation(5003)
    check(unit, rows[:3], rows[3:], [0, 4999, -1], 10, exact=True)


def test_ascending_and_descending_feeds_best_match_first_and_last():
    """Gallery row j = a_j v with a_j rising: a probe with p.v > 0 sees rising scores (the best match in the LAST position, every
    position displaces the list's head), one with p.v < 0 falling scores (the best in the FIRST position)."""
    D, G = 7, 257
    rng = np.random.RandomState(3)
    v = rng.randn(D)
    gal = np.outer(1.0 + np.arange(G) / 64.0, v)
    pr = rng.randn(17, D)
    assert (pr @ v > 0).any() and (pr @ v < 0).any()
    unit = np.concatenate([gal, pr])
    for k in (1, 10, 64):
        d, _ = check(unit, G + np.arange(17), np.arange(G), cycle_mates(17, G), k, exact=True)
        up = pr @ v > 0
        assert np.all(d["top_idx"][up, 0] == G - 1) and np.all(d["top_idx"][~up, 0] == 0)
        assert np.array_equal(d["top_idx"][up][0], np.arange(G - 1, G - 1 - k, -1)) and np.array_equal(d["top_idx"][~up][0], np.arange(k))


def test_repeated_and_unsorted_index_lists():
    unit = table(11, 40, 384)
    rng = np.random.RandomState(12)
    probe, gallery = rng.randint(0, 40, 65), rng.randint(0, 40, 257)                       # rows repeat: ties by position
    d, o = check(unit, probe, gallery, cycle_mates(65, 257), 64, exact=False)
    assert np.array_equal(d["top_idx"], o["top_idx"]) and np.array_equal(d["mate_rank"], o["mate_rank"])


# ----------------------------------------------------------------------------------------------------------------- ties
def test_exact_ties_across_every_boundary():
    """One row sits at gallery positions on both sides of every MFMA-block (16) and tile (64) boundary and at both ends; the probes are
    that row plus noise, so the copies lead every list.  Scores bit-equal, order by position, mate_rank counts the earlier copies only.
    Probes 15 | 16 (waves) and 63 | 64 (workgroups) are bit-identical rows and must give identical bits."""
    D, G, Q, k = 768, 257, 65, 64
    rng = np.random.RandomState(21)
    unit = table(20, 400, D)
    dup = [0, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 127, 128, 191, 192, 255, 256]
    gallery = rng.permutation(399)[:G] + 1
    gallery[dup] = 0
    pr = unit[0] + 0.02 * rng.randn(Q, D)
    pr[16], pr[64] = pr[15], pr[63]
    unit = np.concatenate([unit, pr])
    probe = 400 + np.arange(Q)
    mate = np.array([dup[i % len(dup)] for i in range(Q)], dtype=np.int32)
    mate[16], mate[64] = mate[15], mate[63]
    d, o = check(unit, probe, gallery, mate, k, exact=False)
    nd = len(dup)
    for i in range(Q):
        assert d["top_idx"][i, :nd].tolist() == dup, i
        bits = d["top_score"][i, :nd].view(np.int64)
        assert np.all(bits == bits[0])
        assert d["mate_score"][i].view(np.int64) == bits[0]
        assert d["mate_rank"][i] == dup.index(mate[i])                                     # the earlier copies, not the later ones
        assert d["best_nonmate"][i].view(np.int64) == bits[0]
    assert np.array_equal(d["top_idx"], o["top_idx"]) and np.array_equal(d["mate_rank"], o["mate_rank"])
    for a, b in ((15, 16), (63, 64)):
        assert np.array_equal(d["top_score"][a].view(np.int64), d["top_score"][b].view(np.int64))
        assert np.array_equal(d["top_idx"][a], d["top_idx"][b]) and d["mate_rank"][a] == d["mate_rank"][b]


def test_scores_do_not_depend_on_position_or_launch_geometry():
    D, G, Q, k = 768, 257, 65, 64
    unit = table(30, 330, D)
    rng = np.random.RandomState(31)
    rows = rng.permutation(330)
    probe, gallery, mate = rows[:Q], rows[Q:Q + G], rng.randint(0, G, Q).astype(np.int32)
    a, _ = check(unit, probe, gallery, mate, k, exact=True)
    pp, pg = rng.permutation(Q), rng.permutation(G)
    inv_g = np.argsort(pg)                                                                 # old gallery position -> new position
    b = device_search(unit, probe[pp], gallery[pg], inv_g[mate[pp]], k)
    for name in ("top_score", "mate_score", "best_nonmate"):
        assert np.array_equal(a[name][pp].view(np.int64), b[name].view(np.int64)), name
    assert np.array_equal(a["top_idx"][pp], pg[b["top_idx"]]) and np.array_equal(a["mate_rank"][pp], b["mate_rank"])
    for i in (0, 16, 64):                                                                  # one probe alone, a shorter gallery
        c = device_search(unit, probe[i:i + 1], gallery, mate[i:i + 1], k)
        assert np.array_equal(c["top_score"].view(np.int64), a["top_score"][i:i + 1].view(np.int64))
        assert c["mate_score"].view(np.int64) == a["mate_score"][i].view(np.int64) and c["mate_rank"] == a["mate_rank"][i]
    m = int(mate[5])
    c = device_search(unit, probe[5:6], gallery[m:m + 1], [0], 1)                          # the mate pair alone
    assert c["top_score"][0, 0].view(np.int64) == a["mate_score"][5].view(np.int64) == c["mate_score"][0].view(np.int64)


# ----------------------------------------------------------------------------------------------------------------- NaN, bad input
def test_nan_rows_rank_last_and_a_nan_probe_orders_by_position():
    D, G = 384, 33
    unit = table(40, 80, D)
    unit[70, 5] = np.nan                                                                   # a gallery row
    unit[71, :] = np.nan                                                                   # a probe row
    gallery = np.arange(G)
    gallery[[0, 16, 32]] = 70
    probe = np.array([40, 71, 41, 42])
    mate = np.array([16, 20, 5, -1], dtype=np.int32)
    d, o = check(unit, probe, gallery, mate, 64, exact=False)
    for i in (0, 2, 3):
        assert d["top_idx"][i, G - 3:G].tolist() == [0, 16, 32] and np.isnan(d["top_score"][i, G - 3:G]).all()
        assert not np.isnan(d["top_score"][i, :G - 3]).any() and not np.isnan(d["best_nonmate"][i])
    assert d["mate_rank"][0] == G - 3 + 1 and np.isnan(d["mate_score"][0])                 # 30 numbers and the NaN at position 0
    assert d["top_idx"][1, :G].tolist() == list(range(G)) and np.isnan(d["top_score"][1, :G]).all()
    assert d["mate_rank"][1] == 20 and np.isnan(d["best_nonmate"][1])
    assert np.array_equal(d["top_idx"], o["top_idx"]) and np.array_equal(d["mate_rank"], o["mate_rank"])
    # a gallery of NaN rows only, and the mate the only row: nothing is left for best_nonmate
    d, _ = check(unit, [40, 41], [70], [0, -1], 5, exact=False)
    assert np.isnan(d["best_nonmate"][0]) and np.isnan(d["best_nonmate"][1]) and d["mate_rank"][0] == 0
    assert d["top_idx"].tolist() == [[0, -1, -1, -1, -1]] * 2


def test_out_of_range_indices_never_leave_the_table():
    D, T = 768, 50
    unit = table(50, T, D)
    probe = np.array([3, -1, T, 7, T + 2, -GUARD, 2 ** 31 - 1], dtype=np.int64)
    gallery = np.r_[np.arange(10, 27), [-1, T, T + 1, -2, 2 ** 31 - 1, -2 ** 31]]
    mate = np.array([17, 0, 3, 18, -1, 2, 1], dtype=np.int32)                              # 17, 18: gallery entries outside the table
    d, o = check(unit, probe, gallery, mate, 64, exact=False)
    assert np.array_equal(d["top_idx"], o["top_idx"]) and np.array_equal(d["mate_rank"], o["mate_rank"])
    assert d["mate_rank"][0] == 17 and d["mate_rank"][3] == 18 and np.isnan(d["mate_score"][0])
    assert d["top_idx"][0, 17:23].tolist() == [17, 18, 19, 20, 21, 22] and np.abs(d["top_score"][0, :17]).max() <= 1.0 + 1e-12


def test_mate_outside_the_gallery_is_no_mate_on_the_device_and_an_error_in_python():
    unit = table(60, 20, 5)
    t = torch.from_numpy(unit).to(DEV)
    with pytest.raises(ValueError):
        J.search(t, [0, 1], [2, 3, 4], [3, 0])
    with pytest.raises(ValueError):
        J.search(t, [0, 1], [2, 3, 4], [-2, 0])
    with pytest.raises(ValueError):
        J.search(t, [0, 1], [2, 3, 4], [0, 0], k=65)
    with pytest.raises(ValueError):
        J.search(t, [0, 1], [2, 3, 4], [0, 0], k=0)
    Q, G, k = 2, 3, 2
    ins = [torch.tensor(a, dtype=torch.int32, device=DEV) for a in ([0, 1], [2, 3, 4], [3, -7])]
    ts, ti = torch.zeros(Q, k, device=DEV, dtype=torch.float64), torch.zeros(Q, k, device=DEV, dtype=torch.int32)
    ms, mr, bn = torch.zeros(Q, device=DEV, dtype=torch.float64), torch.zeros(Q, device=DEV, dtype=torch.int32), torch.zeros(Q, device=DEV, dtype=torch.float64)
    call("lafs_ijb_search", _p(t), 20, 5, _p(ins[0]), Q, _p(ins[1]), G, _p(ins[2]), k, _p(ts), _p(ti), _p(ms), _p(mr), _p(bn), None, 0)
    torch.cuda.synchronize()
    assert mr.tolist() == [-1, -1] and torch.isnan(ms).all() and not torch.isnan(bn).any()
    assert torch.equal(bn, ts[:, 0])


def test_bad_arguments_are_refused_with_a_message():
    h = _lib.lib()
    assert h.lafs_ijb_search_workspace(19593, 1772, 10) == 0                               # the design needs none: none can be short
    unit = torch.zeros(4, 8, device=DEV, dtype=torch.float64)
    i32 = torch.zeros(4, device=DEV, dtype=torch.int32)
    f64 = torch.zeros(4 * 64, device=DEV, dtype=torch.float64)
    good = dict(unit=_p(unit), T=4, D=8, probe=_p(i32), Q=4, gallery=_p(i32), G=4, mate=_p(i32), k=4, ts=_p(f64), ti=_p(torch.zeros(256, device=DEV, dtype=torch.int32)),
                ms=_p(f64), mr=_p(i32), bn=_p(f64), ws=None, wsb=0)

    def rc(**kw):
        a = dict(good, **kw)
        return h.lafs_ijb_search(*[a[n] for n in ("unit", "T", "D", "probe", "Q", "gallery", "G", "mate", "k", "ts", "ti", "ms", "mr", "bn", "ws", "wsb")],
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert rc() == 0
    for bad in (dict(k=0), dict(k=65), dict(D=1025), dict(D=0), dict(Q=0), dict(G=0), dict(T=0), dict(unit=None), dict(probe=None), dict(gallery=None),
                dict(mate=None), dict(ts=None), dict(ti=None), dict(ms=None), dict(mr=None), dict(bn=None)):
        assert rc(**bad) < 0 and h.lafs_last_error(), bad
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- 1:1, protocol
def test_search_scores_agree_with_the_pair_kernel():
    D, Q, G, k = 768, 65, 257, 64
    unit = table(70, 330, D)
    rows = np.random.RandomState(71).permutation(330)
    probe, gallery = rows[:Q], rows[Q:Q + G]
    d, o = check(unit, probe, gallery, cycle_mates(Q, G), k, exact=True)
    i1 = np.repeat(probe, k).astype(np.int32)
    i2 = gallery[d["top_idx"].reshape(-1)].astype(np.int32)
    t, a, b = (torch.from_numpy(x).to(DEV) for x in (unit, i1, i2))
    out = torch.empty(len(i1), device=DEV, dtype=torch.float64)
    call("lafs_ijb_pair_scores", _p(t), 330, D, _p(a), _p(b), len(i1), _p(out))
    torch.cuda.synchronize()
    bound = np.take_along_axis(o["bound"], d["top_idx"].astype(np.int64), 1).reshape(-1)
    diff = np.abs(out.cpu().numpy() - d["top_score"].reshape(-1))
    print(f"[1:N] search against the pair kernel: worst |difference| / bound {float((diff / bound).max()):.3f}")
    assert np.all(diff <= 2 * bound)


def _protocol_case():
    feats, faceness, templates, medias, p1, p2, _ = syn.protocol_inputs(22, 96, 384, 32, 9.0)
    tids = np.random.RandomState(22).choice(100000, 96, replace=False)                     # protocol_inputs' own first draw
    assert set(tids.tolist()) == set(np.unique(templates).tolist())
    sid = 500 + 3 * (np.arange(96) % 32)                                                   # template j shows identity j % 32
    lists = dict(g1_tids=tids[0:12], g1_sids=sid[0:12], g2_tids=tids[12:24], g2_sids=sid[12:24], probe_tids=tids[32:96][::-1],
                 probe_sids=sid[32:96][::-1])                                              # identities 24 .. 31 are in neither gallery
    return feats, dict(faceness=faceness, templates=templates, medias=medias), lists


def test_identification_protocol_equals_the_oracle():
    feats, meta, lists = _protocol_case()
    res = J.evaluate_identification(feats, meta, lists, k=10, device=DEV)
    sums, uq = IO.template_sums(feats, meta["faceness"], meta["templates"], meta["medias"])
    unit = IO.unit_rows(sums)
    pr = J.template_rows(uq, lists["probe_tids"])
    cm, tp = [], []
    for g, key in (("G1", "g1"), ("G2", "g2")):
        gr, mate = J.template_rows(uq, lists[key + "_tids"]), NO.mates(lists[key + "_sids"], lists["probe_sids"])
        o = NO.search(unit, pr, gr, mate, 10)
        d = res["searches"][g]
        assert np.array_equal(d["mate"], mate) and (mate >= 0).sum() == 24 and (mate < 0).sum() == 40
        # no decision lies within twice the bound (plus the 1e-13 the device's unit rows may differ by) of a competing score or of tau
        tol = 2 * o["bound"].max() + 4e-13
        assert NO.min_gap_ratio(o["scores"], np.full_like(o["bound"], tol / 2)) > 2.0
        om = NO.gallery_metrics(o, mate)
        pool = np.sort(np.r_[o["mate_score"][mate >= 0], o["top_score"][mate < 0, 0]].astype(np.float64))
        assert np.diff(pool).min() > tol
        assert np.array_equal(d["top_idx"], o["top_idx"]) and np.array_equal(d["mate_rank"], o["mate_rank"])
        assert np.abs(d["top_score"] - o["top_score"].astype(np.float64)).max() <= tol
        assert res[g]["cmc"].tolist() == om["cmc"] and res[g]["tpir"].tolist() == om["tpir"]
        assert np.abs(res[g]["tau"] - np.array(om["tau"])).max() <= tol
        cm.append(om["cmc"]); tp.append(om["tpir"])
    assert res["mean"]["cmc"].tolist() == ((np.array(cm[0]) + np.array(cm[1])) / 2).tolist()
    assert res["mean"]["tpir"].tolist() == ((np.array(tp[0]) + np.array(tp[1])) / 2).tolist()
    assert 0 <= res["mean"]["cmc"][0] <= res["mean"]["cmc"][2] <= 1
    print(f"[1:N] protocol: cmc {res['mean']['cmc']}, tpir {res['mean']['tpir']}")


def test_identify_rejects_bad_lists():
    feats, meta, lists = _protocol_case()
    a = (feats, meta["faceness"], meta["templates"], meta["medias"])
    with pytest.raises(ValueError):                                                        # a template id without images
        J.identify(*a, np.r_[lists["g1_tids"], [100001]], np.r_[lists["g1_sids"], [7]], lists["probe_tids"], lists["probe_sids"], device=DEV)
    with pytest.raises(ValueError):                                                        # two gallery templates of one subject
        J.identify(*a, lists["g1_tids"], np.r_[lists["g1_sids"][:-1], lists["g1_sids"][:1]], lists["probe_tids"], lists["probe_sids"], device=DEV)
    with pytest.raises(ValueError):
        J.evaluate_identification(feats, meta, lists, k=5, device=DEV)                     # rank-10 needs k >= 10


# ----------------------------------------------------------------------------------------------------------------- end to end
def test_module_entry_point_1n_on_the_synthetic_tree(tmp_path):
    tree, res = tmp_path / "ijb", tmp_path / "res"
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_ijb.py"), str(tree), "24"], check=True, env=env, timeout=120)
    from lafs_cvpr2024_amd import train_largescale as tl
    arch = ["--num_class", "32"]
    torch.manual_seed(7)
    backbone = tl.build_backbone(tl.get_args_parser().parse_args(arch))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"module." + k: v for k, v in backbone.state_dict().items()}, ckpt)
    del backbone
    feats = tmp_path / "feats.npz"

    def run(job, *extra):
        p = subprocess.run([sys.executable, "-m", "lafs_cvpr2024_amd.ijb_evaluation", "--image_path", str(tree), "--target", "IJBC",
                            "--result_dir", str(res), "--job", job] + list(extra), capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        return [l for l in p.stdout.splitlines() if "|" in l]

    lines = run("first", "--protocol", "1N", "--checkpoint", str(ckpt), "--batch_size", "10", "--save_features", str(feats), *arch)
    assert len(lines) == 2
    assert [c.strip() for c in lines[0].split("|")] == ["Methods", "rank-1", "rank-5", "rank-10", "TPIR@FPIR=0.01", "TPIR@FPIR=0.1"]
    z = dict(np.load(res / "first" / "ijbc_1N.npz"))
    # the oracle, from the saved features
    with np.load(feats) as f:
        img_feats, faceness = f["img_feats"], f["faceness"]
    ds, ls = syn.dataset(24), syn.identification_lists(24)
    sums, uq = IO.template_sums(img_feats, faceness, ds["tid"], ds["mid"])
    unit = IO.unit_rows(sums)
    pr = J.template_rows(uq, ls["probe_tids"])
    cm, tp = [], []
    for g, key in (("G1", "g1"), ("G2", "g2")):
        mate = NO.mates(ls[key + "_sids"], ls["probe_sids"])
        o = NO.search(unit, pr, J.template_rows(uq, ls[key + "_tids"]), mate, 10)
        tol = 2 * o["bound"].max() + 4e-13
        assert NO.min_gap_ratio(o["scores"], np.full_like(o["bound"], tol / 2)) > 2.0
        pool = np.sort(np.r_[o["mate_score"][mate >= 0], o["top_score"][mate < 0, 0]].astype(np.float64))
        assert np.diff(pool).min() > tol
        assert np.array_equal(z[g + "_mate"], mate) and np.array_equal(z[g + "_gallery_tids"], ls[key + "_tids"])
        assert np.array_equal(z[g + "_top_idx"], o["top_idx"]) and np.array_equal(z[g + "_mate_rank"], o["mate_rank"])
        assert z[g + "_top_score"].shape == (9, 10) and np.all(z[g + "_top_idx"][:, 4:] == -1)
        for name in ("top_score", "mate_score", "best_nonmate"):
            a, b = z[g + "_" + name], o[name].astype(np.float64)
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(np.abs(a - b)) <= tol, name
        m = NO.gallery_metrics(o, mate)
        cm.append(m["cmc"]); tp.append(m["tpir"])
    assert np.array_equal(z["probe_tids"], ls["probe_tids"])
    mean = list((np.array(cm[0]) + np.array(cm[1])) / 2) + list((np.array(tp[0]) + np.array(tp[1])) / 2)
    assert [c.strip() for c in lines[1].split("|")] == ["ijbc-IJBC"] + ["%.2f" % (100 * v) for v in mean]
    # the protocol alone from the saved features: the same file bit for bit
    again = run("again", "--protocol", "1N", "--features", str(feats))
    assert again == lines
    z2 = dict(np.load(res / "again" / "ijbc_1N.npz"))
    assert sorted(z2) == sorted(z) and all(z[n].tobytes() == z2[n].tobytes() and z[n].dtype == z2[n].dtype for n in z)
    # 1:1 on the same tree: the default and --protocol 11 are one and the same, and what the 1:1 oracle computes
    one = run("one", "--features", str(feats))
    two = run("two", "--features", str(feats), "--protocol", "11")
    assert one == two and len(one) == 2 and one[0].split("|")[1].strip() == "1e-06"
    s1, s2 = np.load(res / "one" / "ijbc.npy"), np.load(res / "two" / "ijbc.npy")
    assert s1.tobytes() == s2.tobytes() and sorted(os.listdir(res / "one")) == ["ijbc.npy"]
    o_scores, _, _ = IO.protocol(img_feats, faceness, ds["tid"], ds["mid"], ds["p1"], ds["p2"])
    assert np.abs(s1 - o_scores).max() <= 1e-12
    assert [c.strip() for c in one[1].split("|")][1:] == J.tar_at_far(*J.roc_points(ds["label"], s1))[2]
