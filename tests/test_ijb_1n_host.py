"""CPU checks of the IJB 1:N identification host code (lafs_cvpr2024_amd/ijb_evaluation.py): the csv readers, the mate table, cmc and
tpir_at_fpir on hand-computed cases, the oracle's ranking order (tests/ijb_1n_oracle.py) and the synthetic tree's lists."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ijb_1n_oracle as NO  # noqa: E402
import make_synthetic_ijb as syn  # noqa: E402
from lafs_cvpr2024_amd import ijb_evaluation as J  # noqa: E402

NAN, INF = float("nan"), float("inf")


# ----------------------------------------------------------------------------------------------------------------- readers
def test_csv_reader_is_keyed_on_the_header_and_dedupes(tmp_path):
    f = tmp_path / "g.csv"
    f.write_text("FILENAME,SUBJECT_ID,FACE_X,TEMPLATE_ID\n"
                 "img/1.jpg,70,3.5,12\n"
                 "img/2.jpg,70,1.0,12\n"
                 "frames/9.png,5,0,4000\n"
                 "img/3.jpg,70,2.0,12\n"
                 "img/4.jpg,81,2.0,7\n")
    t, s = J.read_template_subject_csv(str(f))
    assert t.dtype == s.dtype == np.int64
    assert t.tolist() == [12, 4000, 7] and s.tolist() == [70, 5, 81]
    f.write_text("TEMPLATE_ID,SUBJECT_ID\n12,70\n7,81\n")
    t, s = J.read_template_subject_csv(str(f))
    assert t.tolist() == [12, 7] and s.tolist() == [70, 81]


@pytest.mark.parametrize("text", [
    None,                                                        # the file is missing
    "TEMPLATE,SUBJECT_ID\n1,2\n",                                # a missing column
    "TEMPLATE_ID,SUBJECT\n1,2\n",
    "TEMPLATE_ID,SUBJECT_ID\n1,x2\n",                            # not an integer
    "TEMPLATE_ID,SUBJECT_ID\n1.5,2\n",
    "TEMPLATE_ID,SUBJECT_ID,FILENAME\n1\n",                      # a short row
    "TEMPLATE_ID,SUBJECT_ID\n",                                  # an empty list
    "",
    "TEMPLATE_ID,SUBJECT_ID\n1,2\n3,4\n1,5\n",                   # one template, two subjects
])
def test_csv_reader_raises_value_error_with_the_path(tmp_path, text):
    f = tmp_path / "list.csv"
    if text is not None:
        f.write_text(text)
    with pytest.raises(ValueError) as e:
        J.read_template_subject_csv(str(f))
    assert str(f) in str(e.value)


def test_synthetic_tree_lists_read_back(tmp_path):
    syn.make(str(tmp_path), 24, "ijbb")
    lists = J.read_identification_lists(str(tmp_path), "IJBB")
    want = syn.identification_lists(24)
    assert sorted(lists) == sorted(want)
    for key in want:
        assert np.array_equal(lists[key], want[key]), key
    T = syn.TIDS
    assert lists["g1_tids"].tolist() == T[0:4].tolist() and lists["g2_tids"].tolist() == T[4:8].tolist()
    assert lists["probe_tids"].tolist() == T[8:16].tolist() + [T[0]]
    # templates j and j + 8 share their subject; the last probe's subject is in neither gallery
    assert lists["probe_sids"][:4].tolist() == lists["g1_sids"].tolist() and lists["probe_sids"][4:8].tolist() == lists["g2_sids"].tolist()
    assert lists["probe_sids"][8] not in lists["g1_sids"] and lists["probe_sids"][8] not in lists["g2_sids"]
    assert J.mates(lists["g1_sids"], lists["probe_sids"]).tolist() == [0, 1, 2, 3, -1, -1, -1, -1, -1]
    assert J.mates(lists["g2_sids"], lists["probe_sids"]).tolist() == [-1, -1, -1, -1, 0, 1, 2, 3, -1]
    with pytest.raises(ValueError):
        J.read_identification_lists(str(tmp_path), "IJBC")       # written for ijbb
    with pytest.raises(ValueError):
        J.read_identification_lists(str(tmp_path), "LFW")
    os.remove(tmp_path / "meta" / "ijbb_1N_gallery_G2.csv")
    with pytest.raises(ValueError) as e:
        J.read_identification_lists(str(tmp_path), "IJBB")
    assert "ijbb_1N_gallery_G2.csv" in str(e.value)


def test_synthetic_tree_keeps_its_earlier_files_and_data(tmp_path):
    ds = syn.make(str(tmp_path), 24)
    assert sorted(os.listdir(tmp_path / "meta")) == ["ijbc_1N_gallery_G1.csv", "ijbc_1N_gallery_G2.csv", "ijbc_1N_probe_mixed.csv",
                                                      "ijbc_face_tid_mid.txt", "ijbc_name_5pts_score.txt", "ijbc_template_pair_label.txt"]
    meta = J.read_meta(str(tmp_path), "IJBC")
    assert np.array_equal(meta["templates"], ds["tid"]) and np.array_equal(meta["p1"], ds["p1"])


def test_mates_unsorted_subjects_and_a_duplicate():
    assert J.mates([50, 7, 19], [19, 50, 8, 7, 7]).tolist() == [2, 0, -1, 1, 1]
    assert J.mates([50, 7, 19], [19, 50, 8, 7, 7]).dtype == np.int32
    assert np.array_equal(J.mates([50, 7, 19], [19, 50, 8, 7, 7]), NO.mates([50, 7, 19], [19, 50, 8, 7, 7]))
    with pytest.raises(ValueError):
        J.mates([50, 7, 50], [1])
    with pytest.raises(ValueError):
        J.mates([], [1])


# ----------------------------------------------------------------------------------------------------------------- metrics
def test_cmc_by_hand():
    mr = np.array([0, 4, -1, 5, 9, 10, 0, -1])                    # six mated searches
    assert J.cmc(mr).tolist() == [2 / 6, 3 / 6, 5 / 6]
    assert J.cmc(mr, ranks=(11,)).tolist() == [1.0]
    assert J.cmc(mr).tolist() == NO.cmc(mr)
    with pytest.raises(ValueError):
        J.cmc(np.array([-1, -1]))
    with pytest.raises(ValueError):
        J.cmc(np.array([], dtype=np.int32))


def both(ms, mr, nt, fpirs, rank=1):
    a, ta = J.tpir_at_fpir(ms, mr, nt, fpirs, rank)
    b, tb = NO.tpir_at_fpir(ms, mr, nt, fpirs, rank)
    assert a.tolist() == b and ta.tolist() == tb
    return a.tolist(), ta.tolist()


def test_tpir_floor_zero_takes_the_largest_non_mated_top():
    """|N| = 10, f = 0.01: floor(0.1) = 0 alarms allowed, tau = the largest top; only mated scores above it count."""
    nt = [0.1 * i for i in range(10)]                              # largest 0.9
    ms, mr = [0.95, 0.9, 0.5, 0.99], [0, 0, 0, 1]
    tp, tau = both(ms, mr, nt, (0.01,))
    assert tau == [0.9 if 0.1 * 9 == 0.9 else 0.1 * 9] and tp == [1 / 4]          # 0.9 is not > tau; 0.99 has rank 1
    tp, _ = both(ms, mr, nt, (0.01,), rank=2)
    assert tp == [2 / 4]


def test_tpir_ties_at_tau_do_not_alarm():
    """Three tops tie at 0.7 and f |N| = 2: tau = 0.7, so none of the three alarms (realised FPIR 0 <= 0.2), and a mate score
    equal to tau is no hit."""
    nt = [0.7, 0.2, 0.7, 0.1, 0.7, 0.3, 0.0, 0.05, 0.15, 0.25]
    tp, tau = both([0.7, 0.71, 0.69], [0, 0, 0], nt, (0.2,))
    assert tau == [0.7] and tp == [1 / 3]
    assert sum(t > tau[0] for t in nt) == 0


def test_tpir_f_times_n_at_least_n_gives_minus_infinity():
    nt = [0.4, 0.6, 0.5]
    tp, tau = both([-0.9, 0.45, 0.2], [0, 0, 2], nt, (1.0, 0.99, 0.34, 0.33))
    assert tau == [-INF, 0.4, 0.5, 0.6]                            # floor(3 f) = 3, 2, 1, 0
    assert tp == [2 / 3, 1 / 3, 0.0, 0.0]


def test_tpir_reads_f_as_the_decimal_it_prints_as():
    """0.1 * 30 and 0.07 * 100 are not integers in binary floating point; the allowed alarms are 3 and 7 all the same."""
    nt = list(range(30))
    _, tau = both([0.0], [0], nt, (0.1,))
    assert tau == [26.0]
    _, tau = both([0.0], [0], list(range(100)), (0.07, 0.29))
    assert tau == [92.0, 70.0]


def test_tpir_nan_tops_never_alarm_and_a_nan_mate_score_is_no_hit():
    nt = [NAN, 0.3, NAN, 0.8]
    tp, tau = both([0.9, NAN, 0.31, 0.2], [0, 0, 0, 0], nt, (0.0, 0.25, 0.5, 0.75, 1.0))
    assert tau == [0.8, 0.3, -INF, -INF, -INF]                     # the third and fourth largest are the NaNs
    assert tp == [1 / 4, 2 / 4, 3 / 4, 3 / 4, 3 / 4]
    tp, tau = both([0.5, NAN], [0, 0], [NAN, NAN], (0.01,))
    assert tau == [-INF] and tp == [1 / 2]


def test_tpir_raises():
    with pytest.raises(ValueError):
        J.tpir_at_fpir([], [], [0.5])
    with pytest.raises(ValueError):
        J.tpir_at_fpir([0.5], [0], [])
    with pytest.raises(ValueError):
        J.tpir_at_fpir([0.5, 0.4], [0], [0.1])
    with pytest.raises(ValueError):
        J.tpir_at_fpir([0.5], [-1], [0.1])
    with pytest.raises(ValueError):
        J.tpir_at_fpir([0.5], [0], [0.1], fpirs=(1.5,))
    for bad in (([], [], [0.5]), ([0.5], [0], [])):
        with pytest.raises(ValueError):
            NO.tpir_at_fpir(*bad)


def test_identification_metrics_split_mated_and_non_mated():
    res = dict(mate=np.array([1, -1, 0, -1, 2], dtype=np.int32), mate_rank=np.array([0, -1, 3, -1, 0], dtype=np.int32),
               mate_score=np.array([0.9, NAN, 0.2, NAN, 0.4]), top_score=np.array([[0.9], [0.5], [0.6], [0.3], [0.4]]))
    m = J.identification_metrics(res, ranks=(1, 5), fpirs=(0.01, 0.5))
    assert m["cmc"].tolist() == [2 / 3, 1.0] and m["tau"].tolist() == [0.5, 0.3] and m["tpir"].tolist() == [1 / 3, 2 / 3]
    o = NO.gallery_metrics(res, res["mate"], ranks=(1, 5), fpirs=(0.01, 0.5))
    assert o["cmc"] == m["cmc"].tolist() and o["tpir"] == m["tpir"].tolist()
    res["mate"][:] = -1
    with pytest.raises(ValueError):
        J.identification_metrics(res)


def test_identification_row_is_plain_text():
    txt = J.identification_row("ijbc", "IJBC", dict(cmc=np.array([0.5, 0.75, 1.0]), tpir=np.array([0.125, 0.98765])))
    head, row = txt.splitlines()
    assert [c.strip() for c in head.split("|")] == ["Methods", "rank-1", "rank-5", "rank-10", "TPIR@FPIR=0.01", "TPIR@FPIR=0.1"]
    assert [c.strip() for c in row.split("|")] == ["ijbc-IJBC", "50.00", "75.00", "100.00", "12.50", "98.77"]


# ----------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_ranking_order():
    row = np.array([0.5, NAN, 0.9, 0.5, -0.0, 0.0, NAN, 0.9], dtype=np.longdouble)
    assert NO.ranking(row) == [2, 7, 0, 3, 4, 5, 1, 6]


def test_oracle_search_on_exact_integers():
    unit = np.array([[1.0, 2.0], [3.0, -1.0], [0.5, 0.5], [NAN, 1.0], [2.0, 1.0]])
    probe, gallery, mate = [0, 3, 7], [1, 4, 9, 2, 4], [4, 0, 1]
    r = NO.search(unit, probe, gallery, mate, 3)
    assert float(NO.exact_score(unit[0], unit[4])) == 4.0
    # probe row 0: scores [1, 4, NaN, 1.5, 4] -> order 1, 4, 3, 0, 2
    assert r["top_idx"][0].tolist() == [1, 4, 3] and r["top_score"][0].astype(float).tolist() == [4.0, 4.0, 1.5]
    assert r["mate_rank"][0] == 1 and r["mate_score"][0] == 4.0 and r["best_nonmate"][0] == 4.0 and r["nonmate_pos"][0] == 1
    # a NaN probe row: every score NaN, the order is by position; the mate at 0 has rank 0, the best non-mate is position 1
    assert r["top_idx"][1].tolist() == [0, 1, 2] and np.isnan(r["top_score"][1].astype(float)).all()
    assert r["mate_rank"][1] == 0 and np.isnan(r["mate_score"][1]) and r["nonmate_pos"][1] == 1
    # a probe index outside the table
    assert r["top_idx"][2].tolist() == [-1, -1, -1] and r["mate_rank"][2] == -1 and r["nonmate_pos"][2] == -1
    assert np.isnan(r["best_nonmate"][2]) and np.isnan(r["mate_score"][2])
