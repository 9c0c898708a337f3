"""Host tests of the k-NN evaluation: the oracle against brute-force loops, holdout_split, ks filtering, the two parsers, and the
checkpoint key selection.  No GPU."""
import argparse
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import knn_oracle as KO  # noqa: E402
from lafs_cvpr2024_amd import eval_knn, knn  # noqa: E402
from lafs_cvpr2024_amd import lafs_train as LT  # noqa: E402


def test_oracle_search_against_brute_force():
    r = np.random.RandomState(0)
    bank, query = r.randn(9, 3).astype(np.float32), r.randn(4, 3).astype(np.float32)
    bank[5] = bank[2]                                       # a tie
    bank[7, 1] = np.nan
    top, S = KO.search(bank, query, 6, bank_pos0=100, exclude=[102, -1, 107, 100])
    for i in range(4):
        sc = [sum(float(query[i, d]) * float(bank[j, d]) for d in range(3)) for j in range(9)]
        for j in range(9):
            assert (math.isnan(sc[j]) and math.isnan(S[i, j])) or abs(sc[j] - S[i, j]) < 1e-12
        left = [j for j in range(9) if 100 + j != [102, -1, 107, 100][i]]
        picked = []
        while left and len(picked) < 6:                     # selection by repeated "nothing ranks before it"
            best = [a for a in left if not any(KO.before(sc[b], b, sc[a], a) for b in left if b != a)]
            assert len(best) == 1
            picked.append(best[0]); left.remove(best[0])
        assert list(top[i, :len(picked)]) == [100 + j for j in picked] and np.all(top[i, len(picked):] == -1)
    top, _ = KO.search(bank[:3], query, 6)
    assert np.all(top[:, 3:] == -1) and np.all(np.sort(top[:, :3], axis=1) == np.arange(3))
    assert KO.rank([1.0, float("nan"), 1.0, 2.0, float("nan")], [9, 3, 4, 7, 1]) == [7, 4, 9, 1, 3]
    b = KO.bound(bank[:2], query[:1])
    assert b.shape == (1, 2) and abs(b[0, 0] - 5 * 2.0 ** -24 * sum(abs(float(query[0, d]) * float(bank[0, d])) for d in range(3))) < 1e-15


def test_oracle_vote_against_brute_force():
    ts = np.array([[0.9, 0.5, 0.4, 0.1], [0.3, 0.3, 0.3, float("nan")]], np.float32)
    ti = np.array([[0, 1, 2, 3], [2, 1, 7, -1]])
    labels = [5, 3, 5, 3]
    out = KO.vote(ts, ti, labels, (1, 2, 4), 0.5)
    e = lambda s: math.exp(float(np.float32(s)) / 0.5)
    assert out[0][0] == [(5, e(0.9))] and out[1][0] == [(5, e(0.9)), (3, e(0.5))]
    assert [c for c, _ in out[2][0]] == [5, 3] and abs(out[2][0][0][1] - (e(0.9) + e(0.4))) < 1e-12
    assert [c for c, _ in out[2][1]] == [3, 5] and out[2][1][0][1] == out[2][1][1][1]       # equal votes: the smaller label; idx 7, -1 skipped
    assert KO.accuracies(out, [5, 5]) == [(100.0, 100.0), (50.0, 100.0), (50.0, 100.0)]


CASES = [([0, 0, 0, 1, 1, 2], 1, 1), ([3, 1, 3, 1, 3, 2, 2, 2, 2], 2, 1), ([7], 1, 1), ([4, 4, 5, 5, 5], 3, 1), ([1, 2, 1, 2, 1, 2, 1], 1, 3),
         ([], 1, 1), ([9, 8, 9, 8, 7, 9], 2, 2)]


@pytest.mark.parametrize("labels,n_holdout,min_bank", CASES)
def test_holdout_split_equals_the_oracle(labels, n_holdout, min_bank):
    b, q = knn.holdout_split(labels, n_holdout, min_bank)
    ob, oq = KO.holdout_split(labels, n_holdout, min_bank)
    assert list(b) == ob and list(q) == oq


def test_holdout_split_cases():
    b, q = knn.holdout_split([0, 0, 0, 1, 1, 2])            # the singleton 2 gives neither
    assert list(b) == [0, 1, 3] and list(q) == [2, 4]
    b, q = knn.holdout_split([4, 4, 5, 5, 5], n_holdout=3)  # n_holdout >= class size: neither
    assert len(b) == 0 and len(q) == 0
    b, q = knn.holdout_split([3, 1, 3, 1, 3], n_holdout=1)  # record order kept: the LAST record of each identity is the query
    assert list(b) == [0, 1, 2] and list(q) == [3, 4]
    again = knn.holdout_split([3, 1, 3, 1, 3], n_holdout=1)
    assert list(again[0]) == list(b) and list(again[1]) == list(q)
    with pytest.raises(ValueError):
        knn.holdout_split([1, 1], n_holdout=0)


def test_ks_filtering(capsys):
    assert knn.filter_ks((200, 10, 20, 100, 20), 150) == [10, 20, 100]
    assert "k = 200 dropped" in capsys.readouterr().out
    assert knn.filter_ks((10, 20), 20) == [10, 20] and knn.filter_ks((5,), 3) == []
    with pytest.raises(ValueError):
        knn.filter_ks((0,), 10)
    assert knn.parse_ks("10,20, 100,200") == (10, 20, 100, 200)
    assert knn.knn_classify(torch.zeros(3, 4), [0, 1, 2], torch.zeros(2, 4), [0, 1], ks=(5, 10)) == {}   # nothing left: nothing is launched
    text = knn.result_json({10: (50.0, 75.0)}, 40, 8, 0.07)
    assert text == knn.result_json({10: (50.0, 75.0)}, 40, 8, 0.07) and '"knn_top1_k10": 50.0' in text and '"n_bank": 40' in text


def test_eval_knn_parser():
    a = eval_knn.get_args_parser().parse_args(["--checkpoint", "c.pth", "--data_path", "d"])
    assert (a.checkpoint_key, a.nb_knn, a.temperature, a.holdout, a.max_images, a.batch_size, a.decode, a.landmark_ckpt) == \
        ("teacher", "10,20,100,200", 0.07, 1, 0, 256, "pillow", "")
    a = eval_knn.get_args_parser().parse_args(["--checkpoint", "c.pth", "--data_path", "d", "--checkpoint_key", "student", "--nb_knn", "5",
                                               "--decode", "device", "--holdout", "2", "--max_images", "100", "--landmark_ckpt", "l.pth"])
    assert (a.checkpoint_key, knn.parse_ks(a.nb_knn), a.decode, a.holdout, a.max_images, a.landmark_ckpt) == ("student", (5,), "device", 2, 100, "l.pth")
    with pytest.raises(SystemExit):
        eval_knn.get_args_parser().parse_args(["--data_path", "d"])


def test_lafs_train_parser_and_knn_off_builds_nothing(monkeypatch):
    p = argparse.ArgumentParser(parents=[LT.get_args_parser()])
    a = p.parse_args([])
    assert (a.knn_freq, a.knn_data_path, a.knn_nb, a.knn_temperature, a.knn_holdout, a.knn_max_images) == (0, "", "10,20,100,200", 0.07, 1, 0)
    a = p.parse_args(["--knn_freq", "2", "--knn_data_path", "d", "--knn_nb", "5,10", "--knn_temperature", "0.1", "--knn_holdout", "2",
                      "--knn_max_images", "64"])
    assert (a.knn_freq, a.knn_data_path, a.knn_nb, a.knn_temperature, a.knn_holdout, a.knn_max_images) == (2, "d", "5,10", 0.1, 2, 64)
    with pytest.raises(SystemExit):                         # --arch mynet (the default) without a landmark front-end
        LT.KnnProbe(a, engine=None, teacher_backbone=None, frontend=None, device=None)
    a.arch = "vit_tiny"
    probe = LT.KnnProbe(a, None, None, None, None)
    assert probe.records is None and probe.ks == (5, 10)    # nothing is read before the first evaluation
    assert [probe.due(e) for e in range(4)] == [False, True, False, True]
    a.knn_data_path = ""
    with pytest.raises(SystemExit):
        LT.KnnProbe(a, None, None, None, None)
    # --knn_freq 0: the probe is never constructed
    def boom(*args, **kw):
        raise AssertionError("--knn_freq 0 must build nothing")
    monkeypatch.setattr(LT, "KnnProbe", boom)
    a.knn_freq = 0
    assert LT.build_knn_probe(a, None, None, None, None) is None
    a.knn_freq = 1
    with pytest.raises(AssertionError):
        LT.build_knn_probe(a, None, None, None, None)


def test_checkpoint_key_selection_and_prefix_stripping():
    t = lambda v: torch.full((2,), float(v))
    ck = {"student": {"module.backbone.cls_token": t(1), "module.backbone.blocks.0.w": t(2), "module.head.mlp.0.weight": t(3)},
          "teacher": {"backbone.cls_token": t(4), "backbone.blocks.0.w": t(5), "head.mlp.0.weight": t(6), "backbone.backbone.x": t(7)},
          "epoch": 3}
    sd = eval_knn.backbone_state_dict(ck, "teacher")
    assert sorted(sd) == ["backbone.x", "blocks.0.w", "cls_token"] and float(sd["cls_token"][0]) == 4 and float(sd["backbone.x"][0]) == 7
    sd = eval_knn.backbone_state_dict(ck, "student")
    assert sorted(sd) == ["blocks.0.w", "cls_token"] and float(sd["blocks.0.w"][0]) == 2
    with pytest.raises(KeyError):
        eval_knn.backbone_state_dict(ck, "ema")
    with pytest.raises(KeyError):
        eval_knn.backbone_state_dict({"teacher": {"head.x": t(0)}}, "teacher")


def test_view_norm_follows_the_checkpoint_args():
    from lafs_cvpr2024_amd.augment import HALF_NORM, IMAGENET_NORM
    ns = argparse.Namespace
    assert knn.view_norm(ns(views="dino", views_norm="imagenet")) == IMAGENET_NORM
    assert knn.view_norm(ns(views="dino", views_norm="half")) == HALF_NORM
    assert knn.view_norm(ns(views="lafs", views_norm="imagenet")) == HALF_NORM and knn.view_norm(ns()) == HALF_NORM
