"""CPU checks of the host side of the linear probe (lafs_cvpr2024_amd/linear_probe.py, eval_linear.py): the few-shot selection on top of
knn.holdout_split, the label re-indexing, the learning-rate schedule, the result file and the tool's defaults.  The kernels and the
training itself are judged on the GPU (tests/test_gpu_linear_probe.py)."""
import json

import numpy as np
import pytest
import torch

from lafs_cvpr2024_amd import eval_linear, knn
from lafs_cvpr2024_amd import linear_probe as lp


def _labels():
    # identities 40 (5 records), 7 (3), 19 (1: dropped by the hold-out), 3 (2), interleaved in record order
    return np.array([40, 7, 40, 3, 19, 40, 7, 3, 40, 7, 40])


def test_shots_keep_the_first_k_bank_records_of_every_identity_in_order():
    lab = _labels()
    bank, query = knn.holdout_split(lab, n_holdout=1)
    assert bank.tolist() == [0, 1, 2, 3, 5, 6, 8] and query.tolist() == [7, 9, 10]
    assert lp.select_shots(lab, bank, 0).tolist() == bank.tolist()
    assert lp.select_shots(lab, bank, 2).tolist() == [0, 1, 2, 3, 6]            # 40: 0, 2; 7: 1, 6; 3: its only bank record
    assert lp.select_shots(lab, bank, 1).tolist() == [0, 1, 3]
    assert lp.select_shots(lab, bank, 99).tolist() == bank.tolist()
    # a brute-force restatement on random labels
    rng = np.random.RandomState(0)
    lab = rng.randint(0, 12, size=200)
    bank, _ = knn.holdout_split(lab, n_holdout=2)
    for k in (1, 3, 5):
        seen, want = {}, []
        for i in bank:
            seen[lab[i]] = seen.get(lab[i], 0) + 1
            if seen[lab[i]] <= k:
                want.append(i)
        assert lp.select_shots(lab, bank, k).tolist() == want


def test_split_reindexes_the_surviving_identities():
    lab = _labels()
    train_i, val_i, y_train, y_val, n_class = lp.probe_split(lab, holdout=1, shots=0)
    assert n_class == 3                                                          # 19 has one record: neither trained nor validated
    assert train_i.tolist() == [0, 1, 2, 3, 5, 6, 8] and val_i.tolist() == [7, 9, 10]
    assert y_train.tolist() == [2, 1, 2, 0, 2, 1, 2]                             # 3 -> 0, 7 -> 1, 40 -> 2
    assert y_val.tolist() == [0, 1, 2]
    few = lp.probe_split(lab, holdout=1, shots=1)
    assert few[0].tolist() == [0, 1, 3] and few[2].tolist() == [2, 1, 0]
    assert few[1].tolist() == val_i.tolist() and few[3].tolist() == y_val.tolist() and few[4] == 3      # validation unchanged
    with pytest.raises(ValueError):
        lp.probe_split(np.array([1, 2, 3]), holdout=1)


@pytest.mark.parametrize("epochs,lr,batch", [(100, 0.001, 1024), (10, 0.4, 64), (1, 0.01, 256), (7, 0.003, 96)])
def test_schedule_is_cosine_annealing_stepped_per_epoch(epochs, lr, batch):
    base = lp.scaled_lr(lr, batch)
    assert base == pytest.approx(lr * batch / 256.0, rel=1e-15)
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=base, momentum=0.9, weight_decay=0)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, epochs, eta_min=0)
    for epoch in range(epochs):
        assert lp.cosine_lr(base, epoch, epochs) == pytest.approx(opt.param_groups[0]["lr"], rel=1e-9, abs=1e-18)
        opt.step()
        sched.step()
    assert lp.cosine_lr(base, 0, epochs) == base


def test_result_json_is_a_function_of_the_result_alone():
    res = {"top1": 87.5, "top5": 100.0, "loss": 0.12345678901234, "train_top1": 100.0, "n_train": 40, "n_val": np.int64(8), "n_class": 8}
    a = lp.result_json(res)
    b = lp.result_json(dict(reversed(list(res.items()))))
    assert a == b and a.endswith("\n")
    d = json.loads(a)
    assert set(d) == set(lp.RESULT_KEYS) == {"top1", "top5", "loss", "train_top1", "n_train", "n_val", "n_class"}
    assert d["n_val"] == 8 and isinstance(d["n_val"], int) and d["loss"] == res["loss"]


def test_tool_defaults_per_arch():
    p = eval_linear.get_args_parser()
    a = p.parse_args(["--checkpoint", "c.pth", "--data_path", "d"])
    assert (a.epochs, a.lr, a.batch_size, a.holdout, a.shots, a.seed) == (100, 0.001, 1024, 1, 0, 0)
    assert a.checkpoint_key == "teacher" and a.avgpool_patchtokens is False and a.n_last_blocks is None
    assert (a.max_images, a.decode, a.num_workers, a.landmark_ckpt) == (0, "pillow", 4, "")
    for arch in ("vit_tiny", "vit_small", "vit_base"):
        assert eval_linear.resolve_n_last_blocks(a, arch) == 4
    for arch in ("mynet", "fvit"):
        assert eval_linear.resolve_n_last_blocks(a, arch) == 1
    b = p.parse_args(["--checkpoint", "c.pth", "--data_path", "d", "--n_last_blocks", "2", "--avgpool_patchtokens", "true", "--shots", "5"])
    assert eval_linear.resolve_n_last_blocks(b, "fvit") == 2 and eval_linear.resolve_n_last_blocks(b, "vit_small") == 2
    assert b.avgpool_patchtokens is True and b.shots == 5
    kp = __import__("lafs_cvpr2024_amd.eval_knn", fromlist=["x"]).get_args_parser().parse_args(["--checkpoint", "c.pth", "--data_path", "d"])
    for k in ("checkpoint_key", "landmark_ckpt", "max_images", "decode", "num_workers", "holdout"):
        assert getattr(a, k) == getattr(kp, k), k                                 # the shared flags: eval_knn's defaults


def test_probe_refuses_intermediate_layers_of_the_face_vits():
    class NotAViT(torch.nn.Module):
        pass
    with pytest.raises(ValueError, match="n_last_blocks"):
        lp.probe_features(NotAViT(), iter(()), n_last_blocks=2)
    with pytest.raises(ValueError, match="avgpool"):
        lp.probe_features(NotAViT(), iter(()), avgpool=True)
