"""GPU: the k-NN evaluation end to end -- knn.knn_classify against the oracle of tests/knn_oracle.py, the eval_knn tool on checkpoints
of 2-step lafs_train runs (DINO ViT, fViT, Part-fViT with a random landmark CNN), and lafs_train.py --knn_freq, which must leave the
run bit-identical.  The data is 8 identities x 6 synthetic images in the RecordIO layout (what tools/make_synthetic_rec.py writes)."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu

import knn_oracle as KO  # noqa: E402


@pytest.fixture(scope="module")
def rec_dir(tmp_path_factory):
    from PIL import Image
    from lafs_cvpr2024_amd import recordio as R
    out = tmp_path_factory.mktemp("knn_rec")
    n_ids, per = 8, 6
    rng = np.random.RandomState(0)
    w = R.IndexedRecordWriter(str(out / "train.idx"), str(out / "train.rec"))
    n_img = n_ids * per
    w.write_idx(0, R.pack(R.IRHeader(2, [n_img + 1, n_img + 1 + n_ids], 0, 0), b""))
    yy, xx = np.mgrid[0:112, 0:112]
    key = 1
    for ident in range(n_ids):
        base = np.stack([127 + 90 * np.sin(xx / (5.0 + ident % 7) + c) * np.cos(yy / (6.0 + c) - ident) for c in range(3)], -1)
        for _ in range(per):
            img = np.clip(base + rng.randn(112, 112, 3) * 25, 0, 255).astype(np.uint8)
            b = io.BytesIO()
            Image.fromarray(img).save(b, format="JPEG", quality=95)
            w.write_idx(key, R.pack(R.IRHeader(0, float(ident), key, 0), b.getvalue()))
            key += 1
    for ident in range(n_ids):
        w.write_idx(n_img + 1 + ident, R.pack(R.IRHeader(2, [1 + ident * per, 1 + (ident + 1) * per], n_img + 1 + ident, 0), b""))
    w.close()
    return out


def _single_process(monkeypatch, port):
    monkeypatch.setenv("MASTER_PORT", str(port))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)


def _train_args(extra, out):
    from lafs_cvpr2024_amd import lafs_train as L
    return L.get_args_parser().parse_args(
        (f"--out_dim 512 --batch_size_per_gpu 4 --local_crops_number 2 --warmup_epochs 0 --warmup_teacher_temp_epochs 0 --saveckp_freq 0 "
         f"--output_dir {out} " + extra).split())


def test_knn_classify_equals_the_oracle_and_chance_on_shuffled_labels():
    from lafs_cvpr2024_amd import knn
    bank, yb, query, yq = KO.clustered(0, 25, 48, 1000, 70, 1.5)
    ks, T = (10, 20, 100, 200), 0.07
    top, S = KO.search(bank, query, 200)
    ref = KO.accuracies(KO.vote(np.take_along_axis(S, top, axis=1), top, yb, ks, float(np.float32(T))), yq)
    db, dq = torch.from_numpy(bank).cuda(), torch.from_numpy(query).cuda()
    got = knn.knn_classify(db, yb, dq, yq, ks=ks, temperature=T)
    print("\nknn_classify:", got)
    assert list(got) == list(ks)
    for k, r in zip(ks, ref):
        assert got[k] == pytest.approx(r, abs=1e-9), (k, got[k], r)
    assert got[20][0] > 50.0                                 # the clusters are there to be found
    assert got == knn.knn_classify(db, yb, dq, yq, ks=ks, temperature=T, chunk_rows=301, splits=3)       # streamed: the same numbers
    yb_shuffled = np.random.RandomState(1).permutation(yb)
    lost = knn.knn_classify(db, yb_shuffled, dq, yq, ks=ks, temperature=T)
    assert all(lost[k][0] <= 15.0 for k in ks), lost          # 25 classes: chance is 4 %
    few = knn.knn_classify(db[:50], yb[:50], dq, yq, ks=ks, temperature=T)
    assert list(few) == [10, 20]                             # 100 and 200 exceed the bank: dropped


TOOL_CASES = [("--arch vit_tiny --views dino --data synthetic_u8", 29561),
              ("--arch fvit --fvit_dims 128,2,2,256", 29562),
              ("--arch mynet --mynet_dims 128,2,2,256 --data synthetic_u8", 29563)]


@pytest.mark.parametrize("arch,port", TOOL_CASES)
def test_tool_on_a_two_step_checkpoint(tmp_path, monkeypatch, rec_dir, arch, port, capsys):
    from lafs_cvpr2024_amd import eval_knn
    from lafs_cvpr2024_amd import lafs_train as L
    _single_process(monkeypatch, port)
    if "mynet" in arch:                                      # a random landmark CNN, the same one for the run and both evaluations
        torch.manual_seed(0)
        torch.save(L.build_landmark_cnn("").state_dict(), tmp_path / "land.pth")
        arch += f" --landmark_ckpt {tmp_path / 'land.pth'}"
    L.train_lafs(_train_args(f"{arch} --epochs 1 --steps_per_epoch 2", tmp_path))
    ck = tmp_path / "checkpoint.pth"
    argv = ["--checkpoint", str(ck), "--data_path", str(rec_dir), "--nb_knn", "5,10,20,100", "--batch_size", "16", "--num_workers", "0"]
    res = eval_knn.main(argv)
    first = (tmp_path / "knn.json").read_bytes()
    assert "k = 100 dropped" in capsys.readouterr().out and list(res) == [5, 10, 20]
    d = json.loads(first)
    assert set(d) == {"n_bank", "n_query", "temperature"} | {f"knn_top{t}_k{k}" for t in (1, 5) for k in (5, 10, 20)}
    assert d["n_bank"] == 40 and d["n_query"] == 8
    assert all(0.0 <= d[f"knn_top{t}_k{k}"] <= 100.0 for t in (1, 5) for k in (5, 10, 20))
    assert all(d[f"knn_top5_k{k}"] >= d[f"knn_top1_k{k}"] for k in (5, 10, 20))
    eval_knn.main(argv)
    assert (tmp_path / "knn.json").read_bytes() == first             # a second run: the same bytes


def test_knn_freq_leaves_the_run_bit_identical(tmp_path, monkeypatch, rec_dir):
    from lafs_cvpr2024_amd import lafs_train as L
    _single_process(monkeypatch, 29564)
    flags = []
    orig = L.KnnProbe.__call__

    def spy(self):
        before = self.model.training
        out = orig(self)
        flags.append((before, self.model.training))
        return out
    monkeypatch.setattr(L.KnnProbe, "__call__", spy)
    base = "--arch vit_tiny --views dino --data synthetic_u8 --epochs 2 --steps_per_epoch 2"
    plain, probed = tmp_path / "plain", tmp_path / "probed"
    plain.mkdir(); probed.mkdir()
    L.train_lafs(_train_args(base, plain))
    assert flags == []
    L.train_lafs(_train_args(f"{base} --knn_freq 1 --knn_data_path {rec_dir} --knn_nb 5,10", probed))
    assert len(flags) == 2 and all(b == a for b, a in flags)
    la = [json.loads(l) for l in (plain / "log.txt").read_text().splitlines()]
    lb = [json.loads(l) for l in (probed / "log.txt").read_text().splitlines()]
    assert len(la) == len(lb) == 2
    keys = {f"knn_top{t}_k{k}" for t in (1, 5) for k in (5, 10)}
    for a, b in zip(la, lb):
        assert keys <= set(b) and not keys & set(a) and all(0.0 <= b[k] <= 100.0 for k in keys)
        assert a == {k: v for k, v in b.items() if k not in keys}        # the loss (logged at the polled steps), lr, wd, epoch
    assert "train_loss" in la[0]
    ca = torch.load(plain / "checkpoint.pth", map_location="cpu", weights_only=False)
    cb = torch.load(probed / "checkpoint.pth", map_location="cpu", weights_only=False)
    for net in ("student", "teacher"):
        assert set(ca[net]) == set(cb[net])
        for k in ca[net]:
            assert torch.equal(ca[net][k], cb[net][k]), (net, k)
