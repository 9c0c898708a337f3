"""GPU: the AdaFace head on two data-parallel ranks sharing the one GPU over gloo (the pattern of tests/test_gpu_dp.py): each rank forms
its margins from its own rows and keeps its own norm statistics, no collective is added, the replicas' weights stay bit-identical, and
sync_buffers() gives every rank rank 0's statistics."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _model(seed):
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8
    torch.manual_seed(seed)
    model = ViT_face_landmark_patch8(loss_type="AdaFace", GPU_ID=None, num_class=512, image_size=112, patch_size=8, dim=128, depth=2, heads=3,
                                     mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=False, drop_path_rate=0.0)
    with torch.no_grad():                              # a freshly initialised LayerNorm head gives every row the norm sqrt(dim): spread them
        model.mlp_head[0].weight.uniform_(0.5, 1.5)
        model.mlp_head[0].bias.normal_(0.0, 0.3)
    return model


def _data():
    g = torch.Generator().manual_seed(11)
    return [(torch.randint(0, 256, (16, 3, 112, 112), dtype=torch.uint8, generator=g), torch.randint(0, 512, (16,), generator=g)) for _ in range(2)]


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import adaface_cases as ac
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    model = _model(3 if rank == 0 else 77)             # rank 1: another initialisation and other statistics, overridden by the broadcast
    if rank == 1:
        with torch.no_grad():
            model.loss.batch_mean.fill_(5.0)
    model.train()
    eng = FinetuneEngine(model, 8, acc_step=2, margin_type=2, ada_t_alpha=0.5, device="cuda")
    assert eng.world == 2
    start = eng.ada_state.cpu().clone()
    state, bound = torch.tensor(ac.STATE0, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    for u8, y in _data():                              # one accumulation window, this rank's half of every micro-batch
        eng.micro_step(u8[rank * 8:(rank + 1) * 8].cuda(), y[rank * 8:(rank + 1) * 8].cuda(), lam=1.0)
        inv = (1 / eng.emb.detach().float().norm(dim=1).clamp_min(1e-12)).cpu()
        r = ac.margins_ref(inv, (float(state[0]), float(state[1])), 0.5, update=True)
        state, bound = r["state"][0], 0.5 * bound + r["state"][1] + 0.5 * 32 * ac.U * r["stats"][0]
    eng.optimizer_step(lr=1e-3, weight_decay=0.1)
    torch.cuda.synchronize()
    own = eng.ada_state.cpu().clone()
    eng.sync_buffers()
    torch.cuda.synchronize()
    torch.save({"start": start, "own": own, "ref": state, "bound": bound, "synced": eng.ada_state.cpu().clone(),
                "sd": (float(model.state_dict()["loss.batch_mean"]), float(model.state_dict()["loss.batch_std"])),
                "master": eng.arena.master.cpu()}, out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_adaface_two_ranks_keep_their_own_statistics_and_identical_weights(tmp_path):
    """Two ranks x batch 8, one accumulation window of two micro-steps.  Construction broadcasts rank 0's buffers (both start from 20,
    100); each rank's state then follows the fp64 EMA of ITS rows' norms (so the two differ: two ranks do not equal one rank on the full
    batch for this head); the weights after the step are bit-equal across the ranks; after sync_buffers() both hold rank 0's state,
    and state_dict() shows it."""
    out = str(tmp_path / "ada")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0", weights_only=False), torch.load(out + ".1", weights_only=False)
    assert r0["start"].tolist() == [20.0, 100.0] == r1["start"].tolist(), "buffers were not broadcast from rank 0"
    assert torch.equal(r0["master"], r1["master"])
    for r in (r0, r1):
        print(f"[adaface dp] state {r['own'].tolist()} vs fp64 {r['ref'].tolist()} (bound {r['bound'].tolist()})")
        assert bool(((r["own"].double() - r["ref"]).abs() <= r["bound"] + 2 * 2.0 ** -24 * r["ref"].abs()).all())
    assert not torch.equal(r0["own"], r1["own"])
    assert torch.equal(r0["synced"], r0["own"]) and torch.equal(r1["synced"], r0["own"])
    assert r1["sd"] == (float(r0["own"][0]), float(r0["own"][1]))
