"""GPU: landmark supervision (`pre_land and keep_land`) under data parallelism -- two processes sharing the one GPU over gloo, as
tests/test_gpu_dp.py runs the dense fine-tune head, against one process on the full batch."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
LAND_WEIGHT = 100.0


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _model(seed=3):
    from conftest import det_fill_random
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8
    torch.manual_seed(seed)
    m = ViT_face_landmark_patch8(loss_type="CosFace", GPU_ID=None, num_class=512, image_size=112, patch_size=8, dim=128, depth=2, heads=3,
                                 mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=True, drop_path_rate=0.0)
    det_fill_random(m.stn); det_fill_random(m.output_layer)
    return m.eval()                                   # BatchNorm batch statistics differ between a half batch and the full one


def _teacher():
    from conftest import det_fill
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import face_landmark_4simmin_glo_loc
    t = face_landmark_4simmin_glo_loc(loss_type="None", GPU_ID=None, num_class=10, num_patches=196, image_size=112, patch_size=8, dim=64,
                                      depth=1, heads=1, mlp_dim=64)
    det_fill(t.stn); det_fill(t.output_layer)
    return t.eval()


def _data(B):
    g = torch.Generator().manual_seed(11)
    return [(torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8, generator=g), torch.randint(0, 512, (B,), generator=g)) for _ in range(3)]


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    eng = FinetuneEngine(_model(3 if rank == 0 else 77), 8, acc_step=3, device="cuda", landmark_teacher=_teacher(), keep_land=True)
    assert eng.world == 2
    lands = []
    for u8, y in _data(16):                           # this rank's half of every micro-batch
        eng.micro_step(u8[rank * 8:(rank + 1) * 8].cuda(), y[rank * 8:(rank + 1) * 8].cuda(), lam=1.0, land_weight=LAND_WEIGHT)
        lands.append(float(eng.loss_land.item()))
    assert eng._reduced
    eng.reducer.wait_all()
    gsum = eng.arena.grad.clone()                     # SUM over ranks of the accumulated local-mean gradients
    eng._reduced = True
    eng.optimizer_step(lr=1e-3, weight_decay=0.1)
    torch.cuda.synchronize()
    torch.save({"grad": gsum.cpu(), "master": eng.arena.master.cpu(), "lands": lands}, out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_mode_b_two_ranks_equal_one_rank_on_the_full_batch(tmp_path):
    """Two ranks x batch 8, acc_step 3, landmark weight 100, against one process x batch 16 (tolerances of
    test_dense_finetune_two_ranks_equal_one_rank_on_the_full_batch): each rank's landmark term is the mean over its own rows, so the
    summed gradient over 1 / world is the full batch's, and the mean of the two ranks' loss_land is the full batch's."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    out = str(tmp_path / "ft")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0", weights_only=False), torch.load(out + ".1", weights_only=False)
    assert torch.equal(r0["grad"], r1["grad"]) and torch.equal(r0["master"], r1["master"])
    eng = FinetuneEngine(_model(), 16, acc_step=3, device="cuda", landmark_teacher=_teacher(), keep_land=True)
    lands = []
    for u8, y in _data(16):
        eng.micro_step(u8.cuda(), y.cuda(), lam=1.0, land_weight=LAND_WEIGHT)
        lands.append(float(eng.loss_land.item()))
    g_full = eng.arena.grad.clone().cpu()
    for a, b, c in zip(r0["lands"], r1["lands"], lands):
        assert abs(0.5 * (a + b) - c) < 1e-4 * c, (r0["lands"], r1["lands"], lands)
    rel = float((r0["grad"] * 0.5 - g_full).norm() / g_full.norm())
    print(f"[mode B, two ranks] gradient rel-L2 against the full batch {rel:.2e}; loss_land {lands}")
    assert rel < 2e-3, rel
    # the landmark term is a large part of what reaches the CNN: without it the comparison above would not notice it missing
    plain = FinetuneEngine(_model(), 16, acc_step=3, device="cuda")
    for u8, y in _data(16):
        plain.micro_step(u8.cuda(), y.cuda(), lam=1.0)
    assert float((plain.arena.grad.cpu() - g_full).norm() / g_full.norm()) > 0.1
    eng.optimizer_step(lr=1e-3, weight_decay=0.1)
    d = (r0["master"] - eng.arena.master.cpu()).abs()
    assert float(d.median()) < 1e-6 and float((d > 1e-4).float().mean()) < 0.06, (float(d.median()), float((d > 1e-4).float().mean()))
