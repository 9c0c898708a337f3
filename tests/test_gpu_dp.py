"""GPU: the data-parallel path of the engine itself (parameter broadcast, asynchronous flat-gradient and center all-reduces between
the graph segments, 1/world folded into the optimizer) with TWO processes sharing the one GPU over the gloo backend (RCCL needs
one device per rank; gloo accepts device tensors), against a single process on the concatenated batch."""
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


def _build(B, use_graph):
    import torch.nn as nn
    from lafs_cvpr2024_amd import vision_transformer as vits
    from lafs_cvpr2024_amd.dino_loss import DINOLoss
    from lafs_cvpr2024_amd.engine import LafsPretrainEngine
    from lafs_cvpr2024_amd.utils import MultiCropWrapper
    torch.manual_seed(0)
    LN6 = lambda d: nn.LayerNorm(d, eps=1e-6)
    mk = lambda: vits.VisionTransformer(img_size=[224], patch_size=8, embed_dim=128, depth=4, num_heads=2, qkv_bias=True, norm_layer=LN6)
    student = MultiCropWrapper(mk(), vits.DINOHead(128, 1024, hidden_dim=256, bottleneck_dim=64))
    teacher = MultiCropWrapper(mk(), vits.DINOHead(128, 1024, hidden_dim=256, bottleneck_dim=64))
    teacher.load_state_dict(student.state_dict())
    crit = DINOLoss(1024, 4, 0.07, 0.04, 3, 10)
    return LafsPretrainEngine(student, teacher, crit, B, n_local=2, use_graph=use_graph, device="cuda")


def _crops(B):
    g = torch.Generator().manual_seed(7)
    return [torch.randn(B, 3, 112, 112, generator=g).clamp(-1, 1) for _ in range(2)] + [torch.randn(B, 3, 48, 48, generator=g).clamp(-1, 1) for _ in range(2)]


def _worker(rank, world, port, out, use_graph, wire="f32"):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["LAFS_GRAD_WIRE"] = wire
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if rank == 1:
        torch.manual_seed(123)                       # a different initialisation on rank 1: the broadcast must override it
    eng = _build(2, use_graph)
    if rank == 1:
        assert eng.world == 2
    full = _crops(4)
    mine = [c[rank * 2:(rank + 1) * 2].cuda() for c in full]
    losses = []
    for it in range(3):
        losses.append(float(eng.step(mine, lr=1e-3, wd=0.04, momentum=0.9, teacher_temp=0.05, epoch=1).item()))
    torch.cuda.synchronize()
    torch.save({"student": eng.sa.master.cpu(), "teacher": eng.ta.master.cpu(), "center": eng.dino_loss.center.cpu(), "losses": losses},
               out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("use_graph", [False, True])
def test_two_ranks_on_one_gpu_equal_single_process_on_the_full_batch(tmp_path, use_graph):
    out = str(tmp_path / "dp")
    port = _free_port()
    mp.spawn(_worker, args=(2, port, out, use_graph), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0", weights_only=False), torch.load(out + ".1", weights_only=False)
    # the replicas stay identical (same broadcast start, same reduced gradients)
    assert torch.equal(r0["student"], r1["student"]) and torch.equal(r0["teacher"], r1["teacher"]) and torch.equal(r0["center"], r1["center"])
    eng = _build(4, use_graph)
    full = [c.cuda() for c in _crops(4)]
    losses = [float(eng.step(full, lr=1e-3, wd=0.04, momentum=0.9, teacher_temp=0.05, epoch=1).item()) for _ in range(3)]
    # first-step loss of the full batch = mean of the two half-batch losses (both depend only on the shared initial weights)
    assert abs(0.5 * (r0["losses"][0] + r1["losses"][0]) - losses[0]) < 2e-4 * losses[0]
    c_ref = eng.dino_loss.center.cpu()          # three steps in: the weights already differ by Adam's round-off sign flips
    assert float((r0["center"] - c_ref).abs().max()) < 0.1 * float(c_ref.abs().max()) + 1e-6
    d = (r0["student"] - eng.sa.master.cpu()).abs()
    # Adam turns a sign flip of a round-off-sized gradient into a 2*lr step: a few percent of the entries may differ by up to 2*lr*steps
    assert float(d.median()) < 1e-6 and float((d > 1e-4).float().mean()) < 0.06 and float(d.max()) < 7e-3
    dt = (r0["teacher"] - eng.ta.master.cpu()).abs()
    assert float(dt.max()) < 1e-3


def _rccl_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["LAFS_ONE_GRAPH"] = "0"               # the multi-rank launch structure: one graph per segment, collectives between them
    os.environ["LAFS_REDUCE_SINGLE_RANK"] = "1"      # ... with the all-reduces really issued (RCCL, one rank)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    eng = _build(4, True)
    assert eng.n_segments > 1 and eng.reducer.active
    full = [c.cuda() for c in _crops(4)]
    losses = [float(eng.step(full, lr=1e-3, wd=0.04, momentum=0.9, teacher_temp=0.05, epoch=1).item()) for _ in range(3)]
    assert not eng._one_graph and len(eng._graphs) > 1
    t = torch.ones(1 << 20, device="cuda")
    dist.all_reduce(t)                                # the backend is alive after the captured segments
    torch.cuda.synchronize()
    assert float(t.sum()) == float(1 << 20)
    torch.save({"student": eng.sa.master.cpu(), "teacher": eng.ta.master.cpu(), "center": eng.dino_loss.center.cpu(), "losses": losses}, out)
    dist.destroy_process_group()


def test_multi_rank_launch_structure_over_rccl_with_one_rank(tmp_path):
    """What one GPU can show of the RCCL path: init_process_group("nccl", device_id=...), the segmented graphs captured while the
    process group's watchdog thread is alive, asynchronous RCCL all-reduces of the gradient slices and of the center sums issued
    between the graph replays and waited for stream-side -- against the single-graph engine without a process group."""
    out = str(tmp_path / "rccl1")
    mp.spawn(_rccl_worker, args=(1, _free_port(), out), nprocs=1, join=True)
    r = torch.load(out, weights_only=False)
    eng = _build(4, True)
    full = [c.cuda() for c in _crops(4)]
    losses = [float(eng.step(full, lr=1e-3, wd=0.04, momentum=0.9, teacher_temp=0.05, epoch=1).item()) for _ in range(3)]
    assert eng._one_graph
    assert abs(r["losses"][0] - losses[0]) < 1e-6 * abs(losses[0])
    assert abs(r["losses"][2] - losses[2]) < 5e-3 * abs(losses[2])
    d = (r["student"] - eng.sa.master.cpu()).abs()
    assert float(d.median()) < 1e-6 and float((d > 1e-4).float().mean()) < 0.06 and float(d.max()) < 7e-3
    assert float((r["teacher"] - eng.ta.master.cpu()).abs().max()) < 1e-3


def test_two_ranks_with_bf16_gradients_on_the_wire(tmp_path):
    """LAFS_GRAD_WIRE=bf16 (opt-in): gradient slices are cast to bf16, all-reduced and cast back (half the bytes on the links).  The
    replicas must stay bit-identical to each other (both receive the same sums) and close to the fp32-wire run: the first step's
    losses are equal (forward only), later ones differ at the level of a bf16 rounding of the gradients."""
    outs = {}
    for wire in ("f32", "bf16"):
        out = str(tmp_path / f"dp_{wire}")
        mp.spawn(_worker, args=(2, _free_port(), out, True, wire), nprocs=2, join=True)
        outs[wire] = (torch.load(out + ".0", weights_only=False), torch.load(out + ".1", weights_only=False))
    a0, a1 = outs["bf16"]
    assert torch.equal(a0["student"], a1["student"]) and torch.equal(a0["teacher"], a1["teacher"]) and torch.equal(a0["center"], a1["center"])
    f0 = outs["f32"][0]
    assert abs(a0["losses"][0] - f0["losses"][0]) < 1e-6 * abs(f0["losses"][0])
    assert abs(a0["losses"][2] - f0["losses"][2]) < 2e-2 * abs(f0["losses"][2])
    d = (a0["student"] - f0["student"]).abs()
    assert 0 < float(d.max()) < 7e-3 and float(d.median()) < 1e-4             # it IS a different arithmetic, within Adam's step sizes


def _pfc_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lafs_cvpr2024_amd.partial_fc import PartialFC, shard_range
    g = torch.Generator().manual_seed(5)
    C, D, B = 1000, 64, 8
    Wfull = torch.randn(C, D, generator=g) * 0.05
    emb = torch.randn(world * B, D, generator=g)
    lab = torch.randint(0, C, (world * B,), generator=g)
    pfc = PartialFC(D, C, B, sample_rate=1.0, device="cuda")
    start, n = shard_range(C, rank, world)
    assert (pfc.class_start, pfc.num_local) == (start, n)
    with torch.no_grad():
        pfc.weight.copy_(Wfull[start:start + n])
    loss, demb = pfc.forward_backward(emb[rank * B:(rank + 1) * B].cuda(), lab[rank * B:(rank + 1) * B].cuda())
    torch.cuda.synchronize()
    torch.save({"loss": loss.cpu(), "demb": demb.cpu(), "dW": pfc.arena.view(pfc.arena.grad, "weight", (n, D)).cpu(), "start": start},
               out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_partial_fc_two_class_shards_on_one_gpu(tmp_path):
    """PartialFC with the class centres sharded over two ranks (HIP kernels + the MAX / SUM statistics exchange + gather /
    reduce-scatter of the embeddings) == the unsharded CosFace + cross-entropy of the oracle on the global batch."""
    from oracle import margin
    out = str(tmp_path / "pfc")
    port = _free_port()
    mp.spawn(_pfc_worker, args=(2, port, out), nprocs=2, join=True)
    g = torch.Generator().manual_seed(5)
    C, D, B = 1000, 64, 8
    Wfull = (torch.randn(C, D, generator=g) * 0.05).requires_grad_(True)
    emb = torch.randn(2 * B, D, generator=g).requires_grad_(True)
    lab = torch.randint(0, C, (2 * B,), generator=g)
    ref = margin.partial_fc_reference(emb, Wfull, lab)
    ref.backward()
    for r in range(2):
        got = torch.load(out + f".{r}", weights_only=False)
        e = emb.grad[r * B:(r + 1) * B]
        w = Wfull.grad[got["start"]:got["start"] + got["dW"].shape[0]]
        errs = (abs(float(got["loss"].detach()) - float(ref)) / abs(float(ref)), float((got["demb"] - e).abs().max()) / float(e.abs().max()),
                float((got["dW"] - w).abs().max()) / float(Wfull.grad.abs().max()))
        print(f"[pfc] rank {r}: loss / dE / dW errors {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
        assert max(errs) < 1e-2, errs                # (round 5: 2 % / 3 %; the observed values are a few 1e-3: bf16 operands of the logit GEMM)


def _pfc_soft_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lafs_cvpr2024_amd.partial_fc import PartialFC, shard_range
    g = torch.Generator().manual_seed(6)
    C, D, B = 1000, 64, 8
    Wfull = torch.randn(C, D, generator=g) * 0.05
    emb = torch.randn(world * B, D, generator=g)
    lab = torch.randint(0, C, (world * B,), generator=g)
    pfc = PartialFC(D, C, B, sample_rate=1.0, device="cuda")
    start, n = shard_range(C, rank, world)
    with torch.no_grad():
        pfc.weight.copy_(Wfull[start:start + n])
    mine = lab[rank * B:(rank + 1) * B].cuda()
    lam = _PFC_SOFT_LAMS[rank]                               # rank 0 drew "no mixup" (hard labels), rank 1 mixes with its flipped batch
    loss, demb = pfc.forward_backward(emb[rank * B:(rank + 1) * B].cuda(), mine, labels2=None if lam == 1.0 else mine.flip(0), lam=lam)
    torch.cuda.synchronize()
    torch.save({"loss": loss.detach().cpu(), "demb": demb.cpu(), "dW": pfc.arena.view(pfc.arena.grad, "weight", (n, D)).cpu(), "start": start},
               out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


_PFC_SOFT_LAMS = (1.0, 0.3)


def test_partial_fc_soft_labels_with_a_rank_that_drew_no_mixup(tmp_path):
    """The product's class-sharded head (partial_fc.PartialFC: HIP kernels + exchange) with the reference's soft mixup targets where
    the ranks drew DIFFERENT lambdas, one of them 1.0 (90 % of the draws at mixup_prob 0.1, train_largescale.py:389): the ranks'
    collective sequences must not diverge (round-5 advisor finding: a per-rank soft / hard choice hangs), and loss and gradients
    equal the unsharded CosFace-soft + soft-target CE of the oracle (F10-pinned) on the global batch."""
    from oracle import margin
    out = str(tmp_path / "pfcs")
    mp.spawn(_pfc_soft_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    g = torch.Generator().manual_seed(6)
    C, D, B = 1000, 64, 8
    Wfull = (torch.randn(C, D, generator=g) * 0.05).requires_grad_(True)
    emb = torch.randn(2 * B, D, generator=g).requires_grad_(True)
    lab = torch.randint(0, C, (2 * B,), generator=g)
    lab2 = torch.cat([lab[:B], lab[B:].flip(0)])
    lam_rows = torch.tensor([_PFC_SOFT_LAMS[0]] * B + [_PFC_SOFT_LAMS[1]] * B)
    target = torch.zeros(2 * B, C)
    target.scatter_add_(1, lab.view(-1, 1), lam_rows.view(-1, 1))
    target.scatter_add_(1, lab2.view(-1, 1), (1 - lam_rows).view(-1, 1))
    logits = margin.cosface_logits(emb, Wfull, target)
    ref = margin.soft_target_cross_entropy(logits, target)
    ref.backward()
    worst = 0.0
    for r in range(2):
        got = torch.load(out + f".{r}", weights_only=False)
        e = emb.grad[r * B:(r + 1) * B]
        w = Wfull.grad[got["start"]:got["start"] + got["dW"].shape[0]]
        errs = (abs(float(got["loss"]) - float(ref)) / abs(float(ref)), float((got["demb"] - e).abs().max()) / float(e.abs().max()),
                float((got["dW"] - w).abs().max()) / float(Wfull.grad.abs().max()))
        print(f"[pfc-soft] rank {r}: loss / dE / dW errors {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
        worst = max(worst, *errs)
    assert worst < 1.5e-2, worst                       # (observed 8.2e-3: bf16 operands of the logit GEMM; hard labels above: 6.1e-3, gate 1e-2)


# ------------------------------------------------------------------------------------------------ dense fine-tune head, DP
def _ft_model(with_land, seed=3):
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8
    torch.manual_seed(seed)
    return ViT_face_landmark_patch8(loss_type="CosFace", GPU_ID=None, num_class=512, image_size=112, patch_size=8, dim=128, depth=4, heads=3,
                                    mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=with_land, drop_path_rate=0.0)


def _ft_data(B):
    g = torch.Generator().manual_seed(11)
    return [(torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8, generator=g), torch.randint(0, 512, (B,), generator=g)) for _ in range(3)]


def _ft_worker(rank, world, port, out, with_land, use_graph):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    # rank 1 starts from ANOTHER initialisation and from perturbed BatchNorm statistics: the engine's construction-time broadcast of
    # parameters and buffers (DDP, train_largescale.py:676-677) has to override both
    model = _ft_model(with_land, seed=3 if rank == 0 else 77)
    if rank == 1:
        with torch.no_grad():
            for b in model.buffers():
                if b.is_floating_point():
                    b.add_(0.25)
    if with_land:
        model.eval()                                  # BatchNorm batch statistics differ between a half batch and the full one
    eng = FinetuneEngine(model, 8, acc_step=3, device="cuda", use_graph=use_graph)
    assert eng.world == 2 and eng.use_graph == use_graph
    w0 = eng.arena.master.clone()
    bufs = torch.cat([b.detach().float().flatten().cpu() for b in model.buffers()]) if with_land else torch.zeros(1)
    for u8, y in _ft_data(16):                        # this rank's half of every micro-batch
        # batch mixup pairs row i with row B-1-i of the SAME rank's batch: lam = 1 keeps the two decompositions comparable
        loss = eng.micro_step(u8[rank * 8:(rank + 1) * 8].cuda(), y[rank * 8:(rank + 1) * 8].cuda(), lam=1.0)
    assert eng._reduced                               # the slices went out during the third backward, not at the optimizer step
    if use_graph:                                     # two single-graph micro-steps, then the window's last one as one graph per segment
        keys = sorted(eng._graphs)
        assert [len(eng._graphs[k]) for k in keys if not k[2]] == [1, 1] and all(len(eng._graphs[k]) > 2 for k in keys if k[2]), keys
    eng.reducer.wait_all()
    gsum = eng.arena.grad.clone()                     # SUM over ranks of the accumulated local-mean gradients
    eng._reduced = True
    eng.optimizer_step(lr=1e-3, weight_decay=0.1)
    torch.cuda.synchronize()
    torch.save({"grad": gsum.cpu(), "master": eng.arena.master.cpu(), "moved": float((eng.arena.master - w0).abs().max()), "w0": w0.cpu(),
                "bufs": bufs}, out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("with_land,use_graph", [(False, False), (False, True), (True, True)])
def test_dense_finetune_two_ranks_equal_one_rank_on_the_full_batch(tmp_path, with_land, use_graph):
    """train_largescale.py under DDP (:676-677, 842-891): two ranks x batch 8, acc_step 3, against one process x batch 16.  Rank 1
    is built from another seed and perturbed BatchNorm statistics: the engine's broadcast from rank 0 must override them.  The
    gradient slices are launched as the last backward retires them (head first) and optimizer_step only waits; the summed
    gradient over 1/world equals the full-batch gradient, the replicas end bit-identical and close to the single-process run --
    eager, and captured (the window's last micro-step as one hipGraph per segment with the collectives between the replays)."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    out = str(tmp_path / "ft")
    port = _free_port()
    mp.spawn(_ft_worker, args=(2, port, out, with_land, use_graph), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0", weights_only=False), torch.load(out + ".1", weights_only=False)
    assert torch.equal(r0["w0"], r1["w0"]) and torch.equal(r0["bufs"], r1["bufs"]), "parameters / buffers were not broadcast from rank 0"
    assert torch.equal(r0["grad"], r1["grad"]) and torch.equal(r0["master"], r1["master"]) and r0["moved"] > 1e-4
    model = _ft_model(with_land)
    if with_land:
        model.eval()
    eng = FinetuneEngine(model, 16, acc_step=3, device="cuda")
    for u8, y in _ft_data(16):
        eng.micro_step(u8.cuda(), y.cuda(), lam=1.0)
    g_full = eng.arena.grad.clone().cpu()
    # rank-local losses are means over 8 rows: SUM over ranks / world == mean over the 16 rows
    rel = float((r0["grad"] * 0.5 - g_full).norm() / g_full.norm())
    assert rel < 2e-3, rel
    eng.optimizer_step(lr=1e-3, weight_decay=0.1)
    d = (r0["master"] - eng.arena.master.cpu()).abs()
    assert float(d.median()) < 1e-6 and float((d > 1e-4).float().mean()) < 0.06, (float(d.median()), float((d > 1e-4).float().mean()))
