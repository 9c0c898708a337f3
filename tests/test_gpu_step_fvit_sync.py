"""LAFS pre-training of an fViT pair on SEVERAL ranks (LafsPretrainEngine(..., sync_bn=True), lafs_train.py --arch fvit --sync_bn true):
the BatchNorm1d head normalises every crop group with the statistics of all ranks' cls rows, so W ranks with B / W images each compute
the single-process step on the full batch -- the reference's own two-step run in the F27 fixture (B = 4) pins a two-rank result.

Two processes share the one GPU over gloo (the pattern of tests/test_gpu_dp.py); rank r takes rows [2r, 2r + 2) of every F27 crop.
Measured against the fixture and held to the gates of tests/test_gpu_step_fvit.py (the two-rank run differs from the single-process
one in summation order only): mean of the ranks' losses, each rank's logits against its rows, the clipped gradients (the all-reduced
sum over 1 / world), both networks' running buffers, num_batches_tracked 2 / 1 then 4 / 2, center and post-step parameters with F16's
statistic.  The observed figures, worst over both steps and over the eager and captured runs, two ranks / one segmented rank:
                                                   two ranks   one rank    gate (test_gpu_step_fvit.py, unchanged)
  loss (relative)                                  1.04e-3     1.04e-3     2.1e-3
  logits, per rank against its rows (rel-L2)       3.04e-2     2.56e-2     5.2e-2
  clipped per-tensor gradients (rel-L2, worst)     8.09e-2     8.09e-2     1.62e-1   (layers.0.1.fn.norm.bias, step 1)
  BatchNorm running_mean / running_var (rel-L2)    3.35e-3     3.35e-3     6.7e-3
  post-step parameters (F16's statistic)           median 0.011 lr, 90 % quantile 0.057 lr (gates 0.05 lr / 0.6 lr)
No figure exceeds its gate, so no gate moved (DESIGN.md section 2 has the row).
The replicas (student and teacher masters, center, every BatchNorm buffer) must be bit-equal across the two ranks after the steps.
A one-rank RCCL run (LAFS_ONE_GRAPH=0, LAFS_REDUCE_SINGLE_RANK=1) takes the segmented form -- two forward graphs with the exchange
between them, the sums' all-reduce in front of the trunk backward -- and meets the same gates."""
import datetime
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu

from conftest import gate_errors, sub  # noqa: E402
from fvit_ssl_cases import BN, BN_BUFFERS, F27_B, F27_CFG, F27_K, F27_NLOCAL, ZERO_SUM, ZERO_SUM_SCALE, load_f27  # noqa: E402

GATE_LOSS, GATE_LOGITS, GATE_GRAD, GATE_BN = 2.1e-3, 5.2e-2, 1.62e-1, 6.7e-3          # tests/test_gpu_step_fvit.py
TIMEOUT = datetime.timedelta(seconds=90)                                               # a dead peer ends the test


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _build(B, use_graph, sync_bn=True):
    from lafs_cvpr2024_amd import vision_transformer as vits
    from lafs_cvpr2024_amd.dino_loss import DINOLoss
    from lafs_cvpr2024_amd.engine import LafsPretrainEngine
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViTs_face_overlap
    from lafs_cvpr2024_amd.utils import MultiCropWrapper
    mk = lambda: ViTs_face_overlap(dropout=0.0, emb_dropout=0.0, drop_path_rate=0.0, **F27_CFG)
    student = MultiCropWrapper(mk(), vits.DINOHead(64, F27_K, hidden_dim=64, bottleneck_dim=32, norm_last_layer=True))
    teacher = MultiCropWrapper(mk(), vits.DINOHead(64, F27_K, hidden_dim=64, bottleneck_dim=32))
    init = sub(load_f27(), "init.")
    student.load_state_dict(init); teacher.load_state_dict(init)
    crit = DINOLoss(F27_K, 2 + F27_NLOCAL, 0.07, 0.04, 3, 10)
    eng = LafsPretrainEngine(student, teacher, crit, B, n_local=F27_NLOCAL, clip_grad=3.0, freeze_last_layer=1, use_graph=use_graph,
                             device="cuda", sync_bn=sync_bn)
    return student, teacher, crit, eng


def _two_steps(student, teacher, crit, eng, rows):
    """The two F27 steps on rows [rows) of every crop; everything the test looks at, per step, on the CPU."""
    fx = load_f27()
    lrs, wds, moms = fx["hyper"].tolist()
    tt = crit.teacher_temp_schedule
    mine = [fx[f"crop{i}"].float()[rows[0]:rows[1]] for i in range(4)]
    steps = []
    for s in range(2):
        loss = eng.step(mine, lr=lrs[s], wd=wds[s], momentum=moms[s], teacher_temp=float(tt[s]), epoch=s)
        torch.cuda.synchronize()
        cpu = lambda d: {k: v.detach().cpu().clone() for k, v in d.items()}
        steps.append(dict(loss=float(loss.item()), s_out=eng.logits_s[:, :256].cpu(), t_out=eng.logits_t[:, :256].cpu(),
                          grad=cpu({k: p.grad for k, p in student.named_parameters() if p.grad is not None}), student=cpu(student.state_dict()),
                          teacher=cpu(teacher.state_dict()), center=crit.center.cpu().clone()))
    return dict(steps=steps, masters=(eng.sa.master.cpu(), eng.ta.master.cpu()), n_graphs=None if eng._graphs is None else len(eng._graphs),
                n_segments=eng.n_segments, n_fwd=eng.n_fwd)


def _worker(rank, world, port, out, use_graph):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=TIMEOUT)
    student, teacher, crit, eng = _build(F27_B // world, use_graph)
    assert eng.world == world and eng.sync_bn and eng.n_fwd == 2
    b = F27_B // world
    torch.save(_two_steps(student, teacher, crit, eng, (rank * b, (rank + 1) * b)), out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


def _rccl_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["LAFS_ONE_GRAPH"] = "0"
    os.environ["LAFS_REDUCE_SINGLE_RANK"] = "1"
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0), timeout=TIMEOUT)
    student, teacher, crit, eng = _build(F27_B, True)
    assert eng.sync_bn and eng.n_fwd == 2 and eng.reducer.active
    res = _two_steps(student, teacher, crit, eng, (0, F27_B))
    assert not eng._one_graph
    t = torch.ones(1 << 16, device="cuda")
    dist.all_reduce(t)                                                       # the backend is alive after the captured segments
    torch.cuda.synchronize()
    assert float(t.sum()) == float(1 << 16)
    torch.save(res, out + ".0")
    dist.destroy_process_group()


def _against_f27(outs, tag):
    """Measures everything first, prints it, then holds it to the gates."""
    fx = load_f27()
    world = len(outs)
    b = F27_B // world
    lrs, wds, moms = fx["hyper"].tolist()
    names = [str(n) for n in fx["norm_names"]]
    seen = dict(loss={}, logits={}, grad={}, bn={})
    checks = []
    for s in range(2):
        st = [o["steps"][s] for o in outs]
        ref_loss = float(fx[f"s{s}.loss"])
        seen["loss"][f"s{s}.loss"] = abs(sum(x["loss"] for x in st) / world - ref_loss) / ref_loss
        for r, x in enumerate(st):
            pick = lambda ref, ncrop: torch.cat([ref[c * F27_B + r * b: c * F27_B + (r + 1) * b] for c in range(ncrop)])
            seen["logits"][f"s{s}.rank{r}.s_out"] = rel_l2(x["s_out"], pick(fx[f"s{s}.s_out"], 2 + F27_NLOCAL))
            seen["logits"][f"s{s}.rank{r}.t_out"] = rel_l2(x["t_out"], pick(fx[f"s{s}.t_out"], 2))
        post = sub(fx, f"s{s}.grad_post.")
        norms = dict(zip(names, fx[f"s{s}.norms"].tolist()))
        assert float(post[ZERO_SUM].double().norm()) < 1e-4 * float(post[ZERO_SUM_SCALE].double().norm())
        x = st[0]                                                            # (the all-reduced gradients: the SUM over the ranks)
        e_grad = {f"s{s}.{k}": rel_l2(x["grad"][k] / world * min(1.0, 3.0 / (norms[k] + 1e-6)), g) for k, g in post.items() if k != ZERO_SUM}
        seen["grad"].update(e_grad)
        e_bn = {f"s{s}.{who}.{k}": rel_l2(x[who][BN + k], fx[f"s{s}.{who}.{BN}{k}"]) for who in ("student", "teacher") for k in BN_BUFFERS[:2]}
        seen["bn"].update(e_bn)
        c_err = float((x["center"] - fx[f"s{s}.center"]).abs().max())
        checks.append((f"center, step {s}", c_err, 2e-3 * float(fx[f"s{s}.t_out"].abs().max())))
        checks.append((f"student num_batches_tracked, step {s}", abs(int(x["student"][BN + "num_batches_tracked"]) - 2 * (s + 1)), 0.5))
        checks.append((f"teacher num_batches_tracked, step {s}", abs(int(x["teacher"][BN + "num_batches_tracked"]) - (s + 1)), 0.5))
        for who in ("student", "teacher"):                                   # post-step parameters, as F16 measures them
            e = torch.cat([(x[who][k].double() - v.double()).abs().flatten() for k, v in sub(fx, f"s{s}.{who}.").items()
                           if k != ZERO_SUM and not k.endswith(BN_BUFFERS)]).numpy()
            step = lrs[s] if who == "student" else lrs[s] * (1 - moms[s]) * 2
            print(f"[F27 sync {tag} step {s}] post-step {who}: median |err| {np.median(e) / step:.3f} step, 90 % quantile "
                  f"{np.quantile(e, 0.9) / step:.3f} step, center |err| {c_err:.3e}")
            checks.append((f"post-step {who} median, step {s}", float(np.median(e)), 0.05 * step))
            checks.append((f"post-step {who} 90 % quantile, step {s}", float(np.quantile(e, 0.9)), 0.6 * step))
        print(f"[F27 sync {tag} step {s}] " + ", ".join(f"{g} {max(v for k, v in d.items() if k.startswith(f's{s}.')):.3e}" for g, d in seen.items()))
    print(f"[F27 sync {tag}] worst: " + ", ".join(f"{k} {max(v.values()):.3e}" for k, v in seen.items()))
    gate_errors(f"F27 sync {tag} loss (relative)", seen["loss"], GATE_LOSS)
    gate_errors(f"F27 sync {tag} logits", seen["logits"], GATE_LOGITS)
    gate_errors(f"F27 sync {tag} clipped gradients", seen["grad"], GATE_GRAD)
    gate_errors(f"F27 sync {tag} BatchNorm buffers", seen["bn"], GATE_BN)
    bad = [(n, v, lim) for n, v, lim in checks if not v < lim]
    assert not bad, bad


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
def test_two_ranks_against_the_f27_fixture_and_bit_equal_replicas(tmp_path, use_graph):
    out = str(tmp_path / "sync")
    mp.spawn(_worker, args=(2, _free_port(), out, use_graph), nprocs=2, join=True)
    outs = [torch.load(out + f".{r}", weights_only=False) for r in range(2)]
    if use_graph:
        assert outs[0]["n_graphs"] == outs[0]["n_segments"] and outs[0]["n_fwd"] == 2
    # the replicas: masters, center and every BatchNorm buffer of both networks, bit for bit
    a, b = outs
    assert torch.equal(a["masters"][0], b["masters"][0]) and torch.equal(a["masters"][1], b["masters"][1])
    for s in range(2):
        assert torch.equal(a["steps"][s]["center"], b["steps"][s]["center"])
        for who in ("student", "teacher"):
            for k in BN_BUFFERS:
                assert torch.equal(a["steps"][s][who][BN + k], b["steps"][s][who][BN + k]), (s, who, k)
    assert not torch.equal(a["steps"][0]["s_out"], b["steps"][0]["s_out"])              # (the ranks did see different rows)
    _against_f27(outs, "two ranks " + ("captured" if use_graph else "eager"))


def test_one_rank_takes_the_segmented_form_over_rccl(tmp_path):
    out = str(tmp_path / "sync1")
    mp.spawn(_rccl_worker, args=(1, _free_port(), out), nprocs=1, join=True)
    res = torch.load(out + ".0", weights_only=False)
    assert res["n_fwd"] == 2 and res["n_graphs"] == res["n_segments"] > 3
    _against_f27([res], "one rank, segmented")


def test_sync_bn_changes_nothing_where_it_does_not_apply():
    """One rank without LAFS_ONE_GRAPH=0: the plain kernels, one forward segment; without the switch a second rank is still refused
    (tests/test_gpu_step_fvit.py) and the message names the switch."""
    from lafs_cvpr2024_amd.engine import FVIT_MULTI_RANK
    if os.environ.get("LAFS_ONE_GRAPH", "1") != "0":
        _, _, _, eng = _build(F27_B, True)
        assert not eng.sync_bn and eng.n_fwd == 1 and eng.n_segments == len(eng.cuts) + 1
    assert "sync_bn" in FVIT_MULTI_RANK and "SyncBatchNorm" in FVIT_MULTI_RANK
