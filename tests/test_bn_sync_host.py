"""CPU: the cross-rank BatchNorm of the fViT head (lafs_train.py --sync_bn, the reference's SyncBatchNorm conversion :362-364).
(a) The pure-torch statements of the four kernels in lafs_cvpr2024_amd/distributed.py, run by two gloo ranks on CPU tensors through
    BnStatExchange, against nn.BatchNorm1d in fp64 on the concatenated rows: y, the running buffers (unbiased variance of the TOTAL
    count) and dx / dgamma / dbeta from autograd of the sum of the ranks' losses.
(b) The fp64 bounds of tests/bn_sync_cases.py: an fp32 emulation of the kernels' arithmetic stays inside them, seeded faults do not.
(c) --sync_bn parses; without it the multi-rank refusal still fires before a backbone is built."""
import datetime
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(__file__))

import bn_sync_cases as bc  # noqa: E402
import fp64_bounds as fb  # noqa: E402
from lafs_cvpr2024_amd import distributed as D_  # noqa: E402
from lafs_cvpr2024_amd import lafs_train as L, utils  # noqa: E402
from lafs_cvpr2024_amd.engine import FVIT_MULTI_RANK  # noqa: E402

f64 = torch.float64
TABLES = [(2, 3), (4, 1)]            # rank 0 / rank 1 rows per group; group 1 has ONE row on rank 1
DIM = 12


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _data():
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=f64)
    xs = [r(sum(t), DIM) * 2 + 0.7 * k + r(DIM) for k, t in enumerate(TABLES)]
    ws = [r(sum(t), DIM) for t in TABLES]                                    # loss of a rank = sum(y * w): dy = w
    return xs, ws, 1 + 0.1 * r(DIM), 0.1 * r(DIM), 0.1 * r(DIM), 1 + 0.2 * torch.rand(DIM, generator=g, dtype=f64)


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    xs, ws, gamma, beta, rm, rv = _data()
    x, dy, rows = xs[rank], ws[rank], bc.rows_of(TABLES[rank])
    G = len(rows) - 1
    red = D_.FlatReducer()
    ex = D_.BnStatExchange([G, 1], DIM, "cpu", red, dtype=f64)             # (a second network's slot rides along, as the teacher's does)
    ex.clear()
    ex.slot(0).copy_(D_.bn_partial_stats(x, rows))
    ex.slot(1).copy_(D_.bn_partial_stats(x, [0, x.shape[0]]))
    red.wait([ex.gather()])
    y, mean, rstd, rm2, rv2 = D_.bn_sync_forward(x, rows, ex.all(0), gamma, beta, 1e-5, 0.1, rm, rv)
    totals = [sum(t[g] for t in TABLES) for g in range(G)]
    n_all, _, _ = D_.bn_combine_partials(ex.all(1))
    ex.sums.copy_(D_.bn_backward_sums(dy, x, rows, mean, rstd))
    local = ex.sums.clone()                                                  # dgamma / dbeta stay rank-local sums
    red.wait([ex.reduce_sums()])
    dx = D_.bn_sync_backward(dy, x, rows, totals, mean, rstd, gamma, ex.sums)
    torch.save(dict(y=y, rm=rm2, rv=rv2, dx=dx, dbeta=local[:, :DIM].sum(0), dgamma=local[:, DIM:].sum(0), n_all=n_all, mean=mean), out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_equal_batchnorm1d_on_the_concatenated_rows(tmp_path):
    out = str(tmp_path / "bn")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = [torch.load(out + f".{r}", weights_only=False) for r in range(2)]
    xs, ws, gamma, beta, rm, rv = _data()
    bn = torch.nn.BatchNorm1d(DIM, eps=1e-5, momentum=0.1).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    leaves = [x.clone().requires_grad_(True) for x in xs]
    loss, ys = 0, [[], []]
    for g in range(len(TABLES[0])):                                          # the head runs once per group, in order
        sl = [(bc.rows_of(t)[g], bc.rows_of(t)[g + 1]) for t in TABLES]
        y = bn(torch.cat([lf[a:b] for lf, (a, b) in zip(leaves, sl)]))
        at = 0
        for r, (a, b) in enumerate(sl):
            ys[r].append(y[at: at + b - a]); loss = loss + (y[at: at + b - a] * ws[r][a:b]).sum(); at += b - a
    loss.backward()
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-12)
    for r in range(2):
        close(got[r]["y"], torch.cat(ys[r]).detach())
        close(got[r]["dx"], leaves[r].grad)
        close(got[r]["rm"], bn.running_mean); close(got[r]["rv"], bn.running_var)
        assert got[r]["n_all"].flatten().tolist() == [float(sum(map(sum, TABLES)))]
    close(got[0]["dgamma"] + got[1]["dgamma"], bn.weight.grad)
    close(got[0]["dbeta"] + got[1]["dbeta"], bn.bias.grad)
    for k in ("rm", "rv", "mean"):                                           # every rank folds the same partials in the same order
        assert torch.equal(got[0][k], got[1][k]), k


CASES = [(name, D) for name in bc.RANK_TABLES for D in ((64, 200) if name != "w8_16x64" else (64,))]


def _failing(c, got, fwd, bwd):
    """The names of the outputs that leave their bounds."""
    tag, bad = "bn sync emulation", set()

    def chk(name, k, *a):
        try:
            fb.check(name, *a)
        except AssertionError:
            bad.add(k)
    for rk in range(len(c["tables"])):
        chk(f"{tag} rank {rk} y", "y", got["y"][rk], *fwd["y"][rk])
        chk(f"{tag} rank {rk} dx", "dx", got["dx"][rk], *bwd[rk])
    for k in ("save_mean", "save_rstd", "running_mean", "running_var"):
        chk(f"{tag} {k}", k, got[k], *fwd[k])
    return bad


@pytest.mark.parametrize("name,D", CASES)
def test_fp32_emulation_lies_inside_the_bounds_and_seeded_faults_do_not(name, D):
    c = bc.inputs(name, D)
    eps, mom = bc.f32val(bc.EPS), bc.f32val(bc.MOM)
    fwd = bc.sync_forward_reference(c, eps, mom)
    bwd = bc.sync_backward_bounds(c, eps, fwd["stats"])
    assert _failing(c, bc.emulate(c, eps, mom), fwd, bwd) == set()
    # the oracle is the statistic of the concatenated rows: nn.BatchNorm1d on them agrees with it
    X = torch.cat([x for x, _ in bc.group_slices(c, 0)]).double()
    torch.testing.assert_close(fwd["save_mean"][0][0], X.mean(0), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(fwd["save_rstd"][0][0], (X.var(0, unbiased=False) + eps) ** -0.5, rtol=1e-9, atol=0)
    # each fault leaves exactly the outputs it can reach: the biased variance only the running buffer, the per-rank count only dx
    assert _failing(c, bc.emulate(c, eps, mom, fault="biased_running_var"), fwd, bwd) == {"running_var"}
    assert {"save_rstd", "y", "dx", "running_var"} <= _failing(c, bc.emulate(c, eps, mom, fault="no_delta_term"), fwd, bwd)
    assert _failing(c, bc.emulate(c, eps, mom, fault="rank_count"), fwd, bwd) == {"dx"}


def test_the_bounds_mean_something():
    """Relative width of the bounds on ordinary columns: a few ulp for the statistics, some tens for y / dx of 8 x 64 rows."""
    c = bc.inputs("w8_16x64", 64)
    eps = bc.f32val(bc.EPS)
    fwd = bc.sync_forward_reference(c, eps, bc.f32val(bc.MOM))
    v, e = fwd["save_rstd"]
    assert float((e / v)[:, 3:].max()) < 2e-4                                # 640 rows: n u sum|terms| worst case, still 4 digits
    v, e = fwd["save_mean"]
    assert float((e[:, 3:] / (v[:, 3:].abs() + 1)).max()) < 2e-4


def test_sync_bn_flag_parses():
    assert L.get_args_parser().parse_args([]).sync_bn is False
    assert L.get_args_parser().parse_args("--arch fvit --sync_bn true".split()).sync_bn is True
    assert L.get_args_parser().parse_args("--sync_bn false".split()).sync_bn is False


def test_multi_rank_fvit_without_the_flag_is_still_refused_before_anything_is_built(monkeypatch):
    monkeypatch.setattr(utils, "init_distributed_mode", lambda args: setattr(args, "gpu", 0))
    monkeypatch.setattr(utils, "get_world_size", lambda: 2)
    monkeypatch.setattr(L, "build_backbones", lambda args: pytest.fail("a backbone was built"))
    for argv in ("--arch fvit --fvit_dims 64,2,2,128", "--arch fvit --fvit_dims 64,2,2,128 --sync_bn false"):
        with pytest.raises(SystemExit) as e:
            L.train_lafs(L.get_args_parser().parse_args(argv.split()))
        assert e.value.code == FVIT_MULTI_RANK and "SyncBatchNorm" in FVIT_MULTI_RANK and "sync_bn" in FVIT_MULTI_RANK


def test_multi_rank_fvit_with_the_flag_gets_past_the_refusal(monkeypatch):
    class Built(Exception):
        pass

    def built(args):
        raise Built
    monkeypatch.setattr(utils, "init_distributed_mode", lambda args: setattr(args, "gpu", 0))
    monkeypatch.setattr(utils, "get_world_size", lambda: 2)
    monkeypatch.setattr(L, "build_backbones", built)
    with pytest.raises(Built):
        L.train_lafs(L.get_args_parser().parse_args("--arch fvit --fvit_dims 64,2,2,128 --sync_bn true".split()))
