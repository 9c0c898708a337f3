"""lafs_trunk_forward / lafs_trunk_backward with lafs_trunk_desc::cls_only_last (the last block behind its qkv GEMM on the cls rows
only, csrc/engine.hip) against the dense passes on identical inputs, and both against the CPU oracle (oracle/vit.py, fp64).

Depth 2; groups of 2 x 197 and 3 x 37 tokens; widths 128 / 512 (the dense block's MLP as two GEMMs) and 384 / 1536 (one fused
launch in the dense block); the last block's DropPath scales hold a zero and a non-unit value in both branches.  Compared: the cls rows
of x_out, the whole input gradient, every weight / bias / LayerNorm gradient of both blocks -- per tensor, relative L2, under the
composition test's gate (gate_errors, 2e-2).  Both runs' errors are printed side by side: the pruned run sums fewer rounded terms (its
fc2 / fc1 / proj weight gradients add n_seq rows, not n_tok rows of which all but n_seq are zero) and is expected to be no worse.

The two GPU runs against each other are held to 2^-8 = 3.9e-3 relative L2 per tensor, one bf16 rounding unit.  Reasoning: the cls kernels
round where the dense ones do, so the two runs differ first by the order of fp32 sums (relative d0 <= acc_factor(256) u = 4e-6).  A
tensor that is then rounded to bf16 turns a relative perturbation d into flips of a share d / 2^-8 of its elements by 2^-8 each, i.e.
sqrt(d 2^-8) in relative L2: 1.2e-4 after the first bf16 tensor (o, dqkv), 6.9e-4 after the second (h2 / dh of the next block), 1.6e-3
after the third -- approaching, never passing, the 2^-8 of independent roundings.  Sums over rows (weight gradients) average it
down.  That is 5x inside the oracle gate and still far below what a wrong row -> sequence mapping of the DropPath scales does (a
scale of 1.25 for 1: 0.2).  Observed: 1e-8 .. 8e-7 on the 505-row case (hardly any flip), 0 and 1.6e-6 on the two-chain forward-only
pass, 3.6e-4 (width 128) and 7.9e-4 (width 384) on the two-chain backward at depth 3, worst in the middle block's norm1.weight.

Two row chains (two crop groups of >= 4096 rows each, the context's side streams; depth 3): the saving pass with its backward, and the
forward-only pass -- where all blocks of all chains share ONE buffer set and a chain reaches the last block while another still runs
an earlier one -- each with the flag on against the flag off under the same gate."""
import ctypes as C
from functools import partial

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from conftest import gate_errors  # noqa: E402
from lafs_cvpr2024_amd import _lib, functional as Fn  # noqa: E402
from lafs_cvpr2024_amd.ops import _p, call  # noqa: E402
from lafs_cvpr2024_amd.vision_transformer import VisionTransformer, attach_arena  # noqa: E402

DEV = "cuda"
GROUPS = [(2, 112), (3, 48)]            # 2 x 197 + 3 x 37 = 505 token rows, 5 sequences
GATE = 2e-2
PAIR_GATE = 2.0 ** -8                   # flag on against flag off: one bf16 rounding unit (see the module text)
CHAIN_GROUPS = [(21, 112), (112, 48)]   # 21 x 197 = 4137 and 112 x 37 = 4144 token rows: one row chain per group
WIDTHS = {"w128": (128, 2, 512), "w384": (384, 6, 1536)}


def _model(dim, heads, mlp, depth=2):
    torch.manual_seed(1234 + dim)
    vit = VisionTransformer(img_size=[112], patch_size=8, embed_dim=dim, depth=depth, num_heads=heads, mlp_ratio=mlp / dim, qkv_bias=True,
                            norm_layer=partial(nn.LayerNorm, eps=1e-6))
    with torch.no_grad():
        for name, p in vit.named_parameters():
            if not name.startswith("blocks."):
                continue
            if "norm" in name:
                p.add_(0.1 * torch.randn_like(p))
            elif name.endswith(".bias"):
                p.copy_(0.05 * torch.randn_like(p))
            else:
                p.mul_(3.0)                 # std 0.06: both residual branches carry weight against the stream
    return vit


def _inputs(dim):
    g = torch.Generator().manual_seed(77 + dim)
    lens = [197, 197, 37, 37, 37]
    x = torch.randn(sum(lens), dim, generator=g)
    gcls = torch.randn(len(lens), dim, generator=g)
    keep = 0.8
    drop = torch.ones(2, 2, len(lens))
    drop[0] = torch.tensor([[1 / keep, 1, 1 / keep, 1 / keep, 1], [1, 1 / keep, 1 / keep, 1, 1 / keep]])
    drop[1] = torch.tensor([[0.0, 1 / keep, 1, 1 / keep, 0.0], [1 / keep, 0.0, 1 / keep, 1, 1 / keep]])      # a zero and a non-unit value per branch
    return lens, x, gcls, drop


def _oracle(vit, lens, x, gcls, drop):
    """fp64 autograd through oracle.vit.block: cls rows of the output, dL/dx_in and every block gradient for L = sum(cls rows * gcls)."""
    from oracle import vit as ovit
    dim, heads = vit.embed_dim, vit.num_heads
    cfg = ovit.ViTConfig(patch_size=8, embed_dim=dim, depth=2, num_heads=heads, mlp_ratio=vit.blocks[0].mlp.fc1.out_features / dim, img_size=112)
    P = {k: v.detach().cpu().double().requires_grad_(True) for k, v in vit.named_parameters() if k.startswith("blocks.")}
    xin = x.double().requires_grad_(True)
    outs, row, seq = [], 0, 0
    while seq < len(lens):
        n = lens[seq]
        cnt = sum(1 for v in lens if v == n)
        t = xin[row:row + cnt * n].view(cnt, n, dim)
        for i in range(2):
            t = ovit.block(P, i, t, cfg, drop[i, 0, seq:seq + cnt].double(), drop[i, 1, seq:seq + cnt].double())
        outs.append(t[:, 0])
        row, seq = row + cnt * n, seq + cnt
    cls = torch.cat(outs)
    (cls * gcls.double()).sum().backward()
    return cls.detach(), xin.grad, {k: v.grad for k, v in P.items()}


_RUNS = {}


def _run(width):
    """The oracle once and the two GPU runs (flag off, flag on) of one width; shared by the tests."""
    if width in _RUNS:
        return _RUNS[width]
    dim, heads, mlp = WIDTHS[width]
    lens, x, gcls, drop = _inputs(dim)
    res = {}
    for flag in (0, 1):
        vit = _model(dim, heads, mlp)
        if flag == 0:
            res["oracle"] = _oracle(vit, lens, x, gcls, drop)
        arena = attach_arena(vit, torch.device(DEV, torch.cuda.current_device()))
        geom = Fn.geometry(GROUPS, arena.device)
        assert geom.n_tok == sum(lens) and geom.n_seq == len(lens)
        drop_d = drop.to(DEV).contiguous()
        desc = Fn.make_trunk_desc(arena, vit._spec.trunk, geom, drop_d, with_grad=True, cls_only_last=bool(flag))
        plan = _lib.TrunkPlanInfo()
        assert _lib.lib().lafs_trunk_plan(C.byref(desc), 1, C.byref(plan)) == 0
        assert plan.cls_only_last == flag and plan.whole.fwd_fused == plan.whole.bwd_fused == (1 if dim == 384 else 0), \
            (flag, plan.cls_only_last, plan.whole.fwd_fused, plan.whole.bwd_fused)
        ws = Fn.trunk_workspace(desc, True, DEV)
        x_in = x.to(DEV).contiguous()
        x_out = torch.full((geom.n_tok, dim), float("nan"), device=DEV)
        call("lafs_trunk_forward", C.byref(desc), _p(x_in), _p(x_out), _p(ws), 1)
        cls_rows = geom.cu_seqlens[:-1].long()
        g = torch.zeros(geom.n_tok, dim, device=DEV)
        g[cls_rows] = gcls.to(DEV)
        arena.zero_grad()
        call("lafs_trunk_backward", C.byref(desc), _p(x_in), _p(g), _p(ws), 2, 0, None)
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().cpu().clone() for k, p in vit.named_parameters() if k.startswith("blocks.")}
        res[flag] = (x_out[cls_rows].cpu(), g.cpu(), grads, x_in.cpu())
    _RUNS[width] = res
    return res


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _errors(run, oracle):
    cls, dx, grads, _ = run
    o_cls, o_dx, o_grads = oracle
    errs = {"x_out[cls]": _rel(cls, o_cls), "dx_in": _rel(dx, o_dx)}
    for k, v in o_grads.items():
        errs["d " + k] = _rel(grads[k], v)
    return errs


@pytest.mark.parametrize("width", list(WIDTHS))
def test_both_runs_against_the_oracle(width):
    r = _run(width)
    e0, e1 = _errors(r[0], r["oracle"]), _errors(r[1], r["oracle"])
    assert len(e0) == 2 + 2 * 12
    print(f"[trunk cls-last {width}] rel-L2 against the fp64 oracle: dense | cls rows only")
    for k in e0:
        print(f"  {k:34s} {e0[k]:.3e} | {e1[k]:.3e}")
    last = [k for k in e0 if "blocks.1." in k and any(s in k for s in ("mlp.", "proj.", "norm2."))]
    print(f"[trunk cls-last {width}] tensors of the pruned launches where the pruned run is the worse one: "
          f"{[k for k in last if e1[k] > e0[k]]} of {len(last)}")
    gate_errors(f"trunk {width}, dense last block", e0, GATE)
    gate_errors(f"trunk {width}, last block on the cls rows", e1, GATE)


@pytest.mark.parametrize("width", list(WIDTHS))
def test_flag_on_against_flag_off(width):
    """The two GPU runs against each other, per tensor: each lies within its gate of the oracle, so they lie within the two gates'
    sum of each other (relative to the dense run's norm) -- and the inputs were identical and untouched."""
    r = _run(width)
    (cls0, dx0, g0, xin0), (cls1, dx1, g1, xin1) = r[0], r[1]
    assert torch.equal(xin0, xin1) and not bool(torch.isnan(cls1).any()) and not bool(torch.isnan(dx1).any())
    errs = {"x_out[cls]": _rel(cls1, cls0), "dx_in": _rel(dx1, dx0)}
    for k in g0:
        errs["d " + k] = _rel(g1[k], g0[k])
    k = max(errs, key=errs.get)
    print(f"[trunk cls-last {width}] flag on against flag off: worst rel-L2 {errs[k]:.3e} at {k}")
    gate_errors(f"trunk {width}, flag on against flag off", errs, PAIR_GATE)


def _chain_pass(dim, heads, mlp, flag, save):
    """One pass over the two-chain geometry, depth 3: (cls rows of x_out, dL/dx_in or None, block gradients or None)."""
    depth = 3
    vit = _model(dim, heads, mlp, depth)
    arena = attach_arena(vit, torch.device(DEV, torch.cuda.current_device()))
    geom = Fn.geometry(CHAIN_GROUPS, arena.device)
    g = torch.Generator().manual_seed(5 + dim)
    x_in = torch.randn(geom.n_tok, dim, generator=g).to(DEV)
    gcls = torch.randn(geom.n_seq, dim, generator=g).to(DEV)
    # DropPath scales 0 | 1 | 1.25 per (block, branch, sequence): zeros and non-unit values in the last block of both chains
    drop = (torch.randint(0, 3, (depth, 2, geom.n_seq), generator=g).float() * 0.625).clamp_max(1.25)
    drop = torch.where(drop == 0.625, torch.ones(()), drop).to(DEV).contiguous()
    desc = Fn.make_trunk_desc(arena, vit._spec.trunk, geom, drop, with_grad=bool(save), cls_only_last=bool(flag))
    plan = _lib.TrunkPlanInfo()
    assert _lib.lib().lafs_trunk_plan(C.byref(desc), save, C.byref(plan)) == 0
    assert plan.cls_only_last == flag and plan.n_ranges == 2 and [plan.range[i].rows for i in range(2)] == [4137, 4144], \
        (plan.cls_only_last, plan.n_ranges)
    ws = Fn.trunk_workspace(desc, bool(save), DEV)
    ws.fill_(0x7f)                       # (stale workspace contents must not matter: 3.4e38 in every bf16 and f32)
    x_out = torch.full((geom.n_tok, dim), float("nan"), device=DEV)
    call("lafs_trunk_forward", C.byref(desc), _p(x_in), _p(x_out), _p(ws), save)
    cls_rows = geom.cu_seqlens[:-1].long()
    out = x_out[cls_rows].cpu()
    if not save:
        torch.cuda.synchronize()
        return out, None, None
    gr = torch.zeros(geom.n_tok, dim, device=DEV)
    gr[cls_rows] = gcls
    arena.zero_grad()
    call("lafs_trunk_backward", C.byref(desc), _p(x_in), _p(gr), _p(ws), depth, 0, None)
    torch.cuda.synchronize()
    return out, gr.cpu(), {k: p.grad.detach().cpu().clone() for k, p in vit.named_parameters() if k.startswith("blocks.")}


@pytest.mark.parametrize("save", [1, 0], ids=["saving+backward", "forward-only"])
@pytest.mark.parametrize("width", list(WIDTHS))
def test_two_row_chains_flag_on_against_flag_off(width, save):
    dim, heads, mlp = WIDTHS[width]
    (cls0, dx0, g0), (cls1, dx1, g1) = _chain_pass(dim, heads, mlp, 0, save), _chain_pass(dim, heads, mlp, 1, save)
    assert not bool(torch.isnan(cls0).any()) and not bool(torch.isnan(cls1).any())
    errs = {"x_out[cls]": _rel(cls1, cls0)}
    if save:
        errs["dx_in"] = _rel(dx1, dx0)
        errs.update({"d " + k: _rel(g1[k], g0[k]) for k in g0})
        assert len(errs) == 2 + 3 * 12 and not bool(torch.isnan(dx1).any())
    gate_errors(f"trunk {width}, two chains, {'saving pass + backward' if save else 'forward-only pass'}: flag on against flag off", errs, PAIR_GATE)
