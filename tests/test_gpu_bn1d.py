"""lafs_bn1d_fwd / lafs_bn1d_bwd (csrc/unfold.hip: fViT's BatchNorm1d head) against fp64, element by element.  The bounds come from
the operation count of the kernel's formulas (tests/fvit_cases.py bn_*), never from what the kernel returns.  Two columns are planted:
column 0 is constant over the rows (variance 0, rstd = eps^-1/2) and column 1 has mean 1000 and spread 1e-2 -- a one-pass
E[x^2] - E[x]^2 in fp32 loses that variance entirely (1e6 * 2^-24 >> 1e-4)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_bounds as fb  # noqa: E402
from fvit_cases import bn_backward_bounds, bn_forward_reference  # noqa: E402
from lafs_cvpr2024_amd import _lib, ops  # noqa: E402

DEV = "cuda"
f32, f64 = torch.float32, torch.float64
EPS, MOM = 1e-5, 0.1
SHAPES = [(2, 64, 64), (4, 128, 128), (6, 128, 160), (37, 200, 200), (1024, 768, 768)]
_CACHE = {}


def inputs(n, D, ld):
    """fp32 inputs on the CPU, made once per shape and left unchanged (x is a [n, D] view of a [n, ld] buffer)."""
    key = (n, D, ld)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(n * 1000 + D)
        r = lambda *s: torch.randn(*s, generator=g)
        buf = torch.full((n, ld), float("nan"))
        x = r(n, D) * (0.5 + torch.rand(D, generator=g)) + r(D)
        x[:, 0] = 0.37
        x[:, 1] = 1000.0 + 1e-2 * r(n)
        buf[:, :D] = x
        _CACHE[key] = dict(buf=buf, gamma=1 + 0.1 * r(D), beta=0.1 * r(D), rm=0.1 * r(D), rv=1 + 0.2 * torch.rand(D, generator=g),
                           dy=r(n, D), old_dg=r(D), old_db=r(D))
    return _CACHE[key]


def run_fwd(c, D, training):
    buf = c["buf"].to(DEV)
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    y, mean, rstd = ops.bn1d_fwd(buf[:, :D], c["gamma"].to(DEV), c["beta"].to(DEV), EPS, MOM, training, rm, rv)
    return dict(y=y, save_mean=mean, save_rstd=rstd, running_mean=rm, running_var=rv), buf


def f32val(v):
    return float(torch.tensor(v, dtype=f32))            # the fp32 value the kernel receives for a Python float


@pytest.mark.parametrize("n,D,ld", SHAPES)
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_forward(n, D, ld, training):
    c = inputs(n, D, ld)
    got, _ = run_fwd(c, D, training)
    again, _ = run_fwd(c, D, training)
    ref = bn_forward_reference(c["buf"][:, :D].double(), c["gamma"].double(), c["beta"].double(), f32val(EPS), f32val(MOM),
                               c["rm"].double(), c["rv"].double(), training)
    for k, (v, e) in ref.items():
        fb.check(f"bn1d fwd {'train' if training else 'eval'} n{n} D{D} {k}", got[k].cpu(), v, e)
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f"{k}: two runs differ"
    if training:
        assert float(got["save_rstd"][0]) == pytest.approx(f32val(EPS) ** -0.5, rel=1e-6)      # the constant column
    else:                                                                                       # nothing updated: the same bits
        assert torch.equal(got["running_mean"].cpu(), c["rm"]) and torch.equal(got["running_var"].cpu(), c["rv"])


@pytest.mark.parametrize("n,D,ld", SHAPES)
@pytest.mark.parametrize("accumulate", [True, False], ids=["accumulate", "overwrite"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_backward(n, D, ld, accumulate, training):
    c = inputs(n, D, ld)
    fwd, buf = run_fwd(c, D, training)
    x = buf[:, :D]

    def run():
        dg, db = c["old_dg"].to(DEV), c["old_db"].to(DEV)
        dx = ops.bn1d_bwd(c["dy"].to(DEV), x, fwd["save_mean"], fwd["save_rstd"], c["gamma"].to(DEV), training, dg, db, accumulate=accumulate)
        return dict(dx=dx.cpu(), dgamma=dg.cpu(), dbeta=db.cpu())
    got, again = run(), run()
    # the reference: fp64 autograd of nn.BatchNorm1d on the CPU
    bn = torch.nn.BatchNorm1d(D, eps=f32val(EPS), momentum=f32val(MOM)).double()
    with torch.no_grad():
        bn.weight.copy_(c["gamma"]); bn.bias.copy_(c["beta"]); bn.running_mean.copy_(c["rm"]); bn.running_var.copy_(c["rv"])
    bn.train(training)
    xd = c["buf"][:, :D].double().requires_grad_(True)
    (bn(xd) * c["dy"].double()).sum().backward()
    old = (c["old_dg"].double(), c["old_db"].double()) if accumulate else (None, None)
    bounds = bn_backward_bounds(c["dy"].double(), xd.detach(), c["gamma"].double(), f32val(EPS), c["rm"].double(), c["rv"].double(),
                                training, *old)
    ref = dict(dx=xd.grad, dgamma=bn.weight.grad + (old[0] if accumulate else 0), dbeta=bn.bias.grad + (old[1] if accumulate else 0))
    for k in ("dx", "dgamma", "dbeta"):
        closed, e = bounds[k]
        assert bool(((closed - ref[k]).abs() <= 1e-9 * (1 + ref[k].abs()) + 1e-3 * e).all()), f"{k}: the closed form and autograd disagree"
        fb.check(f"bn1d bwd {'train' if training else 'eval'} n{n} D{D} {k}", got[k], ref[k], e)
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f"{k}: two runs differ"


def test_one_row_in_training_is_an_error():
    x = torch.randn(1, 64, device=DEV)
    one, zero = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    with pytest.raises(_lib.LafsHipError):
        ops.bn1d_fwd(x, one, zero, EPS, MOM, True, zero.clone(), one.clone())
    y, _, _ = ops.bn1d_fwd(x, one, zero, EPS, MOM, False, zero.clone(), one.clone())       # eval takes a single row
    assert bool(torch.isfinite(y).all())
