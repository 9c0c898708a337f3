"""lafs_bn1d_groups_fwd / lafs_bn1d_groups_bwd (csrc/unfold.hip: fViT's BatchNorm1d head over the crop groups of one packed pass).

Two yardsticks.  (a) fp64, element by element, per group: y, save_mean, save_rstd and dx inside the operation-count bounds of
tests/fvit_cases.py (bn_forward_reference / bn_backward_bounds), which never look at what the kernel returns.  (b) the chain of
single-group ops.bn1d_fwd / ops.bn1d_bwd calls on the row ranges in group order, bit for bit, for EVERY output -- the running buffers
(updated once per group, group 0 first) and dgamma / dbeta (summed in group order) included; those kernels are held to fp64 by
tests/test_gpu_bn1d.py.  The planted columns are that file's: column 0 constant over the rows, column 1 mean 1000 with spread 1e-2.
x, y, dy and dx are [n, D] views of NaN-filled [n + 3, ld] buffers: the ld padding and the rows behind the last group must stay NaN."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_bounds as fb  # noqa: E402
from fvit_cases import bn_backward_bounds, bn_forward_reference  # noqa: E402
from lafs_cvpr2024_amd import _lib, ops  # noqa: E402

DEV = "cuda"
f32, f64 = torch.float32, torch.float64
EPS, MOM = 1e-5, 0.1
TABLES = [(2,), (2, 3), (4, 6), (2, 2, 2), (128, 512)]
DIMS = [(64, 64), (200, 232), (768, 768)]
GUARD = 3                               # NaN rows behind the last group
_CACHE = {}


def rows_of(table):
    out = [0]
    for n in table:
        out.append(out[-1] + n)
    return out


def f32val(v):
    return float(torch.tensor(v, dtype=f32))


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def inputs(table, D, ld):
    """fp32 inputs on the CPU, made once per case and left unchanged."""
    key = (table, D, ld)
    if key not in _CACHE:
        n = sum(table)
        g = torch.Generator().manual_seed(n * 1000 + D + len(table))
        r = lambda *s: torch.randn(*s, generator=g)
        x = r(n, D) * (0.5 + torch.rand(D, generator=g)) + r(D)
        for a, b in zip(rows_of(table)[:-1], rows_of(table)[1:]):           # every group has a level and a spread of its own
            x[a:b] = x[a:b] * (0.5 + torch.rand(1, generator=g)) + r(D)
        x[:, 0] = 0.37
        x[:, 1] = 1000.0 + 1e-2 * r(n)
        _CACHE[key] = dict(x=x, gamma=1 + 0.1 * r(D), beta=0.1 * r(D), rm=0.1 * r(D), rv=1 + 0.2 * torch.rand(D, generator=g),
                           dy=r(n, D), old_dg=r(D), old_db=r(D))
    return _CACHE[key]


def padded(t, ld):
    """t [n, D] on the device as a view of a NaN-filled [n + GUARD, ld] buffer.  Returns (view, buffer)."""
    n, D = t.shape
    buf = torch.full((n + GUARD, ld), float("nan"), device=DEV)
    buf[:n, :D] = t.to(DEV)
    return buf[:n, :D], buf


def nan_view(n, D, ld):
    buf = torch.full((n + GUARD, ld), float("nan"), device=DEV)
    return buf[:n, :D], buf


def guards_untouched(buf, n, D):
    return bool(torch.isnan(buf[n:]).all()) and bool(torch.isnan(buf[:, D:]).all())


def grouped_fwd(c, table, D, ld, training):
    x, xbuf = padded(c["x"], ld)
    y, ybuf = nan_view(sum(table), D, ld)
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    _, mean, rstd = ops.bn1d_groups_fwd(x, rows_of(table), c["gamma"].to(DEV), c["beta"].to(DEV), EPS, MOM, training, rm, rv, out=y)
    return dict(y=y, save_mean=mean, save_rstd=rstd, running_mean=rm, running_var=rv), x, (xbuf, ybuf)


def chained_fwd(c, table, D, ld, training):
    x, _ = padded(c["x"], ld)
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    ys, means, rstds = [], [], []
    for a, b in zip(rows_of(table)[:-1], rows_of(table)[1:]):
        y, m, r = ops.bn1d_fwd(x[a:b], c["gamma"].to(DEV), c["beta"].to(DEV), EPS, MOM, training, rm, rv)
        ys.append(y); means.append(m); rstds.append(r)
    return dict(y=torch.cat(ys), save_mean=torch.stack(means), save_rstd=torch.stack(rstds), running_mean=rm, running_var=rv)


@pytest.mark.parametrize("D,ld", DIMS)
@pytest.mark.parametrize("table", TABLES, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_forward(table, D, ld, training):
    c = inputs(table, D, ld)
    n = sum(table)
    got, _, (xbuf, ybuf) = grouped_fwd(c, table, D, ld, training)
    again, _, _ = grouped_fwd(c, table, D, ld, training)
    chain = chained_fwd(c, table, D, ld, training)
    tag = f"bn1d groups fwd {'train' if training else 'eval'} {table} D{D}"
    # (a) fp64 per group (the running buffers do not enter y / save_* in training; in eval they are constants)
    for g, (a, b) in enumerate(zip(rows_of(table)[:-1], rows_of(table)[1:])):
        ref = bn_forward_reference(c["x"][a:b].double(), c["gamma"].double(), c["beta"].double(), f32val(EPS), f32val(MOM),
                                   c["rm"].double(), c["rv"].double(), training)
        fb.check(f"{tag} group {g} y", got["y"][a:b].cpu(), *ref["y"])
        fb.check(f"{tag} group {g} save_mean", got["save_mean"][g].cpu(), *ref["save_mean"])
        fb.check(f"{tag} group {g} save_rstd", got["save_rstd"][g].cpu(), *ref["save_rstd"])
        if training:
            assert float(got["save_rstd"][g, 0]) == pytest.approx(f32val(EPS) ** -0.5, rel=1e-6)      # the constant column
    # (b) the chain of single-group launches, (c) a second run: bit for bit
    for k in ("y", "save_mean", "save_rstd", "running_mean", "running_var"):
        assert torch.equal(bits(got[k]), bits(chain[k])), f"{k}: differs from the chain of single-group launches"
        assert torch.equal(bits(got[k]), bits(again[k])), f"{k}: two runs differ"
    if training:
        assert not torch.equal(bits(got["running_mean"]), bits(c["rm"]))
    else:
        assert torch.equal(got["running_mean"].cpu(), c["rm"]) and torch.equal(got["running_var"].cpu(), c["rv"])
    # (d) padding columns and the rows behind the last group
    assert guards_untouched(ybuf, n, D) and guards_untouched(xbuf, n, D)
    assert bool(torch.isfinite(ybuf[:n, :D]).all())


@pytest.mark.parametrize("D,ld", DIMS)
@pytest.mark.parametrize("table", TABLES, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("accumulate", [True, False], ids=["accumulate", "overwrite"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_backward(table, D, ld, accumulate, training):
    c = inputs(table, D, ld)
    n, rows = sum(table), rows_of(table)
    fwd, x, _ = grouped_fwd(c, table, D, ld, training)
    gamma = c["gamma"].to(DEV)

    def run():
        dy, _ = padded(c["dy"], ld)
        dx, dxbuf = nan_view(n, D, ld)
        dg, db = c["old_dg"].to(DEV), c["old_db"].to(DEV)
        ops.bn1d_groups_bwd(dy, x, rows, fwd["save_mean"], fwd["save_rstd"], gamma, training, dg, db, accumulate=accumulate, out=dx)
        return dict(dx=dx, dgamma=dg, dbeta=db), dxbuf
    got, dxbuf = run()
    again, _ = run()
    # the chain: group 0 overwrites when accumulate == 0, every later group adds
    dy, _ = padded(c["dy"], ld)
    dg, db = c["old_dg"].to(DEV), c["old_db"].to(DEV)
    dxs = []
    for g, (a, b) in enumerate(zip(rows[:-1], rows[1:])):
        dxs.append(ops.bn1d_bwd(dy[a:b], x[a:b], fwd["save_mean"][g], fwd["save_rstd"][g], gamma, training, dg, db,
                                accumulate=accumulate or g > 0))
    chain = dict(dx=torch.cat(dxs), dgamma=dg, dbeta=db)
    tag = f"bn1d groups bwd {'train' if training else 'eval'} {table} D{D}"
    for g, (a, b) in enumerate(zip(rows[:-1], rows[1:])):                   # (a)
        bounds = bn_backward_bounds(c["dy"][a:b].double(), c["x"][a:b].double(), c["gamma"].double(), f32val(EPS), c["rm"].double(),
                                    c["rv"].double(), training)
        fb.check(f"{tag} group {g} dx", got["dx"][a:b].cpu(), *bounds["dx"])
    for k in ("dx", "dgamma", "dbeta"):                                      # (b), (c)
        assert torch.equal(bits(got[k]), bits(chain[k])), f"{k}: differs from the chain of single-group launches"
        assert torch.equal(bits(got[k]), bits(again[k])), f"{k}: two runs differ"
    assert guards_untouched(dxbuf, n, D) and bool(torch.isfinite(dxbuf[:n, :D]).all())      # (d)


# ------------------------------------------------------------------------------------------------ (e) refusals
def _table(rows):
    return None if rows is None else (C.c_int * len(rows))(*rows)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _fwd_args(n=5, D=64, ld=64):
    t = dict(x=torch.randn(n, ld, device=DEV), gamma=torch.ones(D, device=DEV), beta=torch.zeros(D, device=DEV),
             rm=torch.zeros(D, device=DEV), rv=torch.ones(D, device=DEV), y=torch.full((n, ld), float("nan"), device=DEV),
             mean=torch.full((8, D), float("nan"), device=DEV), rstd=torch.full((8, D), float("nan"), device=DEV))
    return t, dict(rows=[0, 2, 5], G=2, D=D, ldx=ld, ldy=ld, training=1)


def _call_fwd(t, a):
    _lib.call("lafs_bn1d_groups_fwd", _p(t["x"]), a["ldx"], _table(a["rows"]), a["G"], a["D"], _p(t["gamma"]), _p(t["beta"]), EPS, MOM,
              a["training"], _p(t["rm"]), _p(t["rv"]), _p(t["y"]), a["ldy"], _p(t["mean"]), _p(t["rstd"]))


def _bwd_args(n=5, D=64, ld=64):
    t = dict(dy=torch.randn(n, ld, device=DEV), x=torch.randn(n, ld, device=DEV), mean=torch.zeros(8, D, device=DEV),
             rstd=torch.ones(8, D, device=DEV), gamma=torch.ones(D, device=DEV), dx=torch.full((n, ld), float("nan"), device=DEV),
             dg=torch.full((D,), float("nan"), device=DEV), db=torch.full((D,), float("nan"), device=DEV))
    return t, dict(rows=[0, 2, 5], G=2, D=D, lddy=ld, ldx=ld, lddx=ld, training=1)


def _call_bwd(t, a):
    _lib.call("lafs_bn1d_groups_bwd", _p(t["dy"]), a["lddy"], _p(t["x"]), a["ldx"], _table(a["rows"]), a["G"], a["D"], _p(t["mean"]),
              _p(t["rstd"]), _p(t["gamma"]), a["training"], _p(t["dx"]), a["lddx"], _p(t["dg"]), _p(t["db"]), 0)


BAD_TABLES = [dict(rows=None), dict(G=0), dict(G=9, rows=[0, 2, 4, 6, 8, 10, 12, 14, 16, 18]), dict(rows=[0, 3, 3]), dict(rows=[0, 4, 2]),
              dict(rows=[1, 3, 5]), dict(rows=[0, 1, 5]), dict(D=2112)]


@pytest.mark.parametrize("bad", BAD_TABLES + [dict(ldx=63), dict(ldy=63), dict(null="x"), dict(null="gamma"), dict(null="y"),
                                              dict(null="mean"), dict(null="rv"), dict(training=0, null="rm", also="rv")],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items())[:40])
def test_forward_refuses_and_writes_nothing(bad):
    t, a = _fwd_args(n=18 if bad.get("G") == 9 else 5, D=64, ld=2112 if bad.get("D") else 64)
    if bad.get("D"):
        for k in ("gamma", "beta", "rm", "rv"):
            t[k] = torch.ones(2112, device=DEV)
        t["mean"], t["rstd"] = (torch.full((8, 2112), float("nan"), device=DEV) for _ in range(2))
    bad = dict(bad)
    for k in (bad.pop("null", None), bad.pop("also", None)):
        if k is not None:
            t[k] = None
    a.update(bad)
    before = {k: bits(t[k]) for k in ("rm", "rv") if t[k] is not None}
    with pytest.raises(_lib.LafsHipError):
        _call_fwd(t, a)
    torch.cuda.synchronize()
    for k in ("y", "mean", "rstd"):
        assert t[k] is None or bool(torch.isnan(t[k]).all()), f"{k} was written"
    for k, v in before.items():
        assert torch.equal(bits(t[k]), v), f"{k} was written"


def test_forward_eval_takes_one_row_groups():
    t, a = _fwd_args()
    a.update(rows=[0, 1, 5], training=0)
    _call_fwd(t, a)
    assert bool(torch.isfinite(t["y"]).all())


@pytest.mark.parametrize("bad", BAD_TABLES + [dict(lddy=63), dict(ldx=63), dict(lddx=63), dict(null="dy"), dict(null="x"),
                                              dict(null="mean"), dict(null="gamma"), dict(null="dx"), dict(null="dg"), dict(null="db")],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items())[:40])
def test_backward_refuses_and_writes_nothing(bad):
    t, a = _bwd_args(n=18 if bad.get("G") == 9 else 5, D=64, ld=2112 if bad.get("D") else 64)
    if bad.get("D"):
        t["gamma"] = torch.ones(2112, device=DEV)
        t["mean"], t["rstd"] = torch.zeros(8, 2112, device=DEV), torch.ones(8, 2112, device=DEV)
        t["dg"], t["db"] = (torch.full((2112,), float("nan"), device=DEV) for _ in range(2))
    bad = dict(bad)
    k = bad.pop("null", None)
    if k is not None:
        t[k] = None
    a.update(bad)
    with pytest.raises(_lib.LafsHipError):
        _call_bwd(t, a)
    torch.cuda.synchronize()
    for k in ("dx", "dg", "db"):
        assert t[k] is None or bool(torch.isnan(t[k]).all()), f"{k} was written"


def test_ops_refuse_a_table_that_does_not_cover_the_rows():
    t, _ = _fwd_args()
    with pytest.raises(_lib.LafsHipError):
        ops.bn1d_groups_fwd(t["x"], [0, 2, 4], t["gamma"], t["beta"], EPS, MOM, True, t["rm"], t["rv"])
