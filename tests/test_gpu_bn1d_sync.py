"""lafs_bn1d_groups_stats / _sync_fwd / _bwd_sums / _sync_bwd (csrc/unfold.hip: fViT's BatchNorm1d head with the statistics of all ranks).

One process plays W ranks: every rank's rows go through the kernels as they would on that rank, the exchange buffer is filled slot by
slot and a torch sum stands in for the all-reduce of the backward sums.  Two yardsticks.  (a) fp64 on the CONCATENATED rows of a group,
element by element: y, save_mean, save_rstd, the running buffers and dx inside the operation-count bounds of tests/bn_sync_cases.py,
which never look at what a kernel returns (tests/test_bn_sync_host.py shows that they hold for the kernels' arithmetic and catch seeded
faults).  (b) bits: W = 1 is ops.bn1d_groups_fwd / _bwd in every output; every rank computes the same statistics and running buffers
from the same gathered buffer; dgamma / dbeta are the rank's own sums added in group order.
Planted columns: 0 constant, 1 level 1000 / spread 1e-2, 2 a level that moves by five spreads from rank to rank.  x, y, dy, dx are
[n, D] views of NaN-filled [n + 3, ld] buffers and the ranks' partials lie in a NaN-filled buffer with a padded rank stride: the
padding, the rows behind the last group and the gaps between the partials must stay NaN."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import bn_sync_cases as bc  # noqa: E402
import fp64_bounds as fb  # noqa: E402
from lafs_cvpr2024_amd import _lib, ops  # noqa: E402

DEV = "cuda"
f32 = torch.float32
EPS, MOM = bc.EPS, bc.MOM
GUARD, PAD = 3, 5                       # NaN rows behind the last group; NaN floats between the ranks' partials
_REF = {}


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def padded(t, ld):
    n, D = t.shape
    buf = torch.full((n + GUARD, ld), float("nan"), device=DEV)
    buf[:n, :D] = t.to(DEV)
    return buf[:n, :D], buf


def nan_view(n, D, ld):
    buf = torch.full((n + GUARD, ld), float("nan"), device=DEV)
    return buf[:n, :D], buf


def guards_untouched(buf, n, D):
    return bool(torch.isnan(buf[n:]).all()) and bool(torch.isnan(buf[:, D:]).all())


def reference(name, D):
    """fp64 references and bounds of a case, computed once."""
    if (name, D) not in _REF:
        c = bc.inputs(name, D)
        fwd = bc.sync_forward_reference(c, bc.f32val(EPS), bc.f32val(MOM))
        _REF[(name, D)] = (fwd, bc.sync_backward_bounds(c, bc.f32val(EPS), fwd["stats"]))
    return _REF[(name, D)]


def gathered(c, D, ld):
    """Every rank's lafs_bn1d_groups_stats into its slot of the exchange buffer.  Returns (partials view [W, G, 1 + 2 D], buffer, xs)."""
    W, G = len(c["tables"]), len(c["tables"][0])
    width = G * (1 + 2 * D)
    buf = torch.full((W, width + PAD), float("nan"), device=DEV)
    xs = []
    for rk, table in enumerate(c["tables"]):
        x, xbuf = padded(c["x"][rk], ld)
        ops.bn1d_groups_stats(x, bc.rows_of(table), out=buf[rk, :width].view(G, 1 + 2 * D))
        assert guards_untouched(xbuf, sum(table), D)
        xs.append(x)
    return buf[:, :width].unflatten(1, (G, 1 + 2 * D)), buf, xs


def totals(c):
    return [sum(t[g] for t in c["tables"]) for g in range(len(c["tables"][0]))]


def run_forward(c, D, ld):
    parts, pbuf, xs = gathered(c, D, ld)
    out = []
    for rk, table in enumerate(c["tables"]):
        n = sum(table)
        y, ybuf = nan_view(n, D, ld)
        rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
        _, mean, rstd = ops.bn1d_groups_sync_fwd(xs[rk], bc.rows_of(table), totals(c), parts, c["gamma"].to(DEV), c["beta"].to(DEV), EPS, MOM,
                                                 rm, rv, out=y)
        assert guards_untouched(ybuf, n, D) and bool(torch.isfinite(ybuf[:n, :D]).all())
        out.append(dict(y=y, save_mean=mean, save_rstd=rstd, running_mean=rm, running_var=rv))
    return out, parts, pbuf, xs


@pytest.mark.parametrize("D,ld", bc.DIMS)
@pytest.mark.parametrize("name", list(bc.RANK_TABLES))
def test_forward_and_backward_of_w_ranks_against_fp64_on_the_concatenated_rows(name, D, ld):
    c = bc.inputs(name, D)
    fwd_ref, bwd_ref = reference(name, D)
    W, G = len(c["tables"]), len(c["tables"][0])
    got, parts, pbuf, xs = run_forward(c, D, ld)
    tag = f"bn1d sync {name} D{D}"
    # the partials: counts, nothing written between the ranks' slots, a single row gives M2 = 0
    assert bool(torch.isnan(pbuf[:, G * (1 + 2 * D):]).all()) and bool(torch.isfinite(parts).all())
    assert parts[:, :, 0].cpu().tolist() == [[float(n) for n in t] for t in c["tables"]]
    for rk, table in enumerate(c["tables"]):
        for g, n in enumerate(table):
            if n == 1:
                assert bool((parts[rk, g, 1 + D:] == 0).all()) and torch.equal(parts[rk, g, 1:1 + D].cpu(), c["x"][rk][bc.rows_of(table)[g]])
    for rk in range(W):                                                      # (a) forward
        fb.check(f"{tag} rank {rk} y", got[rk]["y"].cpu(), *fwd_ref["y"][rk])
    for k in ("save_mean", "save_rstd", "running_mean", "running_var"):
        fb.check(f"{tag} {k}", got[0][k].cpu(), *fwd_ref[k])
        for rk in range(1, W):                                               # (b) the same bits on every rank
            assert torch.equal(bits(got[rk][k]), bits(got[0][k])), f"{k}: rank {rk} differs from rank 0"
    assert float(got[0]["save_rstd"][0, bc.COL_CONST]) == pytest.approx(bc.f32val(EPS) ** -0.5, rel=1e-6)
    again, _, _, _ = run_forward(c, D, ld)
    for k in got[0]:
        assert torch.equal(bits(got[W - 1][k]), bits(again[W - 1][k])), f"{k}: two runs differ"
    # backward: the ranks' sums, their total (the all-reduce), dx per rank
    mean, rstd, gamma = got[0]["save_mean"], got[0]["save_rstd"], c["gamma"].to(DEV)
    sums, dys = [], []
    for rk, table in enumerate(c["tables"]):
        dy, _ = padded(c["dy"][rk], ld)
        dg, db = c["old_dg"].to(DEV), c["old_db"].to(DEV)
        s = ops.bn1d_groups_bwd_sums(dy, xs[rk], bc.rows_of(table), mean, rstd, dg, db, accumulate=True)
        want_dg, want_db = c["old_dg"].to(DEV), c["old_db"].to(DEV)
        for g in range(G):                                                   # rank-local sums, added in group order
            want_db, want_dg = want_db + s[g, :D], want_dg + s[g, D:]
        assert torch.equal(bits(dg), bits(want_dg)) and torch.equal(bits(db), bits(want_db))
        sums.append(s); dys.append(dy)
    total = torch.stack(sums).sum(0)
    for rk, table in enumerate(c["tables"]):
        n = sum(table)
        dx, dxbuf = nan_view(n, D, ld)
        ops.bn1d_groups_sync_bwd(dys[rk], xs[rk], bc.rows_of(table), totals(c), mean, rstd, gamma, total, out=dx)
        assert guards_untouched(dxbuf, n, D) and bool(torch.isfinite(dxbuf[:n, :D]).all())
        fb.check(f"{tag} rank {rk} dx", dx.cpu(), *bwd_ref[rk])


@pytest.mark.parametrize("D,ld", bc.DIMS)
@pytest.mark.parametrize("table", [(2,), (2, 3), (4, 6), (2, 2, 2), (128, 512)], ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("accumulate", [True, False], ids=["accumulate", "overwrite"])
def test_one_rank_is_the_grouped_kernel_bit_for_bit(table, D, ld, accumulate):
    n, rows = sum(table), bc.rows_of(table)
    g = torch.Generator().manual_seed(n + D)
    r = lambda *s: torch.randn(*s, generator=g)
    x0 = r(n, D) * (0.5 + torch.rand(D, generator=g)) + r(D)
    x0[:, 0], x0[:, 1] = 0.37, 1000.0 + 1e-2 * r(n)
    x, _ = padded(x0, ld)
    dy, _ = padded(r(n, D), ld)
    gamma, beta = (1 + 0.1 * r(D)).to(DEV), (0.1 * r(D)).to(DEV)
    rm0, rv0, dg0, db0 = 0.1 * r(D), 1 + 0.2 * torch.rand(D, generator=g), r(D), r(D)
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    y, mean, rstd = ops.bn1d_groups_fwd(x, rows, gamma, beta, EPS, MOM, True, rm, rv)
    dg, db = dg0.to(DEV), db0.to(DEV)
    dx = ops.bn1d_groups_bwd(dy, x, rows, mean, rstd, gamma, True, dg, db, accumulate=accumulate)
    rm2, rv2 = rm0.to(DEV), rv0.to(DEV)
    part = ops.bn1d_groups_stats(x, rows)
    y2, mean2, rstd2 = ops.bn1d_groups_sync_fwd(x, rows, list(table), part[None], gamma, beta, EPS, MOM, rm2, rv2)
    dg2, db2 = dg0.to(DEV), db0.to(DEV)
    sums = ops.bn1d_groups_bwd_sums(dy, x, rows, mean2, rstd2, dg2, db2, accumulate=accumulate)
    dx2 = ops.bn1d_groups_sync_bwd(dy, x, rows, list(table), mean2, rstd2, gamma, sums)
    for k, a, b in (("y", y, y2), ("save_mean", mean, mean2), ("save_rstd", rstd, rstd2), ("running_mean", rm, rm2), ("running_var", rv, rv2),
                    ("dx", dx, dx2), ("dgamma", dg, dg2), ("dbeta", db, db2)):
        assert torch.equal(bits(a), bits(b)), f"{k}: the one-rank pair differs from the grouped kernel"
    assert not torch.equal(bits(rm), bits(rm0))


# ------------------------------------------------------------------------------------------------ refusals
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _tab(v):
    return None if v is None else (C.c_int * len(v))(*v)


def _args(n=5, D=64, ld=64, W=2):
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    t = dict(x=torch.randn(n, ld, device=DEV), dy=torch.randn(n, ld, device=DEV), gamma=torch.ones(D, device=DEV), beta=torch.zeros(D, device=DEV),
             rm=torch.zeros(D, device=DEV), rv=torch.ones(D, device=DEV), y=nan(n, ld), mean=nan(8, D), rstd=nan(8, D), dx=nan(n, ld),
             partial=nan(2, 1 + 2 * D), partials=torch.ones(W, 2, 1 + 2 * D, device=DEV), sums=nan(2, 2 * D), dg=nan(D), db=nan(D))
    return t, dict(rows=[0, 1, 5], total=[4, 9], G=2, D=D, ld=ld, W=W, ldw=2 * (1 + 2 * D))


def _call(which, t, a):
    if which == "stats":
        _lib.call("lafs_bn1d_groups_stats", _p(t["x"]), a["ld"], _tab(a["rows"]), a["G"], a["D"], _p(t["partial"]))
    elif which == "sync_fwd":
        _lib.call("lafs_bn1d_groups_sync_fwd", _p(t["x"]), a["ld"], _tab(a["rows"]), _tab(a["total"]), a["G"], a["D"], _p(t["partials"]), a["W"],
                  a["ldw"], _p(t["gamma"]), _p(t["beta"]), EPS, MOM, _p(t["rm"]), _p(t["rv"]), _p(t["y"]), a["ld"], _p(t["mean"]), _p(t["rstd"]))
    elif which == "bwd_sums":
        _lib.call("lafs_bn1d_groups_bwd_sums", _p(t["dy"]), a["ld"], _p(t["x"]), a["ld"], _tab(a["rows"]), a["G"], a["D"], _p(t["rm"]), _p(t["rv"]),
                  _p(t["sums"]), _p(t["dg"]), _p(t["db"]), 0)
    else:
        _lib.call("lafs_bn1d_groups_sync_bwd", _p(t["dy"]), a["ld"], _p(t["x"]), a["ld"], _tab(a["rows"]), _tab(a["total"]), a["G"], a["D"],
                  _p(t["rm"]), _p(t["rv"]), _p(t["gamma"]), _p(t["partials"]), _p(t["dx"]), a["ld"])


OUTPUTS = dict(stats=("partial",), sync_fwd=("y", "mean", "rstd"), bwd_sums=("sums", "dg", "db"), sync_bwd=("dx",))
BAD = [("stats", dict(rows=None)), ("stats", dict(rows=[0, 0, 5])), ("stats", dict(G=9)), ("stats", dict(ld=63)), ("stats", dict(null="partial")),
       ("sync_fwd", dict(total=[1, 9], rows=[0, 1, 5])), ("sync_fwd", dict(total=[4, 3])), ("sync_fwd", dict(total=None)), ("sync_fwd", dict(W=0)),
       ("sync_fwd", dict(W=4097)), ("sync_fwd", dict(ldw=100)), ("sync_fwd", dict(null="partials")), ("sync_fwd", dict(null="rv")),
       ("sync_fwd", dict(rows=[0, 5, 5])), ("bwd_sums", dict(null="sums")), ("bwd_sums", dict(rows=[1, 2, 5])), ("bwd_sums", dict(D=2112)),
       ("sync_bwd", dict(total=[4, 3])), ("sync_bwd", dict(total=[1, 4], rows=[0, 1, 5])), ("sync_bwd", dict(null="partials")),
       ("sync_bwd", dict(ld=63))]


@pytest.mark.parametrize("which,bad", BAD, ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={x}" for k, x in v.items())[:32])
def test_refusals_write_nothing(which, bad):
    t, a = _args()
    bad = dict(bad)
    k = bad.pop("null", None)
    if k is not None:
        t[k] = None
    a.update(bad)
    before = {k: bits(t[k]) for k in ("rm", "rv") if t[k] is not None}
    with pytest.raises(_lib.LafsHipError):
        _call(which, t, a)
    torch.cuda.synchronize()
    for k in OUTPUTS[which]:
        assert t[k] is None or bool(torch.isnan(t[k]).all()), f"{k} was written"
    for k, v in before.items():
        assert torch.equal(bits(t[k]), v), f"{k} was written"


def test_one_row_on_a_rank_is_accepted_where_the_total_has_two():
    t, a = _args()
    _call("stats", t, a)
    _call("sync_fwd", t, a)
    assert bool(torch.isfinite(t["y"][:, :64]).all()) and float(t["partial"][0, 0]) == 1.0 and float(t["partial"][1, 0]) == 4.0


def test_ops_refuse_partials_of_another_shape():
    t, _ = _args()
    with pytest.raises(_lib.LafsHipError):
        ops.bn1d_groups_sync_fwd(t["x"][:, :64], [0, 1, 5], [4, 9], t["partials"][:, :1], t["gamma"], t["beta"], EPS, MOM, t["rm"], t["rv"])
    with pytest.raises(_lib.LafsHipError):
        ops.bn1d_groups_sync_fwd(t["x"][:, :64], [0, 1, 5], [4], t["partials"], t["gamma"], t["beta"], EPS, MOM, t["rm"], t["rv"])
