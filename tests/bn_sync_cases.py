"""Shared by the cross-rank BatchNorm tests (tests/test_bn_sync_host.py, test_gpu_bn1d_sync.py, test_gpu_step_fvit_sync.py): the case
grid, the fp64 oracle of lafs_bn1d_groups_stats / _sync_fwd / _bwd_sums / _sync_bwd with per-element bounds, and an fp32 emulation of the
kernels' arithmetic on the CPU.

The bounds extend those of tests/fvit_cases.py (bn_stats, bn_forward_reference, bn_backward_bounds) to W partials.  They count the
roundings of the formulas in include/lafs_hip.h and never read what a kernel returns:
  partial of rank r   mean_r, M2_r = n_r var_r of `bn_stats` on the rank's own rows (its e_var bounds var = M2 / n, so n e_var bounds M2)
  fold a <- a + b     n = n_a + n_b (exact), delta = mean_b - mean_a (1 rounding), mean = mean_a + delta n_b / n: algebraically
                      mean_a n_a / n + mean_b n_b / n, so the partials' errors enter with those weights; product, quotient and the
                      rounding of delta give 3 u |delta| n_b / n, the addition u |mean|
                      M2 = M2_a + M2_b + delta^2 n_a n_b / n: delta is off by e_a + e_b + u |delta|, the term rounds 4 times, the two
                      additions once each
  statistics          var = M2 / N (1 rounding), rstd as bn_stats (interval through the root + 4 u), running buffers as
                      bn_forward_reference with the TOTAL count, chained over the groups: the buffer a group reads carries the
                      previous group's bound, scaled by (1 - momentum)
  backward            the ranks' sums as bn_backward_bounds per rank (n_r u sum|terms|), the all-reduce in ANY order ((W - 1) u sum of
                      the ranks' magnitudes), then dx exactly as bn_backward_bounds with N in place of n
"""
import torch

from fvit_cases import SLACK, U, _rs, bn_stats, bn_xhat

f32, f64 = torch.float32, torch.float64
EPS, MOM = 1e-5, 0.1
BN_WAVES = 8                          # csrc/unfold.hip: rows strided over 8 waves, the waves' sums added in wave order

# per-rank row tables: one tuple per rank, one entry per group
RANK_TABLES = {
    "w2_one_row": [(1,), (3,)],
    "w2_uneven": [(2, 3), (4, 1)],
    "w3_uneven": [(3, 1, 2), (1, 5, 2), (7, 2, 1)],
    "w8_2x2": [(2, 2)] * 8,
    "w8_16x64": [(16, 64)] * 8,
}
DIMS = [(64, 64), (200, 232), (768, 768)]
COL_CONST, COL_LEVEL, COL_RANK_LEVEL = 0, 1, 2      # the planted columns


def f32val(v):
    return float(torch.tensor(v, dtype=f32))


def rows_of(table):
    out = [0]
    for n in table:
        out.append(out[-1] + n)
    return out


_CACHE = {}


def inputs(name, D):
    """fp32 inputs on the CPU, made once per case and left unchanged: per rank x / dy [n_r, D] (groups packed in order), shared gamma,
    beta, running buffers, old dgamma / dbeta.  Column 0 is constant, column 1 has level 1000 and spread 1e-2 (the planted columns of
    tests/test_gpu_bn1d_groups.py), column 2 has spread 1e-2 around a level that moves by 0.05 = five spreads from rank to rank."""
    key = (name, D)
    if key not in _CACHE:
        tables = RANK_TABLES[name]
        G = len(tables[0])
        g = torch.Generator().manual_seed(sum(map(sum, tables)) * 1000 + D + len(tables))
        r = lambda *s: torch.randn(*s, generator=g)
        scale, level = 0.5 + torch.rand(D, generator=g), r(D)
        glevel = [r(D) for _ in range(G)]
        xs, dys = [], []
        for rk, table in enumerate(tables):
            n = sum(table)
            x = r(n, D) * scale + level + 0.3 * r(D)                        # every rank has a level of its own in every column
            for gi, (a, b) in enumerate(zip(rows_of(table)[:-1], rows_of(table)[1:])):
                x[a:b] += glevel[gi]
            x[:, COL_CONST] = 0.37
            x[:, COL_LEVEL] = 1000.0 + 1e-2 * r(n)
            x[:, COL_RANK_LEVEL] = 2.0 + 0.05 * rk + 1e-2 * r(n)
            xs.append(x)
            dys.append(r(n, D))
        _CACHE[key] = dict(tables=tables, x=xs, dy=dys, gamma=1 + 0.1 * r(D), beta=0.1 * r(D), rm=0.1 * r(D),
                           rv=1 + 0.2 * torch.rand(D, generator=g), old_dg=r(D), old_db=r(D))
    return _CACHE[key]


def group_slices(c, g):
    """The rows of group g on every rank: [(x_r, dy_r)] in rank order (fp32)."""
    out = []
    for table, x, dy in zip(c["tables"], c["x"], c["dy"]):
        a, b = rows_of(table)[g], rows_of(table)[g + 1]
        out.append((x[a:b], dy[a:b]))
    return out


# ------------------------------------------------------------------------------------------------ fp64 oracle with bounds
def sync_stats(xs, eps):
    """One group.  xs: the ranks' rows [n_r, D] (fp64, rank order).  Returns a dict of fp64 references and bounds: the exact statistics
    of the concatenated rows, and how far the kernels' fold of the W fp32 partials may lie from them."""
    X = torch.cat(xs)
    N = X.shape[0]
    mean = X.mean(0)
    M2 = ((X - mean) ** 2).sum(0)
    n = mu = e_mu = M = e_M = None
    for x in xs:
        nb = x.shape[0]
        mb, e_mb, vb, e_vb, _, _ = bn_stats(x, eps)
        Mb, e_Mb = vb * nb, e_vb * nb
        if n is None:
            n, mu, e_mu, M, e_M = nb, mb, e_mb, Mb, e_Mb
            continue
        tot = n + nb
        d = mb - mu
        e_d = e_mu + e_mb + U * (d.abs() + e_mu + e_mb)
        mu2 = mu + d * nb / tot
        e_mu2 = SLACK * (e_mu * n / tot + e_mb * nb / tot + 3 * U * (d.abs() + e_mu + e_mb) * nb / tot + U * mu2.abs())
        w = n * nb / tot
        c = d * d * w
        e_c = (2 * d.abs() * e_d + e_d * e_d) * w + 4 * U * (d.abs() + e_d) ** 2 * w
        M2n = M + Mb + c
        e_M = SLACK * (e_M + e_Mb + e_c + 2 * U * (M2n + e_M + e_Mb + e_c))
        n, mu, e_mu, M = tot, mu2, e_mu2, M2n
    var = M2 / N
    e_var = SLACK * (e_M / N + U * var)
    rs = _rs(var, eps)
    e_rs = torch.maximum(_rs(var - e_var, eps) - rs, rs - _rs(var + e_var, eps)) + 4 * U * rs
    return dict(N=N, mean=mean, e_mean=e_mu, M2=M2, e_M2=e_M, var=var, e_var=e_var, rstd=rs, e_rstd=e_rs)


def running_step(old, e_old, new, e_new, momentum):
    """(1 - m) old + m new on a buffer known to within e_old: (1 - m) rounds, two products, one addition (bn_forward_reference)."""
    a, b = (1 - momentum) * old, momentum * new
    return a + b, SLACK * ((1 - momentum) * e_old + momentum * e_new + 3 * U * (a.abs() + b.abs()))


def sync_forward_reference(c, eps, momentum):
    """Everything lafs_bn1d_groups_sync_fwd writes on every rank for case `c`, as (fp64 value, bound):
    {"y": [per rank [n_r, D]], "save_mean" / "save_rstd": [G, D], "running_mean" / "running_var": [D]} plus "stats": per group."""
    gamma, beta = c["gamma"].double(), c["beta"].double()
    G = len(c["tables"][0])
    rm, e_rm = c["rm"].double(), torch.zeros_like(c["rm"].double())
    rv, e_rv = c["rv"].double(), torch.zeros_like(c["rv"].double())
    ys = [[] for _ in c["tables"]]
    stats, means, rstds = [], [], []
    for g in range(G):
        xs = [x.double() for x, _ in group_slices(c, g)]
        st = sync_stats(xs, eps)
        stats.append(st)
        N = st["N"]
        for rk, x in enumerate(xs):
            xh, e_xh = bn_xhat(x, st["mean"], st["e_mean"], st["rstd"], st["e_rstd"])
            y = xh * gamma + beta
            ys[rk].append((y, SLACK * (e_xh * gamma.abs() + U * (xh * gamma).abs() + U * y.abs())))
        means.append((st["mean"], st["e_mean"]))
        rstds.append((st["rstd"], st["e_rstd"]))
        rm, e_rm = running_step(rm, e_rm, st["mean"], st["e_mean"], momentum)
        vu = st["var"] * N / (N - 1)
        rv, e_rv = running_step(rv, e_rv, vu, st["e_var"] * N / (N - 1) + 2 * U * vu, momentum)
    cat = lambda pairs: (torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs]))
    stack = lambda pairs: (torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs]))
    return {"y": [cat(p) for p in ys], "save_mean": stack(means), "save_rstd": stack(rstds), "running_mean": (rm, e_rm),
            "running_var": (rv, e_rv), "stats": stats}


def sync_backward_bounds(c, eps, stats):
    """dx of lafs_bn1d_groups_sync_bwd per rank ([n_r, D], the groups in order) as (fp64 value, bound), fed with the forward kernels'
    own save_mean / save_rstd (their bounds enter) and with the ranks' sums added in any order."""
    gamma = c["gamma"].double()
    W = len(c["tables"])
    out = [[] for _ in range(W)]
    for g, st in enumerate(stats):
        N = st["N"]
        parts = []
        db = dg = e_db = e_dg = a_db = a_dg = 0
        for x, dy in group_slices(c, g):
            x, dy = x.double(), dy.double()
            n = x.shape[0]
            xh, e_xh = bn_xhat(x, st["mean"], st["e_mean"], st["rstd"], st["e_rstd"])
            db_r, e_db_r = dy.sum(0), n * U * dy.abs().sum(0)
            dg_r = (dy * xh).sum(0)
            e_dg_r = (dy.abs() * e_xh).sum(0) + (n + 1) * U * (dy.abs() * (xh.abs() + e_xh)).sum(0)
            db, dg, e_db, e_dg = db + db_r, dg + dg_r, e_db + e_db_r, e_dg + e_dg_r
            a_db, a_dg = a_db + db_r.abs() + e_db_r, a_dg + dg_r.abs() + e_dg_r
            parts.append((dy, xh, e_xh))
        e_db, e_dg = e_db + (W - 1) * U * a_db, e_dg + (W - 1) * U * a_dg
        gr = gamma * st["rstd"]
        e_gr = gamma.abs() * st["e_rstd"] + U * gr.abs()
        mb, mg = db / N, dg / N
        e_mb, e_mg = e_db / N + U * mb.abs(), e_dg / N + U * mg.abs()
        for rk, (dy, xh, e_xh) in enumerate(parts):
            t2 = xh * mg
            e_t2 = e_xh * mg.abs() + xh.abs() * e_mg + e_xh * e_mg + U * t2.abs()
            inner = dy - mb - t2
            e_in = e_mb + e_t2 + 2 * U * (dy.abs() + mb.abs() + t2.abs())
            dx = gr * inner
            out[rk].append((dx, SLACK * (e_gr * inner.abs() + gr.abs() * e_in + e_gr * e_in + U * dx.abs())))
    return [(torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])) for pairs in out]


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels (CPU)
def _wave_sum(terms):
    """Sum over the rows as the kernels do it: row r goes to wave r % 8, a wave adds its rows in order, the waves' sums are added in
    wave order.  terms: f32 [n, D]."""
    parts = []
    for w in range(BN_WAVES):
        s = torch.zeros(terms.shape[1], dtype=f32)
        for r in range(w, terms.shape[0], BN_WAVES):
            s = s + terms[r]
        parts.append(s)
    s = parts[0]
    for p in parts[1:]:
        s = s + p
    return s


def emulate(c, eps, momentum, fault=None):
    """The four kernels in fp32 on the CPU, rank by rank, with torch sums standing in for the all-reduce.  fault: None, or one of
    "biased_running_var" (the running buffer takes M2 / N), "no_delta_term" (the fold drops delta^2 n_a n_b / n), "rank_count"
    (the backward divides the sums by the rank's own row count).  Returns the outputs in the layout of sync_forward_reference plus
    "dx": [per rank]."""
    tables, W, G = c["tables"], len(c["tables"]), len(c["tables"][0])
    D = c["gamma"].numel()
    eps32, mom32 = torch.tensor(eps, dtype=f32), torch.tensor(momentum, dtype=f32)
    one = torch.tensor(1.0, dtype=f32)
    rm, rv = c["rm"].clone(), c["rv"].clone()
    ys, dxs = [[] for _ in range(W)], [[] for _ in range(W)]
    means, rstds = [], []
    for g in range(G):
        sl = group_slices(c, g)
        parts = []
        for x, _ in sl:
            n = torch.tensor(float(x.shape[0]), dtype=f32)
            mean = x[0] + _wave_sum(x - x[0]) / n
            d = x - mean
            parts.append((n, mean, _wave_sum(d * d)))
        nf, mean, m2 = parts[0]
        for nb, mean_b, m2_b in parts[1:]:
            tot, delta = nf + nb, mean_b - mean
            mean = mean + delta * nb / tot
            m2 = m2 + m2_b + (0 if fault == "no_delta_term" else delta * delta * nf * nb / tot)
            nf = tot
        var = m2 / nf
        rstd = one / torch.sqrt(var + eps32)
        rm = (one - mom32) * rm + mom32 * mean
        rv = (one - mom32) * rv + mom32 * (var if fault == "biased_running_var" else var * (nf / (nf - one)))
        means.append(mean); rstds.append(rstd)
        sb = sg = 0
        for x, dy in sl:
            sb, sg = sb + _wave_sum(dy), sg + _wave_sum(dy * ((x - mean) * rstd))
        for rk, (x, dy) in enumerate(sl):
            ys[rk].append((x - mean) * rstd * c["gamma"] + c["beta"])
            cnt = torch.tensor(float(x.shape[0]), dtype=f32) if fault == "rank_count" else nf
            xh = (x - mean) * rstd
            dxs[rk].append(c["gamma"] * rstd * (dy - sb / cnt - xh * (sg / cnt)))
    return {"y": [torch.cat(v) for v in ys], "dx": [torch.cat(v) for v in dxs], "save_mean": torch.stack(means),
            "save_rstd": torch.stack(rstds), "running_mean": rm, "running_var": rv}
