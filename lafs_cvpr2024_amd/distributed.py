"""Data-parallel plumbing of the LAFS step: flat-arena gradient all-reduce (sum; the 1/world mean is folded into the fused
AdamW kernel's grad_scale) and the DINO center column-sum all-reduce (reference: DDP at lafs_train.py:375 and
dist.all_reduce at :675).  Backend-agnostic: "nccl" is RCCL over xGMI on MI355X, "gloo" is used by the CPU tests.

The arena orders parameters [trunk | head]; the head range (the 25.6 M-parameter last layer dominates) is reduced while the
trunk backward is still running, the trunk range right after it."""
import torch
import torch.distributed as dist


def world_size():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


class FlatReducer:
    """Launches asynchronous SUM all-reduces on slices of flat buffers and waits for all of them at once.

    wire="bf16" (LAFS_GRAD_WIRE=bf16, opt-in): fp32 slices travel as bf16 -- cast into a staging buffer, reduced there, cast back
    on wait_all -- which halves the bytes on the xGMI links (211 -> 105 MB per LAFS step) at the price of a bf16 rounding of every
    rank's contribution and of the partial sums inside the collective; the default "f32" is what the reference's DDP sends."""

    def __init__(self, group=None, wire=None):
        import os
        self.group = group
        self.pending = []
        self.wire = wire or os.environ.get("LAFS_GRAD_WIRE", "f32")
        if self.wire not in ("f32", "bf16"):
            raise ValueError("LAFS_GRAD_WIRE must be f32 or bf16")

    @property
    def active(self):
        # LAFS_REDUCE_SINGLE_RANK=1 (tests): issue the collectives even in a one-rank process group, so that a single GPU runs the
        # whole multi-rank launch structure (graph segments, asynchronous RCCL all-reduces between them, stream-side waits)
        if world_size() > 1:
            return True
        import os
        return os.environ.get("LAFS_REDUCE_SINGLE_RANK") == "1" and dist.is_available() and dist.is_initialized()

    def launch(self, tensor, exact=False):
        """Starts the all-reduce; returns a token for wait() (None when there is nothing to wait for).  exact: never through the bf16
        wire (statistics, not gradients)."""
        if not self.active:
            return None
        if not exact and self.wire == "bf16" and tensor.dtype == torch.float32 and tensor.is_cuda and tensor.numel() >= (1 << 16):
            from .ops import _p, call
            stage = torch.empty(tensor.numel(), device=tensor.device, dtype=torch.bfloat16)
            call("lafs_cast_bf16", _p(tensor), _p(stage), tensor.numel())
            tok = (dist.all_reduce(stage, op=dist.ReduceOp.SUM, group=self.group, async_op=True), stage, tensor)
        else:
            tok = (dist.all_reduce(tensor, op=dist.ReduceOp.SUM, group=self.group, async_op=True), None, None)
        self.pending.append(tok)
        return tok

    def wait(self, tokens):
        """Makes the current stream wait for these launches (and casts bf16-wire slices back to fp32)."""
        for tok in tokens:
            if tok is None or tok not in self.pending:
                continue
            work, stage, tensor = tok
            work.wait()
            if stage is not None:
                from .ops import _p, call
                call("lafs_cast_f32", _p(stage), _p(tensor), tensor.numel())
            self.pending.remove(tok)

    def wait_all(self):
        self.wait(list(self.pending))


def center_from_colsum(center, colsum, rows_per_rank, momentum):
    """center <- m*center + (1-m) * (sum over ranks of column sums) / (rows * world)   (reference lafs_train.py:674-679).
    `colsum` must already be all-reduced.  Pure torch: used by the CPU tests as the statement of what the HIP
    lafs_center_ema kernel computes."""
    return center * momentum + colsum / (rows_per_rank * world_size()) * (1 - momentum)


# ---------------------------------------------------------------------------------------------- cross-rank BatchNorm statistics
class BnStatExchange:
    """The two small collectives of the fViT head's cross-rank BatchNorm (the reference's SyncBatchNorm, lafs_train.py:362-364), outside
    the graphs like the gradient all-reduces.

    Forward: the partial statistics of ALL networks (student and teacher) travel in ONE buffer f32 [W, sum_i G_i (1 + 2 D)].  A rank's
    kernels write its own row (`slot(i)`, after `clear()` has zeroed the buffer), `gather()` SUM-all-reduces the buffer: every other
    rank contributed +0.0 to this row, so the sum is exact and the result is the all-gather -- on every backend, gloo with device
    tensors included.  `all(i)` is network i's [W, G_i, 1 + 2 D] view for lafs_bn1d_groups_sync_fwd.
    Backward: `sums` f32 [G_0, 2 D] (the first network is the one that is trained) is SUM-all-reduced by `reduce_sums()`.
    Both go through `reducer` (a FlatReducer: same group, same tokens, `exact`: never the bf16 wire); without a process group nothing
    is sent and one rank's values stay as they are."""

    def __init__(self, groups, D, device, reducer, dtype=torch.float32):
        self.reducer, self.D = reducer, D
        self.world = world_size()
        self.rank = dist.get_rank(reducer.group) if self.world > 1 else 0
        w = 1 + 2 * D
        self.spans, at = [], 0
        for G in groups:
            self.spans.append((at, G))
            at += G * w
        self.partials = torch.zeros(self.world, at, device=device, dtype=dtype)
        self.sums = torch.zeros(groups[0], 2 * D, device=device, dtype=dtype)

    def clear(self):
        """Zeroes the exchange buffer (capturable); this rank's slots are written afterwards."""
        from .ops import zero_
        return zero_(self.partials) if self.partials.is_cuda else self.partials.zero_()

    def slot(self, i):
        at, G = self.spans[i]
        return self.partials[self.rank, at: at + G * (1 + 2 * self.D)].view(G, 1 + 2 * self.D)

    def all(self, i):
        at, G = self.spans[i]
        return self.partials[:, at: at + G * (1 + 2 * self.D)].unflatten(1, (G, 1 + 2 * self.D))

    def gather(self):
        return self.reducer.launch(self.partials, exact=True)

    def reduce_sums(self):
        return self.reducer.launch(self.sums, exact=True)


# Pure torch statements of what the four lafs_bn1d_groups_* cross-rank kernels compute (any dtype; the CPU tests run them in fp64 under
# gloo).  `rows`: this rank's row table [0, ..., n]; a partial is [G, 1 + 2 D] = per group {count, mean[D], M2[D]}.
def bn_partial_stats(x, rows):
    out = x.new_zeros(len(rows) - 1, 1 + 2 * x.shape[1])
    for g, (a, b) in enumerate(zip(rows[:-1], rows[1:])):
        mean = x[a:b].mean(0)
        out[g] = torch.cat([x.new_tensor([b - a]), mean, ((x[a:b] - mean) ** 2).sum(0)])
    return out


def bn_combine_partials(partials):
    """partials [W, G, 1 + 2 D] -> (N [G, 1], mean [G, D], M2 [G, D]), folded in rank order 0 .. W-1 with the pairwise update."""
    D = (partials.shape[2] - 1) // 2
    n, mean, m2 = partials[0, :, :1].clone(), partials[0, :, 1:1 + D].clone(), partials[0, :, 1 + D:].clone()
    for r in range(1, partials.shape[0]):
        nb, mean_b, m2_b = partials[r, :, :1], partials[r, :, 1:1 + D], partials[r, :, 1 + D:]
        tot, delta = n + nb, mean_b - mean
        mean = mean + delta * nb / tot
        m2 = m2 + m2_b + delta * delta * n * nb / tot
        n = tot
    return n, mean, m2


def bn_sync_forward(x, rows, partials, gamma, beta, eps, momentum, running_mean, running_var):
    """-> (y, save_mean [G, D], save_rstd [G, D], running_mean, running_var): the running buffers stepped once per group, group 0
    first, with the unbiased variance M2 / (N - 1) of the TOTAL count."""
    n, mean, m2 = bn_combine_partials(partials)
    rstd = 1 / torch.sqrt(m2 / n + eps)
    y = torch.empty_like(x)
    for g, (a, b) in enumerate(zip(rows[:-1], rows[1:])):
        y[a:b] = (x[a:b] - mean[g]) * rstd[g] * gamma + beta
        running_mean = (1 - momentum) * running_mean + momentum * mean[g]
        running_var = (1 - momentum) * running_var + momentum * m2[g] / (n[g] - 1)
    return y, mean, rstd, running_mean, running_var


def bn_backward_sums(dy, x, rows, mean, rstd):
    """-> sums [G, 2 D] = per group {sum dy, sum dy xhat} over this rank's rows; their sum over the groups is this rank's dbeta / dgamma."""
    return torch.stack([torch.cat([dy[a:b].sum(0), (dy[a:b] * (x[a:b] - mean[g]) * rstd[g]).sum(0)])
                        for g, (a, b) in enumerate(zip(rows[:-1], rows[1:]))])


def bn_sync_backward(dy, x, rows, totals, mean, rstd, gamma, sums):
    """dx = gamma rstd (dy - sum dy / N - xhat sum(dy xhat) / N) with the sums of ALL ranks and the total counts N."""
    D = x.shape[1]
    dx = torch.empty_like(x)
    for g, (a, b) in enumerate(zip(rows[:-1], rows[1:])):
        xh = (x[a:b] - mean[g]) * rstd[g]
        dx[a:b] = gamma * rstd[g] * (dy[a:b] - sums[g, :D] / totals[g] - xh * sums[g, D:] / totals[g])
    return dx
