"""KoLeo regulariser (Kozachenko-Leonenko differential entropy estimator) as a module, for use outside the pre-training engine.

Signature and semantics of DINOv2's published KoLeoLoss (PARITY UNPINNED: restated, the definition is in include/lafs_hip.h): the rows
are L2-normalised, every row's nearest neighbour in the batch is found by the largest dot product, and the loss is
-mean(log(||xh_i - xh_I(i) + eps|| + eps)).  Forward and gradient are one call of the HIP kernel pair behind ops.koleo (csrc/koleo.hip),
all fp32; the engine calls the same kernels directly on its static buffers (engine.py, koleo_weight)."""
import torch
from torch import nn

from . import _lib, ops


class _KoLeo(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        xc = x.detach()
        if xc.dim() != 2 or xc.dtype != torch.float32:
            raise _lib.LafsHipError("KoLeoLoss: one group of [n, D] float32 rows expected")
        if xc.stride(-1) != 1 or xc.stride(0) % 4 or xc.data_ptr() % 16:
            xc = xc.contiguous()
        dx = torch.empty_like(xc, memory_format=torch.contiguous_format)
        loss, _ = ops.koleo(xc, 1, xc.shape[0], eps=eps, dx=dx)
        ctx.save_for_backward(dx)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_output):
        (dx,) = ctx.saved_tensors
        return dx * grad_output, None


class KoLeoLoss(nn.Module):
    def forward(self, student_output, eps=1e-8):
        """student_output: [n, D] float32 device rows of ONE group (n >= 2, 4 <= D <= 1024, D % 4 == 0) -> scalar loss."""
        return _KoLeo.apply(student_output, eps)
