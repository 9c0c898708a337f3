"""Oracle of the mixing recipe beyond batch-mode mixup: per-row mixing of an image batch from explicit parameters, the DENSE soft
target with label smoothing, CosFace with a dense label, soft-target CE -- plain torch on the CPU (fp64 unless the caller passes
fp32), differentiated by autograd.  Test infrastructure only; pinned to the reference by tests/golden/f25_mixup_modes.npz
(tests/test_mixup_modes_host.py).  oracle/margin.py keeps the batch-mode forms."""
import torch
import torch.nn.functional as F


def mix_images(x, lam, cut, box):
    """Row b of `x` [B, 3, H, W] mixed with row B-1-b of the UNMIXED batch (util/mixup_my.py:152-200: every mode pairs b with B-1-b):
    cut[b]: the partner's pixels inside box[b] = (yl, yh, xl, xh), the row's own outside; otherwise lam[b] x[b] + (1 - lam[b]) x[B-1-b]
    (lam 1: untouched).  lam's dtype decides the blend's arithmetic (fp32 lambdas reproduce the reference's fp32 operations)."""
    B = x.shape[0]
    out = x.clone()
    for b in range(B):
        j = B - 1 - b
        if bool(cut[b]):
            yl, yh, xl, xh = (int(v) for v in box[b])
            out[b, :, yl:yh, xl:xh] = x[j, :, yl:yh, xl:xh]
        elif float(lam[b]) != 1.0:
            out[b] = x[b] * lam[b] + x[j] * (1 - lam[b])
    return out


def dense_target(y, num_classes, lam, smoothing=0.0, dtype=torch.float64):
    """y_bk = off + (1 - eps) (lam_b [k = y_b] + (1 - lam_b) [k = y_{B-1-b}]), off = eps / C (util/mixup_my.py:18-24: both one-hots
    carry on = 1 - eps + off and off elsewhere).  lam: [B]."""
    B = y.numel()
    lam = torch.as_tensor(lam, dtype=dtype).reshape(B, 1)
    off = smoothing / num_classes
    t = torch.full((B, num_classes), off, dtype=dtype)
    rows = torch.arange(B)
    t[rows, y.long()] += ((1.0 - smoothing) * lam).view(B)
    t[rows, y.long().flip(0)] += ((1.0 - smoothing) * (1.0 - lam)).view(B)
    return t


def cosface_dense_from_cos(cos, target, s=64.0, m=0.4):
    """CosFace's soft-label branch (face_pre_pro/ViT_face.py:65-87): y (cos - m) + (1 - y) cos, times s."""
    return s * (target * (cos - m) + (1.0 - target) * cos)


def cosine(emb, weight):
    return F.linear(F.normalize(emb), F.normalize(weight))


def soft_ce(logits, target):
    """timm SoftTargetCrossEntropy (train_largescale.py:820)."""
    return torch.sum(-target * F.log_softmax(logits, dim=-1), dim=-1).mean()


def loss_and_dcos(cos, y, lam, smoothing, s=64.0, m=0.4, dtype=torch.float64):
    """(mean loss, per-row losses, d mean loss / d cos) of the dense formulation, in `dtype`."""
    c = cos.detach().to(dtype).clone().requires_grad_(True)
    t = dense_target(y, c.shape[1], lam, smoothing, dtype)
    logits = cosface_dense_from_cos(c, t, s, m)
    rows = torch.sum(-t * F.log_softmax(logits, dim=-1), dim=-1)
    rows.mean().backward()
    return rows.mean().detach(), rows.detach(), c.grad
