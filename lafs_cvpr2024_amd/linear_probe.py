"""Linear-probe evaluation of frozen features on the device (DINO's eval_linear.py protocol; no counterpart in the reference; the
protocol is restated: PARITY UNPINNED).  The trained half of the pair whose other half is lafs_cvpr2024_amd.knn.

    features f32 [N, F], computed once per record, not normalised
      -> LinearProbe: logits = x W^T + b on lafs_gemm_nt (bf16 operands, fp32 logits)
      -> lafs_softmax_ce_rank: per row the cross-entropy, the rank of the target among the logits, the bf16 gradient
      -> lafs_gemm_tn_acc: dW = dlogits^T x with db as its column sum
      -> lafs_clip_momentum_ema_range: SGD, momentum 0.9, no weight decay, no clip -- on a ParamArena (fp32 master, bf16 shadow, one
         momentum buffer)
      -> top-1 / top-5 accuracy in percent (rank == 0 / rank < 5) and the mean loss

The evaluation set is knn's: a RecordIO face set split per identity by knn.holdout_split; the bank rows train the classifier and the
query rows validate it.  `shots = K` keeps the first K training records of every identity: the few-shot probe.  `evaluate_backbone` is
what `python -m lafs_cvpr2024_amd.eval_linear` runs.

Deviations from DINO's script: the features are cached, so there is no training augmentation (RandomResizedCrop, flip); the identity
hold-out split stands in for a val folder; the short last batch of an epoch is padded with rows that have no target (y = -1) and
normalised by the rows that have one, not dropped; the images are not resized or centre-cropped (the face sets are 112 x 112).
"""
import json
import math

import numpy as np
import torch

from . import _lib, knn, ops
from .arena import ParamArena
from .ops import _p, call

MOMENTUM = 0.9                                            # DINO's eval_linear.py: SGD(momentum=0.9, weight_decay=0)
K_GRANULE = 32                                            # lafs_gemm_nt: K % 32 == 0
N_GRANULE = 8                                             # lafs_gemm_tn_acc: N1 % 8 == 0


def _round_up(n, m):
    return (n + m - 1) // m * m


# --------------------------------------------------------------------------------------------------------------- features
@torch.no_grad()
def probe_features(model, images_iter, n_last_blocks=1, avgpool=False, norm=None, landmark_teacher=None, device=None):
    """Eval-mode probe features over uint8 batches [B, 3, S, S] -> f32 [N, F] on the device, not L2-normalised.
    VisionTransformer: the cls rows of get_intermediate_layers(x, n_last_blocks) concatenated in block order and, with avgpool, the
    mean of the last block's patch tokens behind them (DINO's eval_linear feature).  Part-fViT and fViT: exactly knn.extract_bank's
    rows, the model's own output, which the fine-tune consumes; n_last_blocks > 1 or avgpool is refused for them."""
    from . import vision_transformer as vits
    from .augment import HALF_NORM
    if not isinstance(model, vits.VisionTransformer):
        if int(n_last_blocks) != 1 or avgpool:
            raise ValueError(f"{type(model).__name__}: the probe takes the model's own output; n_last_blocks > 1 and avgpool are "
                             "defined for the DINO VisionTransformer only")
        return knn.extract_bank(model, images_iter, norm=norm, landmark_teacher=landmark_teacher, device=device)
    mean, std = norm if norm is not None else HALF_NORM
    device = torch.device(device if device is not None else ("cuda", torch.cuda.current_device()))
    was_training = model.training
    model.eval()
    try:
        arena = getattr(model, "_arena", None)
        if arena is None:
            arena = vits.attach_arena(model, device)
        arena.ensure_fresh()
        feats = []
        for u8 in images_iter:
            x = knn._normalise(u8.to(device), mean, std)
            outs = model.get_intermediate_layers(x, int(n_last_blocks))
            cols = [o[:, 0] for o in outs]
            if avgpool:
                cols.append(outs[-1][:, 1:].mean(dim=1))
            feats.append(torch.cat(cols, dim=-1).float())
        if not feats:
            raise ValueError("probe_features: no images")
        return torch.cat(feats)
    finally:
        model.train(was_training)


# --------------------------------------------------------------------------------------------------------------- split, schedule
def select_shots(labels, bank_idx, shots):
    """The first `shots` records of every identity among bank_idx (ascending record indices), order kept; an identity with fewer
    keeps what it has.  shots <= 0: all of them."""
    bank_idx = np.asarray(bank_idx, np.int64)
    if shots is None or shots <= 0 or len(bank_idx) == 0:
        return bank_idx
    lab = np.asarray(labels).astype(np.int64).ravel()[bank_idx]
    order = np.argsort(lab, kind="stable")
    sorted_l = lab[order]
    first = np.flatnonzero(np.r_[True, sorted_l[1:] != sorted_l[:-1]])
    place = np.arange(len(lab)) - np.repeat(first, np.diff(np.r_[first, len(lab)]))
    return np.sort(bank_idx[order[place < int(shots)]])


def probe_split(labels, holdout=1, shots=0):
    """-> (train indices, val indices, y_train, y_val, n_class): knn.holdout_split (bank = training set, queries = validation set), the
    identities that survive it re-indexed to 0..C-1, the training set cut to `shots` records per identity."""
    labels = np.asarray(labels).astype(np.int64).ravel()
    bank_i, query_i = knn.holdout_split(labels, n_holdout=holdout)
    if len(bank_i) == 0 or len(query_i) == 0:
        raise ValueError("linear probe: the hold-out split left no training or no validation rows")
    classes = np.unique(labels[bank_i])
    train_i = select_shots(labels, bank_i, shots)
    return train_i, query_i, np.searchsorted(classes, labels[train_i]), np.searchsorted(classes, labels[query_i]), len(classes)


def cosine_lr(base_lr, epoch, epochs):
    """torch.optim.lr_scheduler.CosineAnnealingLR(T_max=epochs, eta_min=0) stepped once per epoch, in closed form."""
    return 0.5 * base_lr * (1.0 + math.cos(math.pi * epoch / epochs))


def scaled_lr(lr, batch_size):
    """DINO's linear scaling rule: lr * batch_size / 256."""
    return lr * batch_size / 256.0


# --------------------------------------------------------------------------------------------------------------- the classifier
class _ProbeParams(torch.nn.Module):
    def __init__(self, weight, bias):
        super().__init__()
        self.weight = torch.nn.Parameter(weight)
        self.bias = torch.nn.Parameter(bias)


class LinearProbe:
    """nn.Linear(in_features, num_classes) trained by SGD on the device.  weight [C, F] ~ normal(0, 0.01) from a seeded CPU generator,
    bias zero; in the arena they are [Cp, Fp] and [Cp]: F zero-padded to the GEMM's K granule of 32, C to the 8 of the weight-gradient
    GEMM.  The pad rows and columns are zero, get zero gradients and stay zero.  Every buffer of a step is allocated once per batch
    size and reused, and the step makes no host round trip."""

    def __init__(self, in_features, num_classes, device, seed=0):
        self.F, self.C = int(in_features), int(num_classes)
        if self.F < 1 or self.C < 2:
            raise ValueError("LinearProbe: in_features >= 1 and num_classes >= 2 expected")
        self.Fp, self.Cp = _round_up(self.F, K_GRANULE), _round_up(self.C, N_GRANULE)
        self.device = torch.device(device)
        gen = torch.Generator()
        gen.manual_seed(int(seed))
        w = torch.zeros(self.Cp, self.Fp)
        w[:self.C, :self.F] = torch.empty(self.C, self.F).normal_(0.0, 0.01, generator=gen)
        self.params = _ProbeParams(w, torch.zeros(self.Cp))
        self.arena = ParamArena(self.params, self.device, with_grad=True, second_moment=False)
        a = self.arena
        self.w_bf16, self.b = a.bf("weight"), a.view(a.master, "bias")
        self.dW, self.db = a.view(a.grad, "weight", (self.Cp, self.Fp)), a.view(a.grad, "bias")
        self._hyper_host = torch.zeros(_lib.HP_COUNT, dtype=torch.float32)
        self._hyper_host[_lib.HP_MOMENTUM], self._hyper_host[_lib.HP_GRAD_SCALE] = MOMENTUM, 1.0       # wd, clip: 0
        self.hyper = self._hyper_host.to(self.device)
        self._buf = {}
        self.last_x_bf16 = self.last_dlogits = self.last_logits = self.last_y = None

    @property
    def weight(self):
        """The fp32 master weight [C, F] (a view of the arena)."""
        return self.params.weight.data[:self.C, :self.F]

    @property
    def bias(self):
        return self.params.bias.data[:self.C]

    def set_lr(self, lr):
        self._hyper_host[_lib.HP_LR] = float(lr)
        self.hyper.copy_(self._hyper_host)

    def _buffers(self, B, grad):
        key = (int(B), bool(grad))
        b = self._buf.get(key)
        if b is None:
            dev, f32 = self.device, torch.float32
            b = dict(xf=torch.empty(B, self.Fp, device=dev, dtype=f32), x=torch.empty(B, self.Fp, device=dev, dtype=torch.bfloat16),
                     logits=torch.empty(B, self.Cp, device=dev, dtype=f32), y=torch.empty(B, device=dev, dtype=torch.int32),
                     loss=torch.empty(B, device=dev, dtype=f32), rank=torch.empty(B, device=dev, dtype=torch.int32),
                     ws=ops.softmax_ce_rank_workspace(B, self.C, dev))
            if grad:
                b["dl"] = torch.empty(B, self.Cp, device=dev, dtype=torch.bfloat16)
            self._buf[key] = b
        return b

    def cache(self, feats, labels):
        """(features f32 [N + 1, Fp], labels i32 [N + 1]) on the device: the columns zero-padded to Fp, and one more row, all zero with
        label -1 -- the row the padding of a short batch points at."""
        feats = feats.to(self.device, torch.float32)
        if feats.dim() != 2 or feats.shape[1] != self.F:
            raise ValueError(f"LinearProbe: features [N, {self.F}] expected, got {tuple(feats.shape)}")
        N = feats.shape[0]
        y = torch.as_tensor(np.asarray(labels) if not torch.is_tensor(labels) else labels).to(torch.int64).flatten()
        if y.numel() != N:
            raise ValueError("LinearProbe: one label per feature row expected")
        fp = torch.zeros(N + 1, self.Fp, device=self.device, dtype=torch.float32)
        fp[:N, :self.F] = feats
        yp = torch.full((N + 1,), -1, device=self.device, dtype=torch.int32)
        yp[:N] = y.to(self.device, torch.int32)
        return fp, yp

    def _forward(self, b, rows):
        call("lafs_cast_bf16", _p(b["xf"]), _p(b["x"]), rows * self.Fp)
        ops.gemm_nt(b["x"][:rows], self.w_bf16, _lib.EPI_F32, bias=self.b, out=b["logits"][:rows])

    def step(self, cached, idx, n_target):
        """One SGD step on the rows `idx` (int64 [B] on the device) of cache()'s pair; n_target: how many of them have a target (the
        gradient is the mean over those).  Returns the row losses (f32 [B], a view of a reused buffer)."""
        fp, yp = cached
        B = idx.numel()
        b = self._buffers(B, True)
        torch.index_select(fp, 0, idx, out=b["xf"])                # data movement only
        torch.index_select(yp, 0, idx, out=b["y"])
        self._forward(b, B)
        ops.softmax_ce_rank(b["logits"], b["y"], self.C, 1.0 / max(int(n_target), 1), b["dl"], b["loss"], b["rank"], b["ws"])
        a = self.arena
        ops.zero_(a.grad)
        # one slice: every element of dW and db receives a single add, so the step is the same bits on every run
        ops.gemm_tn_acc(b["dl"], b["x"], self.dW, splits=1, colsum=self.db)
        call("lafs_clip_momentum_ema_range", _lib.UPDATE_SGD, _p(a.master), _p(a.grad), _p(a.exp_avg), None, _p(a.shadow), None,
             _p(a.chunk_seg), a.n_chunks, 0, a.n_chunks, _p(a.seg_flags), _p(a.seg_step), a.n_seg, 0, a.n_seg, _p(a.seg_sumsq), None,
             _p(self.hyper))
        self.last_x_bf16, self.last_dlogits, self.last_logits, self.last_y = b["x"], b["dl"], b["logits"], b["y"]
        return b["loss"]

    def fit(self, feats, labels, epochs=100, batch_size=1024, lr=0.001, seed=0):
        """SGD over the cached features: lr * batch_size / 256 at the start, cosine to 0, stepped once per epoch; a fresh permutation per
        epoch from a seeded generator; the short last batch padded with rows that have no target."""
        cached = self.cache(feats, labels)
        N, B = cached[0].shape[0] - 1, int(batch_size)
        if N < 1 or B < 1 or epochs < 1:
            raise ValueError("LinearProbe.fit: no rows, no batch or no epochs")
        base = scaled_lr(lr, B)
        gen = torch.Generator()
        gen.manual_seed(int(seed))
        n_pad = _round_up(N, B) - N
        for epoch in range(int(epochs)):
            self.set_lr(cosine_lr(base, epoch, epochs))
            perm = torch.cat([torch.randperm(N, generator=gen), torch.full((n_pad,), N, dtype=torch.int64)]).to(self.device)
            for i in range(0, N, B):
                self.step(cached, perm[i:i + B], min(B, N - i))
        return self

    def evaluate(self, feats, labels, batch_size=1024):
        """-> (top1 %, top5 %, mean loss) over the rows with a label in [0, C), from row_rank and row_loss; no gradient buffer."""
        fp, yp = self.cache(feats, labels)
        N = fp.shape[0] - 1
        B = min(int(batch_size), N)
        b = self._buffers(B, False)
        loss = torch.empty(N, device=self.device, dtype=torch.float32)
        rank = torch.empty(N, device=self.device, dtype=torch.int32)
        for i in range(0, N, B):
            n = min(B, N - i)
            b["xf"][:n].copy_(fp[i:i + n])
            self._forward(b, n)
            ops.softmax_ce_rank(b["logits"][:n], yp[i:i + n], self.C, 1.0, None, loss[i:i + n], rank[i:i + n], b["ws"])
        rank, loss = rank.cpu().numpy(), loss.double().cpu().numpy()
        if (rank == -2).any():
            raise ValueError(f"LinearProbe.evaluate: {int((rank == -2).sum())} labels lie outside [0, {self.C}) and are not -1")
        ok = rank >= 0
        if not ok.any():
            raise ValueError("LinearProbe.evaluate: no row has a label in [0, C)")
        n = int(ok.sum())
        return 100.0 * int((rank[ok] == 0).sum()) / n, 100.0 * int((rank[ok] < 5).sum()) / n, float(loss[ok].sum() / n)


# --------------------------------------------------------------------------------------------------------------- the evaluation
def evaluate_backbone(model, records, args=None, *, n_last_blocks=1, avgpool=False, epochs=100, batch_size=1024, lr=0.001, holdout=1,
                      shots=0, seed=0, norm=None, feature_batch=256, decode="pillow", num_workers=0, landmark_teacher=None, device=None):
    """The whole evaluation of one backbone, as knn.evaluate_backbone: features of every record once (record order), the per-identity
    hold-out split, identities re-indexed to 0..C-1, `shots` records per identity for training (0: all), fit, validate.  records:
    knn.load_records' pair.  -> {top1, top5, loss, train_top1, n_train, n_val, n_class}."""
    from .recordio import device_batches
    ds, labels = records
    device = torch.device(device if device is not None else ("cuda", torch.cuda.current_device()))
    if norm is None:
        norm = knn.view_norm(args)
    train_i, val_i, y_train, y_val, n_class = probe_split(labels, holdout, shots)
    if n_class < 2:
        raise ValueError("linear probe: fewer than two identities survive the hold-out split")
    batches = (u8 for u8, _ in device_batches(ds, feature_batch, device, num_workers=num_workers, shuffle=False, seed=0, drop_last=False,
                                              decode=decode))
    feats = probe_features(model, batches, n_last_blocks=n_last_blocks, avgpool=avgpool, norm=norm, landmark_teacher=landmark_teacher,
                           device=device)
    sel = lambda idx: feats[torch.from_numpy(idx).to(device)]
    f_train, f_val = sel(train_i), sel(val_i)
    probe = LinearProbe(feats.shape[1], n_class, device, seed=seed)
    probe.fit(f_train, y_train, epochs=epochs, batch_size=batch_size, lr=lr, seed=seed)
    top1, top5, loss = probe.evaluate(f_val, y_val)
    train_top1 = probe.evaluate(f_train, y_train)[0]
    return {"top1": top1, "top5": top5, "loss": loss, "train_top1": train_top1, "n_train": len(train_i), "n_val": len(val_i),
            "n_class": int(n_class)}


RESULT_KEYS = ("top1", "top5", "loss", "train_top1", "n_train", "n_val", "n_class")


def result_json(res):
    """The text of linear.json: a function of the result alone (a second run writes the same bytes)."""
    d = {k: (int(res[k]) if k.startswith("n_") else float(res[k])) for k in RESULT_KEYS}
    return json.dumps(d, sort_keys=True, indent=1) + "\n"
