"""LFW / CFP-FP / AgeDB verification with the flip test (reference util/utils.py:27-65 load_bin / get_val_data, :292-397 perform_val,
util/verification.py evaluate / calculate_roc / calculate_accuracy) on the HIP kernels.

Per batch of B images (B even, so that a pair never straddles a batch), all on the device:

    u8 [B,3,S,S] -> lafs_eval_flip_normalize -> f32 [2B,3,S,S] (the batch, then the batch mirrored along W)
      -> (with_land) frozen-CNN inference plan (landmark_cnn.HipLandmarkCNN) on 2B rows -> lafs_landmark_theta (no jitter, no selection)
      -> lafs_patch_gather_fwd -> packed Part-fViT trunk (functional.vit_forward, save=False, no DropPath / dropout)
      -> lafs_verify_tail: per-copy norms (XNorm), e = emb(orig) + emb(flip) L2-normalised, dist = |e1 - e2|^2, all in fp64, and
         the histogram hist[fold][issame][k0] of k0 = #{k : t_k <= dist} over the 400 thresholds np.arange(0, 4, 0.01)

The pair counts with dist < t_k are prefix sums of that histogram, so every fold's TP / FP / TN / FN at every threshold, train and
test, follow on the host without a pass over the pairs per threshold; `metrics_from_hist` then makes calculate_roc's choices with the
same float operations (first maximum of the train accuracy, tpr / fpr = 0 on an empty class, np.mean over the folds).

fViT (ViTs_face_overlap, `--net VITs`) takes the same path without a landmark plan or a mosaic: the window geometry of its overlapping
embedding and, in the BatchNorm1d head, the running statistics (read, never written).

The model is evaluated as the reference's backbone.eval() runs it (BatchNorm running statistics, Dropout and DropPath off) without
touching the model's state: the CNN plan is rebuilt from the live weights and running statistics at every evaluation (the HIP training
plan of landmark_train.py updates the module's own running_mean / running_var tensors in place), nothing is written to the parameter
arena, the dropout counters and num_batches_tracked are not advanced, and `backbone.training` is left as it was.

Deliberate deviations from the reference:
  * the reference feeds its last partial batch UNSCALED (utils.py:361-363 skips `/255.0-0.5`); here every batch is scaled;
  * images that are not 112 x 112 are rejected instead of going through mxnet's resize_short (not available to restate);
  * JPEG / PNG decoding uses Pillow, as recordio.py does (the reference decodes with OpenCV through mxnet): PARITY UNPINNED;
  * the .bin file is unpickled by a restricted Unpickler that admits only lists, tuples, bytes, bools and numpy uint8 arrays;
  * data-parallel runs evaluate on every rank, each on a contiguous range of whole batches, and combine the histogram and the norm
    sums with one all_reduce each (the reference evaluates everything on rank 0).
The ROC image, tensorboard and calculate_val (VAL@FAR) are not computed.
"""
import argparse
import io
import os
import pickle
import time

import numpy as np
import torch
import torch.distributed as dist

from . import functional as Fn
from .ops import _p, call
from .vision_transformer import attach_arena

f32 = torch.float32
N_FOLDS = 10
THRESHOLDS = np.arange(0, 4, 0.01)                       # verification.py:294
# x -> x / div * mul + add, each operation rounded on its own (lafs_eval_flip_normalize)
NORMS = {"reference": (255.0, 1.0, -0.5),                # utils.py:314 `batch/255.0-0.5` as torch evaluates it on the CPU
         "train": (1.0, 2.0 / 255.0, -1.0)}              # the fine-tune feed, bit for bit as lafs_mixup_normalize computes it


# ----------------------------------------------------------------------------------------------------------------- data
class _BinUnpickler(pickle.Unpickler):
    """Admits lists, tuples, bytes and bools (pickle opcodes, no class lookup; protocol 2 spells bytes as _codecs.encode(str,
    'latin1')) and numpy arrays, whose dtype is checked afterwards."""
    _ALLOWED = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"), ("numpy", "ndarray"),
                ("numpy", "dtype"), ("_codecs", "encode")}

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"a verification .bin may not hold {module}.{name}")


def _read_bin(path):
    with open(path, "rb") as f:
        obj = _BinUnpickler(f, encoding="bytes").load()
    if not (isinstance(obj, (tuple, list)) and len(obj) == 2):
        raise ValueError(f"{path}: expected (bins, issame_list)")
    bins, issame = obj
    if isinstance(issame, np.ndarray) or not isinstance(issame, (list, tuple)) or not all(isinstance(v, bool) for v in issame):
        raise ValueError(f"{path}: issame_list must be a list of bools")
    if not isinstance(bins, (list, tuple)) or len(bins) != 2 * len(issame):
        raise ValueError(f"{path}: expected {2 * len(issame)} encoded images for {len(issame)} pairs")
    out = []
    for b in bins:
        if isinstance(b, np.ndarray):
            if b.dtype != np.uint8:
                raise ValueError(f"{path}: image arrays must be uint8, got {b.dtype}")
            b = b.tobytes()
        elif not isinstance(b, (bytes, bytearray)):
            raise ValueError(f"{path}: an encoded image is a {type(b).__name__}")
        out.append(bytes(b))
    return out, list(issame)


def load_bin(path, image_size=(112, 112)):
    """reference utils.py:27-46 -> (uint8 [2P,3,H,W] CPU tensor, bool [P] numpy array).  The mirrored copy the reference also keeps
    is made on the device (lafs_eval_flip_normalize)."""
    from PIL import Image
    bins, issame = _read_bin(path)
    H, W = image_size
    data = torch.empty(len(bins), 3, H, W, dtype=torch.uint8)
    for i, b in enumerate(bins):
        with Image.open(io.BytesIO(b)) as im:
            arr = np.asarray(im.convert("RGB"))
        if arr.shape[:2] != (H, W):
            raise ValueError(f"{path}: image {i} is {arr.shape[1]}x{arr.shape[0]}; only {W}x{H} images are supported "
                             "(the reference's resize_short is not restated)")
        data[i] = torch.from_numpy(arr.transpose(2, 0, 1).copy())
    return data, np.asarray(issame, dtype=bool)


def get_val_pair(path, name):
    ver_path = os.path.join(path, name + ".bin")
    if not os.path.exists(ver_path):
        raise FileNotFoundError(ver_path)
    return load_bin(ver_path)


def get_val_data(data_path, targets):
    """reference utils.py:57-64: [[name, uint8 images, issame], ...] for the comma-separated or listed targets."""
    if isinstance(targets, str):
        targets = [t for t in targets.split(",") if t]
    if not targets:
        raise ValueError("no verification targets")
    return [[t, *get_val_pair(data_path, t)] for t in targets]


# ----------------------------------------------------------------------------------------------------------------- metric
def fold_bounds(n_pairs, n_folds=N_FOLDS):
    """KFold(n_folds, shuffle=False): the first n_pairs % n_folds folds hold n_pairs // n_folds + 1 pairs.  -> int32 [n_folds + 1]."""
    if n_pairs < n_folds:
        raise ValueError(f"{n_pairs} pairs cannot be split into {n_folds} folds")
    sizes = np.full(n_folds, n_pairs // n_folds, dtype=np.int64)
    sizes[: n_pairs % n_folds] += 1
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def hist_from_dist(dist, issame, thresholds=THRESHOLDS, n_folds=N_FOLDS):
    """The histogram lafs_verify_tail accumulates, from host distances: int64 [n_folds, 2, n_thr + 1]."""
    dist = np.asarray(dist, dtype=np.float64)
    k0 = np.searchsorted(thresholds, dist, side="right")          # #{k : t_k <= dist}
    k0[np.isnan(dist)] = len(thresholds)
    fold = np.searchsorted(fold_bounds(len(dist), n_folds), np.arange(len(dist)), side="right") - 1
    hist = np.zeros((n_folds, 2, len(thresholds) + 1), dtype=np.int64)
    np.add.at(hist, (fold, np.asarray(issame, dtype=bool).astype(np.int64), k0), 1)
    return hist


def metrics_from_hist(hist, thresholds=THRESHOLDS):
    """calculate_roc (verification.py:38-87) from the histogram: (tpr [n_thr], fpr [n_thr], accuracy [n_folds], best_thresholds
    [n_folds]), each value produced by the same float operations as the reference's."""
    hist = np.asarray(hist, dtype=np.int64)
    n_folds, n_thr = hist.shape[0], len(thresholds)
    below = np.cumsum(hist, axis=2)[:, :, :n_thr]                  # [fold, class, k] pairs with dist < t_k
    total = hist.sum(axis=2)                                        # [fold, class]

    def counts(b, t):
        tp, fp = b[1], b[0]
        return tp, fp, t[0] - fp, t[1] - tp

    def rates(tp, fp, tn, fn):
        tpr = np.zeros(n_thr)
        fpr = np.zeros(n_thr)
        np.divide(tp.astype(np.float64), (tp + fn).astype(np.float64), out=tpr, where=(tp + fn) != 0)
        np.divide(fp.astype(np.float64), (fp + tn).astype(np.float64), out=fpr, where=(fp + tn) != 0)
        return tpr, fpr

    tprs, fprs = np.zeros((n_folds, n_thr)), np.zeros((n_folds, n_thr))
    accuracy, best_thresholds = np.zeros(n_folds), np.zeros(n_folds)
    all_below, all_total = below.sum(axis=0), total.sum(axis=0)
    for f in range(n_folds):
        tp, fp, tn, fn = counts(all_below - below[f], all_total - total[f])
        n_train = int((all_total - total[f]).sum())
        acc_train = (tp + tn).astype(np.float64) / n_train
        best = int(np.argmax(acc_train))
        best_thresholds[f] = thresholds[best]
        tp, fp, tn, fn = counts(below[f], total[f])
        tprs[f], fprs[f] = rates(tp, fp, tn, fn)
        accuracy[f] = float(tp[best] + tn[best]) / int(total[f].sum())
    return np.mean(tprs, 0), np.mean(fprs, 0), accuracy, best_thresholds


def evaluate(hist, norm_sum, norm_count, thresholds=THRESHOLDS):
    """perform_val's return values without the ROC image: (acc_mean, acc_std, xnorm, best_threshold_mean, tpr, fpr)."""
    tpr, fpr, accuracy, best_thresholds = metrics_from_hist(hist, thresholds)
    return accuracy.mean(), accuracy.std(), float(norm_sum) / float(norm_count), best_thresholds.mean(), tpr, fpr


# ----------------------------------------------------------------------------------------------------------------- device path
def landmark_plan(model, device, landmark_teacher=None):
    """The frozen-CNN inference plan of the landmark branch, built from the live weights and running statistics (None without one).
    landmark_teacher: the frozen stage-1 CNN of a `pre_land` fine-tune without `keep_land` (reference util/utils.py:326-334): used
    when the backbone has no branch of its own, so that such a model is validated on the feed it was trained on; a backbone with its
    own branch ignores it."""
    from .landmark_cnn import HipLandmarkCNN
    if getattr(model, "with_land", False):
        return HipLandmarkCNN(model, device)
    if landmark_teacher is not None and not getattr(model._spec, "overlapping", False):
        return HipLandmarkCNN(landmark_teacher, device)
    return None


@torch.no_grad()
def extract_features(model, arena, x, n, cnn, mosaic, device):
    """x f32 [2n,3,S,S] -> trunk embeddings f32 [2n, D] (eval mode); mosaic: f32 scratch [>= 2n,3,S,S] of the landmark branch.
    Shared by VerificationEvaluator and ijb_evaluation.IJBEvaluator."""
    S = x.shape[-1]
    img = x
    if cnn is not None:
        t = cnn(x)
        n_full = t.shape[1] // 2
        theta = torch.empty(2 * n, n_full, 2, device=device, dtype=f32)
        call("lafs_landmark_theta", _p(t), 2 * n, n_full, None, 0.0, None, n_full, _p(theta))
        img = mosaic[: 2 * n]
        call("lafs_patch_gather_fwd", _p(x), _p(theta), 2 * n, S, n_full, _p(img))
    side = img.shape[-1]
    # (fViT: the overlapping embedding's window geometry; its BatchNorm1d head runs on the running statistics, bn_training=False)
    geom = Fn.geometry([(2 * n, side)], device, window=model._spec.window if model._spec.overlapping else None)
    D = model._spec.trunk.dim
    pos = arena.view(arena.master, model._spec.prefix + model._spec.pos).view(-1, D)[: geom.npatch(0) + 1]
    feat, _, _ = Fn.vit_forward(arena, model._spec, geom, [img], [pos], None, save=False, dropout=None)
    return feat


class VerificationEvaluator:
    def __init__(self, backbone, batch_size, device=None, norm="reference", n_folds=N_FOLDS, landmark_teacher=None):
        """backbone: ViT_face_landmark_patch8 (with or without the landmark branch) or ViTs_face_overlap; batch_size: images per batch (even);
        norm: 'reference' (x/255 - 0.5, utils.py:314) or 'train' (x/255*2 - 1, the fine-tune feed); landmark_teacher: see landmark_plan."""
        if batch_size <= 0 or batch_size % 2:
            raise ValueError(f"the verification batch size must be even, got {batch_size}")
        if norm not in NORMS:
            raise ValueError(f"norm must be one of {sorted(NORMS)}")
        self.device = torch.device(device if device is not None else ("cuda", torch.cuda.current_device()))
        self.model, self.B, self.norm, self.n_folds = backbone, int(batch_size), norm, n_folds
        self.teacher = landmark_teacher
        self.arena = attach_arena(backbone, self.device)
        self.thr = torch.tensor(THRESHOLDS, dtype=torch.float64, device=self.device)
        self.keep_features = False                 # test hook: keep every batch's per-copy embeddings (self.features [2, 2P, D])
        self.features = None
        self._bufs = None

    def _buffers(self, S):
        if self._bufs is None or self._bufs["S"] != S:
            dev, B = self.device, self.B
            self._bufs = dict(S=S, u8=torch.empty(B, 3, S, S, device=dev, dtype=torch.uint8),
                              x=torch.empty(2 * B, 3, S, S, device=dev, dtype=f32),
                              mosaic=(torch.empty(2 * B, 3, S, S, device=dev, dtype=f32)
                                      if getattr(self.model, "with_land", False) or self.teacher is not None else None))
        return self._bufs

    def _landmark_plan(self):
        return landmark_plan(self.model, self.device, self.teacher)

    def _features(self, x, n, cnn):
        """x f32 [2n,3,S,S] -> trunk embeddings f32 [2n, D] (eval mode)."""
        return extract_features(self.model, self.arena, x, n, cnn, self._bufs["mosaic"], self.device)

    @torch.no_grad()
    def __call__(self, images, issame, engine=None):
        """images: uint8 [2P,3,S,S] (CPU or device), issame: bool [P] -> (acc_mean, acc_std, xnorm, best_threshold_mean, tpr, fpr).
        engine: the FinetuneEngine of a data-parallel run (its buffers are synchronised first); every rank must call this."""
        if engine is not None:
            engine.sync_buffers()
        issame = np.asarray(issame, dtype=bool)
        P = len(issame)
        if images.dim() != 4 or images.shape[0] != 2 * P or images.shape[1] != 3 or images.dtype != torch.uint8:
            raise ValueError(f"expected uint8 images [{2 * P}, 3, S, S]")
        S = images.shape[-1]
        dev, B, m = self.device, self.B, self.model
        m._arena.ensure_fresh()
        bufs = self._buffers(S)
        bounds = torch.tensor(fold_bounds(P, self.n_folds), device=dev)
        same = torch.tensor(issame.astype(np.uint8), device=dev)
        hist = torch.zeros(self.n_folds, 2, len(THRESHOLDS) + 1, device=dev, dtype=torch.int32)
        norms = torch.zeros(2, 2 * P, device=dev, dtype=torch.float64)
        D = m._spec.trunk.dim
        div, mul, add = NORMS[self.norm]
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
        n_batches = (2 * P + B - 1) // B
        lo, hi = n_batches * rank // world, n_batches * (rank + 1) // world
        self.features = torch.zeros(2, 2 * P, D, dtype=f32) if self.keep_features else None
        cnn = self._landmark_plan() if lo < hi else None
        for bi in range(lo, hi):
            i0 = bi * B
            n = min(B, 2 * P - i0)                                   # (even: 2P and B are)
            bufs["u8"][:n].copy_(images[i0:i0 + n])
            x = bufs["x"][: 2 * n]
            call("lafs_eval_flip_normalize", _p(bufs["u8"]), _p(x), n, S, div, mul, add)
            feat = self._features(x, n, cnn)
            call("lafs_verify_tail", _p(feat), D, n, D, i0 // 2, P, _p(self.thr), len(THRESHOLDS), _p(bounds), self.n_folds, _p(same),
                 _p(hist), _p(norms), None, None)
            if self.features is not None:
                self.features[0, i0:i0 + n] = feat[:n].cpu()
                self.features[1, i0:i0 + n] = feat[n:2 * n].cpu()
        n_mine = min(hi * B, 2 * P) - min(lo * B, 2 * P)             # images of this rank's batches; two embeddings each
        acc = torch.stack([norms.sum(), torch.tensor(2.0 * n_mine, device=dev, dtype=torch.float64)])
        if world > 1:
            dist.all_reduce(hist)
            dist.all_reduce(acc)
        acc = acc.cpu()
        self.last_hist = hist.cpu().numpy().astype(np.int64)
        return evaluate(self.last_hist, float(acc[0]), float(acc[1]))


def report(name, batch, result):
    """The reference's three lines per set (train_largescale.py:945-947)."""
    accuracy, std, xnorm, best_threshold = result[:4]
    print('[%s][%d]XNorm: %1.5f' % (name, batch, xnorm))
    print('[%s][%d]Accuracy-Flip: %1.5f+-%1.5f' % (name, batch, accuracy, std))
    print('[%s][%d]Best-Threshold: %1.5f' % (name, batch, best_threshold))


# ----------------------------------------------------------------------------------------------------------------- entry point
def main(argv=None):
    """Accuracy of a saved fine-tune checkpoint (the `module.`-prefixed state dict train_largescale.py writes) without training."""
    from . import train_largescale as tl
    p = argparse.ArgumentParser("Part-fViT / fViT verification", parents=[tl.get_args_parser()])
    p.add_argument("--checkpoint", required=True, type=str)
    args = p.parse_args(argv)
    if not args.val_path:
        raise SystemExit("--val_path is required")
    device = torch.device("cuda", torch.cuda.current_device())
    backbone = tl.build_backbone(args)
    sd = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    backbone.load_state_dict(sd)
    attach_arena(backbone, device)
    ev = VerificationEvaluator(backbone, args.val_batch_size or args.batch_size, device, norm=args.val_norm,
                               landmark_teacher=None if args.keep_land else tl.build_landmark_teacher(args))     # (a --pre_land checkpoint without a branch)
    for name, images, issame in get_val_data(args.val_path, args.target):
        t0 = time.time()
        res = ev(images, issame)
        report(name, 0, res)
        print(f"[{name}] {len(issame)} pairs in {time.time() - t0:.2f} s")


if __name__ == "__main__":
    main()
