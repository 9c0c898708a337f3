"""Weighted k-NN evaluation of frozen features on the device (DINO's eval_knn.py protocol; no counterpart in the reference; the vote
restates DINO's knn_classifier formula: PARITY UNPINNED).

    features f32 [N, D], L2-normalised rows
      -> lafs_knn_search: per query the k bank rows with the largest float32 dot product (ties by position), the bank streamed in
         chunks that merge into the running result; the Q x N scores are never stored
      -> lafs_knn_vote: per k in `ks` each of the first k neighbours gives exp(score / T) to its identity; the five best identities
      -> top-1 / top-5 accuracy in percent

The evaluation set is a RecordIO face set (train.rec / train.idx) split per identity by `holdout_split`: the last `n_holdout` records
of an identity are queries, the rest is the bank.  `evaluate_backbone` is shared by `python -m lafs_cvpr2024_amd.eval_knn` and
`lafs_train.py --knn_freq`.

Deviations from DINO's script: no [B, k, C] one-hot table (the vote touches the k retrieved labels only, so the number of identities
does not matter); equal votes order by the smaller label; the images are not resized or centre-cropped (the face sets are 112 x 112).
"""
import json
import os

import numpy as np
import torch

from . import ops

MAX_K = 256
DEFAULT_KS = (10, 20, 100, 200)
DEFAULT_CHUNK_ROWS = 1 << 18


def l2_normalize(feats):
    """Rows divided by max(||row||_2, 1e-12) (torch.nn.functional.normalize, as DINO's script does once per feature table)."""
    return torch.nn.functional.normalize(feats.float(), dim=1, p=2)


def _aligned(x):
    """A contiguous float32 copy whose row stride is a multiple of 4 (lafs_knn_search's alignment rule); a view [N, D] of it."""
    x = x.float()
    N, D = x.shape
    if x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.stride(0) >= D and x.data_ptr() % 16 == 0:
        return x
    buf = torch.zeros(N, (D + 3) // 4 * 4, device=x.device, dtype=torch.float32)
    buf[:, :D] = x
    return buf[:, :D]


def knn_search(bank, query, k, exclude=None, chunk_rows=None, splits=0):
    """-> (top_score f32 [Q, k], top_idx i32 [Q, k]) of the whole bank, presented to lafs_knn_search `chunk_rows` rows at a time
    (merge).  The result does not depend on chunk_rows or splits, bit for bit.  exclude: int [Q] bank positions (-1: none)."""
    if bank.dim() != 2 or query.dim() != 2 or bank.shape[1] != query.shape[1] or bank.shape[0] == 0 or query.shape[0] == 0:
        raise ValueError("knn_search: bank [N, D] and query [Q, D] with N, Q > 0 expected")
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
    bank, query = _aligned(bank), _aligned(query)
    if exclude is not None:
        exclude = torch.as_tensor(exclude).to(bank.device, torch.int32).contiguous()
    step = int(chunk_rows or DEFAULT_CHUNK_ROWS)
    top_score = top_idx = None
    for r0 in range(0, bank.shape[0], step):
        top_score, top_idx = ops.knn_search(bank[r0:r0 + step], query, int(k), bank_pos0=r0, exclude=exclude, merge=r0 > 0, splits=splits,
                                            top_score=top_score, top_idx=top_idx)
    return top_score, top_idx


def knn_vote(top_score, top_idx, bank_labels, ks, temperature=0.07):
    """-> (pred i32, vote f32) [len(ks), Q, 5]: see ops.knn_vote."""
    labels = torch.as_tensor(bank_labels).to(top_score.device, torch.int32).contiguous()
    return ops.knn_vote(top_score, top_idx, labels, ks, temperature)


def filter_ks(ks, n_bank):
    """ks ascending without duplicates; an entry greater than the bank is dropped with a printed note."""
    keep = []
    for k in sorted(set(int(v) for v in ks)):
        if k < 1:
            raise ValueError(f"k must be positive, got {k}")
        if k > n_bank:
            print(f"k-NN: k = {k} dropped (the bank holds {n_bank} rows)")
        else:
            keep.append(k)
    return keep


def knn_classify(bank, bank_labels, query, query_labels, ks=DEFAULT_KS, temperature=0.07, chunk_rows=None, splits=0):
    """-> {k: (top1, top5)} in percent.  bank / query: L2-normalised feature rows on the device; labels: non-negative integers."""
    ks = filter_ks(ks, bank.shape[0])
    if not ks:
        return {}
    if ks[-1] > MAX_K:
        raise ValueError(f"k must be at most {MAX_K}, got {ks[-1]}")
    top_score, top_idx = knn_search(bank, query, ks[-1], chunk_rows=chunk_rows, splits=splits)
    pred, _ = knn_vote(top_score, top_idx, bank_labels, ks, temperature)
    y = torch.as_tensor(query_labels).to(pred.device, torch.int32).view(1, -1, 1)
    hit = (pred == y).cpu().numpy()                                   # [n_ks, Q, 5]; unused slots hold -1, labels are >= 0
    Q = hit.shape[1]
    return {k: (100.0 * int(hit[n, :, 0].sum()) / Q, 100.0 * int(hit[n].any(axis=1).sum()) / Q) for n, k in enumerate(ks)}


def holdout_split(labels, n_holdout=1, min_bank=1):
    """Deterministic bank / query split: per identity the last n_holdout records in record order are queries, the rest bank; an
    identity left with fewer than min_bank bank records contributes to neither.  -> (bank indices, query indices), int64, ascending."""
    labels = np.asarray(labels).astype(np.int64).ravel()
    if n_holdout < 1 or min_bank < 1:
        raise ValueError("n_holdout and min_bank must be at least 1")
    order = np.argsort(labels, kind="stable")                         # identities together, record order kept inside each
    sorted_l = labels[order]
    first = np.flatnonzero(np.r_[True, sorted_l[1:] != sorted_l[:-1]]) if len(labels) else np.zeros(0, np.int64)
    size = np.diff(np.r_[first, len(labels)])
    place = np.arange(len(labels)) - np.repeat(first, size)           # position of a record inside its identity
    n_bank = np.repeat(size - n_holdout, size)
    ok = n_bank >= min_bank
    return np.sort(order[ok & (place < n_bank)]), np.sort(order[ok & (place >= n_bank)])


# --------------------------------------------------------------------------------------------------------------- features
def view_norm(args):
    """(mean, std) per channel of the run that wrote `args`: --views dino scales with its --views_norm; --views lafs as the landmark
    front-end's views are scaled (0.5 / 0.5)."""
    from .augment import HALF_NORM, IMAGENET_NORM
    if getattr(args, "views", "lafs") == "dino" and getattr(args, "views_norm", "imagenet") == "imagenet":
        return IMAGENET_NORM
    return HALF_NORM


def _normalise(u8, mean, std):
    """ToTensor + Normalize(mean, std) with the operation order of the view kernels: (v / 255 - mean) / std in float32."""
    m = torch.tensor(mean, device=u8.device, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(std, device=u8.device, dtype=torch.float32).view(1, 3, 1, 1)
    return ((u8.float() / 255.0 - m) / s).contiguous()


@torch.no_grad()
def extract_bank(model, images_iter, norm=None, landmark_teacher=None, device=None):
    """Eval-mode features of a backbone over uint8 batches [B, 3, S, S] -> f32 [N, D] on the device (not normalised).
    Part-fViT and fViT go through verification.extract_features; a Part-fViT without a landmark branch (the `--arch mynet` teacher) is
    fed `landmark_teacher`'s mosaics, as a pre_land model is validated; the DINO VisionTransformer runs its own eval forward.  The
    module's training flag is restored; no parameter, buffer or random generator is touched."""
    from . import vision_transformer as vits
    from .augment import HALF_NORM
    from .verification import extract_features, landmark_plan
    mean, std = norm if norm is not None else HALF_NORM
    device = torch.device(device if device is not None else ("cuda", torch.cuda.current_device()))
    was_training = model.training
    model.eval()
    try:
        plain = isinstance(model, vits.VisionTransformer)
        arena = getattr(model, "_arena", None)
        if arena is None:
            arena = vits.attach_arena(model, device)
        arena.ensure_fresh()
        cnn = None if plain else landmark_plan(model, device, landmark_teacher)
        mosaic, feats = None, []
        for u8 in images_iter:
            u8 = u8.to(device)
            n = u8.shape[0]
            if n % 2 and not plain:                                   # extract_features takes an even number of rows
                u8 = torch.cat([u8, u8[-1:]])
            x = _normalise(u8, mean, std)
            if plain:
                f = model(x)
            else:
                if cnn is not None and (mosaic is None or mosaic.shape[0] < x.shape[0] or mosaic.shape[-1] != x.shape[-1]):
                    mosaic = torch.empty_like(x)
                f = extract_features(model, arena, x, x.shape[0] // 2, cnn, mosaic, device)
            feats.append(f[:n].float().clone())
        if not feats:
            raise ValueError("extract_bank: no images")
        return torch.cat(feats)
    finally:
        model.train(was_training)


def load_records(data_path, max_images=0):
    """(FaceRecordDataset over data_path/train.rec cut to its first max_images records, int64 labels in record order)."""
    from .recordio import FaceRecordDataset, unpack
    ds = FaceRecordDataset(os.path.join(data_path, "train.rec"))
    if max_images and max_images > 0:
        ds.seq = ds.seq[:int(max_images)]
    labels = np.empty(len(ds.seq), np.int64)
    for i, key in enumerate(ds.seq):
        lab = unpack(ds.rec.read_idx(key))[0].label
        labels[i] = int(lab if isinstance(lab, (int, float)) else lab[0])
    return ds, labels


def evaluate_backbone(model, records, args=None, norm=None, ks=DEFAULT_KS, temperature=0.07, holdout=1, batch_size=256, decode="pillow",
                      num_workers=0, landmark_teacher=None, device=None):
    """The whole evaluation of one backbone: features of every record (record order, nothing shuffled), the per-identity hold-out
    split, leave-the-queries-out k-NN.  records: load_records' pair.  -> ({k: (top1, top5)}, n_bank, n_query)."""
    from .recordio import device_batches
    ds, labels = records
    device = torch.device(device if device is not None else ("cuda", torch.cuda.current_device()))
    if norm is None:
        norm = view_norm(args)
    batches = (u8 for u8, _ in device_batches(ds, batch_size, device, num_workers=num_workers, shuffle=False, seed=0, drop_last=False,
                                              decode=decode))
    feats = l2_normalize(extract_bank(model, batches, norm=norm, landmark_teacher=landmark_teacher, device=device))
    bank_i, query_i = holdout_split(labels, n_holdout=holdout)
    if len(bank_i) == 0 or len(query_i) == 0:
        raise ValueError("k-NN evaluation: the hold-out split left no bank or no queries")
    sel = lambda idx: feats[torch.from_numpy(idx).to(device)]
    res = knn_classify(sel(bank_i), labels[bank_i], sel(query_i), labels[query_i], ks=ks, temperature=temperature)
    return res, len(bank_i), len(query_i)


def parse_ks(text):
    return tuple(int(v) for v in str(text).split(",") if v.strip())


def result_json(res, n_bank, n_query, temperature):
    """The text of knn.json: a function of the result alone (a second run writes the same bytes)."""
    d = {"n_bank": int(n_bank), "n_query": int(n_query), "temperature": float(temperature)}
    for k, (t1, t5) in res.items():
        d[f"knn_top1_k{k}"] = t1
        d[f"knn_top5_k{k}"] = t5
    return json.dumps(d, sort_keys=True, indent=1) + "\n"
