"""Supervised Part-fViT + CosFace / ArcFace / AdaFace / PartialFC fine-tuning loop (reference train_largescale.py:317-963) on the HIP
fine-tune engine.  Model configuration as the reference builds it (:432, 542-557): with_land=True (trainable MobileNetV3
landmark branch), dropout = emb_dropout = 0.1, DropPath 0.1, CosFace(s=64, m=0.4) over all classes on every rank.
`--head PartialFC` / `--head ArcFace` select the class-sharded head of config C5 (parity unpinned, see partial_fc.py).
`--head AdaFace` (parity unpinned; Kim, Jain, Liu, CVPR 2022) trains the dense head with a margin per sample from the embedding's norm
(`--adaface_h`, `--adaface_t_alpha`); the progress line then shows the running norm statistics (`ada_mean`, `ada_std`).

Kept from the reference: flags that define the step (batch size, epochs, the lr rescale of :472
`acc_step/480 * lr * sqrt(world*bs/336) * 336`, weight decay 0.1 on >= 2-D tensors (:618-627; `--weight-decay` is parsed by the
reference but never reaches its optimizer), mixup alpha/prob, cutmix / cutmix-minmax / switch-prob / mixup-mode / smoothing (:383-395), acc_step=3 from supervised_config.py:37, warm-up(5 epochs)+cosine(eta_min 1e-6) LR, loading
`ckpt['teacher']` of an SSL checkpoint with the 'encoder.|backbone.|module.' prefixes stripped and strict=False).

Input: `--data recordio --data_path DIR` reads DIR/train.rec (MXNet RecordIO, InsightFace layout, recordio.FaceRecordDataset) with
the labels of its records, one pass over this rank's shard per epoch (lafs_train.epoch_shard: every rank runs the same number of
steps); `--data synthetic` feeds random uint8 batches and labels.  The reference's FaceDataset (image_iter.py:299-351, built at
train_largescale.py:506) is applied in its order: JPEG decode (Pillow on the CPU workers, or `--decode device`: one launch per
batch, jpeg.py, byte-identical) -> `--rand_mirror` -> channel reversal when
'ms1m' is not in the path (RecordIO only) -> `--rand_au` RandAugment (randaug.py) -> `--random_resizecrop` torchvision tensor
chain RandomResizedCrop / ColorJitter / RandomErasing (face_tensor_aug.py; PARITY UNPINNED (restated from torchvision 0.9.1;
torchvision is not installed)), all after the decode on the device.  With RecordIO the tensor chain's decisions are drawn in the
DataLoader workers next to the decode, from each worker's own torch generator, as the reference draws them.
Verification (`--val_path DIR`, off by default): the sets named by `--target` (DIR/<name>.bin) are evaluated with the flip test on the
reference's cadence (train_largescale.py:702-703, 925) -- after the optimizer step where (eval_step - 2) % (VER_FREQ // acc_step) == 1,
VER_FREQ = len(dataset) // (world * batch * 2) or `--ver_freq` -- printing XNorm, Accuracy-Flip and Best-Threshold per set (:945-947),
and rank 0 saves a `_checkpoint.pth` whenever need_save (:49-62, 955-959) says the accuracies improved (verification.py).  Cadence:
the divisor is clamped to >= 1 (the reference divides by zero on small datasets) and an evaluation happens at eval_step = 3, 3 + F,
3 + 2F, ...: the reference's test for every divisor F >= 3; with F = 2 the reference would also fire at eval_step 1 (Python's -1 % 2 == 1),
with F = 1 never.
`--net VITs` trains fViT (ViTs_face_overlap: overlapping 12/8/4 window embedding, BatchNorm1d head, no landmark branch) in the released
configuration instead of Part-fViT (`--net VIT_land_8`, the default): the reference's names (:324-326).
`--pre_land true` builds the frozen stage-1 landmark CNN of the reference (:565-582, weights from `--pretrain_path`): with
`--with_land false` its patches feed the trunk, with `--keep_land true` (and the backbone's own branch) it labels every batch and
`land_loss_control(epoch) * MSE` joins the loss (:825-836; `--land_loss_weight W` replaces the schedule by a constant), `loss_land` the
progress line (:914-915).
Out of scope here: tensorboard, IJB evaluation.
"""
import argparse
import math
import os
import time
from datetime import datetime

import numpy as np
import torch
import torch.distributed as dist

from . import utils
from .face_pre_pro.ViT_face import ViT_face_landmark_patch8, ViTs_face_overlap
from .finetune_engine import FinetuneEngine


def get_config(args):
    """The few supervised_config.py entries that define the step."""
    return dict(acc_step=3, SEED=1337, INPUT_SIZE=[112, 112], EMBEDDING_SIZE=768, WARMUP_EPOCH=5)


def get_args_parser():
    p = argparse.ArgumentParser("Part-fViT fine-tuning", add_help=False)
    p.add_argument("--net", "-n", default="VIT_land_8", type=str, choices=["VIT_land_8", "VITs"],
                   help="VIT_land_8: Part-fViT; VITs: fViT, the overlapping-patch face transformer with a BatchNorm1d head (reference :324-326)")
    p.add_argument("--batch_size", "-b", default=128, type=int)
    p.add_argument("--epochs", "-e", default=34, type=int)
    p.add_argument("--lr", default=1e-3, type=float, help="base rate before the reference's rescale (train_largescale.py:355,472)")
    p.add_argument("--weight_decay", default=0.1, type=float)
    p.add_argument("--head", default="CosFace", type=str, choices=["CosFace", "PartialFC", "ArcFace", "AdaFace"],
                   help="CosFace: the reference's dense head; ArcFace: dense head with the additive angular margin (m=0.5); "
                        "AdaFace: dense head whose margin adapts per sample to the embedding's norm (m=0.4); "
                        "PartialFC: class centres sharded over the ranks (config C5)")
    p.add_argument("--adaface_h", default=0.333, type=float, help="AdaFace: slope from the normalised embedding norm to the margin")
    p.add_argument("--adaface_t_alpha", default=0.01, type=float, help="AdaFace: EMA rate of the running norm mean / std")
    p.add_argument("--partial_margin", default="CosFace", type=str, choices=["CosFace", "ArcFace"])
    p.add_argument("--sample_rate", default=1.0, type=float, help="PartialFC negative-class sampling rate")
    p.add_argument("--with_land", default=True, type=utils.bool_flag, help="trainable landmark branch (reference :432)")
    p.add_argument("--pre_land", default=False, type=utils.bool_flag,
                   help="frozen stage-1 landmark CNN (reference :435, 565-582), loaded from --pretrain_path.  Alone (with --with_land false): "
                        "its patches feed the trunk, as in LAFS pre-training; with --keep_land: it labels every batch for the backbone's own branch")
    p.add_argument("--keep_land", default=False, type=utils.bool_flag,
                   help="landmark supervision (reference :437, 825-836): loss += land_loss_control(epoch) * MSE(teacher's landmarks / 111, "
                        "the backbone's / 111); needs --pre_land true and --with_land true")
    p.add_argument("--land_loss_weight", default=None, type=float,
                   help="a constant weight of the landmark term instead of the reference's schedule over the epochs (short runs)")
    p.add_argument("--dropout", default=0.1, type=float, help="dropout = emb_dropout of the reference (:552-555)")
    p.add_argument("--landmark_ckpt", default="", type=str, help="stn./output_layer. weights (reference :659-661)")
    p.add_argument("--num_class", default=205990, type=int)
    p.add_argument("--mixup", default=0.2, type=float)
    p.add_argument("--mixup-prob", dest="mixup_prob", default=0.1, type=float)
    p.add_argument("--cutmix", default=0.0, type=float, help="cutmix alpha, cutmix enabled if > 0 (reference :385)")
    p.add_argument("--cutmix-minmax", dest="cutmix_minmax", default=None, type=float, nargs=2, metavar=("MIN", "MAX"),
                   help="cutmix min/max box ratio, overrides alpha and enables cutmix if set (reference :387)")
    p.add_argument("--mixup-switch-prob", dest="mixup_switch_prob", default=0.5, type=float,
                   help="probability of switching to cutmix when both mixup and cutmix are enabled (reference :391)")
    p.add_argument("--mixup-mode", dest="mixup_mode", default="batch", type=str, choices=["batch", "pair", "elem"],
                   help="how to apply mixup/cutmix parameters: per batch, per pair of rows or per row (reference :393)")
    p.add_argument("--smoothing", default=0.0, type=float, help="label smoothing (reference :395); dense CosFace head only")
    p.add_argument("--drop_path", default=0.1, type=float)
    p.add_argument("--model_dir", default="", type=str, help="LAFS checkpoint whose ['teacher'] weights initialise the backbone")
    p.add_argument("--pretrain_path", default="", type=str, help="stage-1 checkpoint with the landmark CNN (alias of --landmark_ckpt)")
    p.add_argument("--data", default="synthetic", type=str,
                   help="'synthetic': random uint8 batches and labels; 'recordio': --data_path/train.rec (MXNet RecordIO, InsightFace "
                        "layout; JPEG decode on --num_workers CPU workers unless --decode device, everything after it on the device)")
    p.add_argument("--data_path", default="", type=str, help="directory holding train.rec / train.idx (--data recordio)")
    p.add_argument("--num_workers", default=6, type=int, help="DataLoader workers decoding RecordIO samples")
    p.add_argument("--decode", default="pillow", type=str, choices=["pillow", "device"],
                   help="--data recordio: 'pillow' decodes the JPEG records on the CPU workers; 'device' decodes each batch in one launch "
                        "(jpeg.DeviceJpegDecoder, byte-identical; records the device does not take still go through Pillow)")
    p.add_argument("--rand_au", default=False, type=utils.bool_flag,
                   help="RandAugment of the reference's FaceDataset (rand_au=True, train_largescale.py:506) on the device")
    p.add_argument("--rand_au_config", default="rand-m1-mstd0.5-inc1", type=str, help="config_str of train_largescale.py:506")
    p.add_argument("--rand_mirror", default=False, type=utils.bool_flag, help="FaceDataset's random horizontal flip (image_iter.py:308-311)")
    p.add_argument("--random_resizecrop", default=False, type=utils.bool_flag,
                   help="FaceDataset's torchvision tensor chain RandomResizedCrop(112, scale=(0.9, 1)) / ColorJitter(0.1, 0.1, 0.1, 0.1) / "
                        "RandomErasing(scale=(0.02, 0.1)) (image_iter.py:214-219, applied at :349-351) on the device; "
                        "PARITY UNPINNED (restated from torchvision 0.9.1; torchvision is not installed)")
    p.add_argument("--steps_per_epoch", default=100, type=int,
                   help="iterations per epoch for --data synthetic (with --data recordio an epoch is one pass over the rank's shard)")
    p.add_argument("--val_path", default="", type=str,
                   help="directory holding the verification sets <target>.bin; empty (the default): no verification")
    p.add_argument("--target", "-t", default="lfw,cfp_fp,agedb_30", type=str, help="verification targets (reference :329)")
    p.add_argument("--val_batch_size", default=0, type=int, help="images per verification batch (even; 0: --batch_size)")
    p.add_argument("--val_norm", default="reference", type=str, choices=["reference", "train"],
                   help="verification input scaling: 'reference' x/255 - 0.5 (utils.py:314), 'train' x/255*2 - 1 (the training feed)")
    p.add_argument("--ver_freq", default=0, type=int,
                   help="VER_FREQ in micro-batches (0: the reference's len(dataset) // (world * batch_size * 2), :718)")
    p.add_argument("--outdir", "-o", default=".", type=str)
    p.add_argument("--dist_url", default="env://", type=str)
    p.add_argument("--local_rank", default=0, type=int)
    return p


def need_save(acc, highest_acc):
    """reference train_largescale.py:49-62 (updates `highest_acc` in place)."""
    do_save = False
    save_cnt = 0
    if acc[0] > 0.98:
        do_save = True
    for i, accuracy in enumerate(acc):
        if accuracy > highest_acc[i]:
            highest_acc[i] = accuracy
            do_save = True
        if i > 0 and accuracy >= highest_acc[i] - 0.002:
            save_cnt += 1
    if save_cnt >= len(acc) * 3 / 4 and acc[0] > 0.99:
        do_save = True
    print("highest_acc:", highest_acc)
    return do_save


def ver_divisor(n_data, world, batch_size, acc_step, ver_freq=0):
    """VER_FREQ // acc_step (reference :718, 925) with VER_FREQ = n_data // (world * batch_size * 2) unless `ver_freq` > 0, clamped
    to >= 1."""
    vf = ver_freq if ver_freq > 0 else n_data // (world * batch_size * 2)
    return max(1, vf // acc_step)


def is_eval_step(eval_step, divisor):
    """Evaluate after the optimizer step that made the (never reset) optimizer-step counter `eval_step`: 3, 3 + F, 3 + 2F, ...
    -- `(eval_step - 2) % F == 1` of the reference (:925) for F >= 3 (see the module docstring for F < 3)."""
    return eval_step >= 3 and (eval_step - 3) % divisor == 0


def mixing_active(args):
    """timm's rule: mixing runs when any of mixup, cutmix or a cutmix min/max ratio is set.  The reference commented the last two
    out (train_largescale.py:526), so its `--mixup 0 --cutmix 1` silently trains unmixed; here it mixes."""
    return args.mixup > 0 or args.cutmix > 0.0 or args.cutmix_minmax is not None


def get_time():
    """reference util/utils.py:23-24."""
    return (str(datetime.now())[:-10]).replace(' ', '-').replace(':', '-')


def land_loss_control(epoch):
    """Weight of the landmark-supervision term over the 0-based epoch (reference train_largescale.py:825-834)."""
    if epoch < 8:
        return 1000
    if epoch < 14:
        return 100
    if epoch < 21:
        return 1
    if epoch < 28:
        return 0.11
    return 0


def check_net_args(args):
    """An argument error for flags that have no meaning with the chosen --net, and for the landmark-teacher modes that cannot run."""
    pre, keep = getattr(args, "pre_land", False), getattr(args, "keep_land", False)
    if args.net == "VITs" and (pre or keep):
        raise SystemExit("error: --pre_land / --keep_land feed or supervise landmark patches, which --net VITs does not embed")
    if args.net == "VITs" and (args.landmark_ckpt or args.pretrain_path):
        raise SystemExit("error: --landmark_ckpt / --pretrain_path load a landmark CNN, which --net VITs does not have")
    if keep and not pre:
        raise SystemExit("error: --keep_land regresses the backbone's landmarks onto the frozen CNN's: it needs --pre_land true")
    if pre and keep and not args.with_land:
        raise SystemExit("error: --pre_land true --keep_land true supervises the backbone's own landmark branch: it needs --with_land true")
    if pre and not keep and args.with_land:
        raise SystemExit("error: --pre_land true without --keep_land feeds the trunk the frozen CNN's patches: it needs --with_land false "
                         "(the reference's hard-coded with_land=True cannot run this combination either)")


def build_landmark_teacher(args):
    """The frozen stage-1 landmark CNN of --pre_land with the reference's constructor arguments (:565-571), its `stn.*` /
    `output_layer.*` tensors from --pretrain_path (:572-581), in eval mode; None without --pre_land."""
    if not getattr(args, "pre_land", False):
        return None
    check_net_args(args)
    from .face_pre_pro.ViT_face import face_landmark_4simmin_glo_loc
    teacher = face_landmark_4simmin_glo_loc(loss_type="CosFace", GPU_ID=None, num_class=30000, num_patches=196, image_size=112,
                                            patch_size=8, dim=512, depth=12, heads=11, mlp_dim=2560, dropout=0.1, emb_dropout=0.1)
    if args.pretrain_path:
        load_landmark_branch(teacher, args.pretrain_path)
    else:
        print("WARNING: --pre_land without --pretrain_path: the landmark teacher keeps its seeded initialisation")
    return teacher.eval()


def checkpoint_stem(args):
    """Backbone_<this>_Epoch_... : 'VIT' for Part-fViT (as before), 'VITs' for fViT."""
    return "VITs" if args.net == "VITs" else "VIT"


def build_backbone(args):
    """The fine-tune model of the reference (:432, 542-557) for these flags."""
    check_net_args(args)
    sharded = args.head == "PartialFC"
    loss_type = "None" if sharded else "AdaFace" if args.head == "AdaFace" else "CosFace"
    if args.net == "VITs":              # the released fViT configuration; --with_land is not read
        return ViTs_face_overlap(loss_type=loss_type, GPU_ID=None, num_class=args.num_class, image_size=112,
                                 patch_size=8, ac_patch_size=12, pad=4, dim=768, depth=12, heads=11, mlp_dim=2048,
                                 dropout=args.dropout, emb_dropout=args.dropout, drop_path_rate=args.drop_path)
    # the dense ArcFace head lives in the same `loss.weight` tensor as CosFace (the reference names an ArcFace class it never
    # defines, ViT_face.py:654-655); the margin is applied by the fused kernel
    return ViT_face_landmark_patch8(loss_type=loss_type, GPU_ID=None, num_class=args.num_class,
                                    image_size=112, patch_size=8, dim=768, depth=12, heads=11, mlp_dim=2048,
                                    dropout=args.dropout, emb_dropout=args.dropout, with_land=args.with_land,
                                    drop_path_rate=args.drop_path)


def warmup_cosine(base_lr, epoch_float, warmup_epochs, total_epochs, eta_min=1e-6):
    """GradualWarmupScheduler(multiplier=1) + CosineAnnealingLR (train_largescale.py:728-733); the `warmup_scheduler` package is
    not vendored by the reference, so this follows its documented behaviour (parity unpinned)."""
    if epoch_float < warmup_epochs:
        return base_lr * epoch_float / warmup_epochs
    t, T = epoch_float - warmup_epochs, max(total_epochs - warmup_epochs, 1)
    return eta_min + 0.5 * (base_lr - eta_min) * (1 + math.cos(math.pi * t / T))


def load_ssl_teacher(backbone, path, min_matched=0.9):
    """Initialise from ckpt['teacher'] with the 'encoder.' / 'backbone.' / 'module.' prefixes removed, strict=False
    (train_largescale.py:639-657).  Unlike the reference this refuses to continue silently from random weights: a tensor whose
    shape does not fit (e.g. a `loss.weight` of another class count) is dropped with a message, and fewer than `min_matched` of
    the backbone's trunk tensors being initialised is an error -- that is what a checkpoint of the wrong architecture (a DINO
    ViT teacher: keys blocks.N.attn.qkv..., pos_embed) looks like under strict=False."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd = ck.get("teacher", ck)
    own = backbone.state_dict()
    clean, dropped = {}, []
    for k, v in sd.items():
        if 'dummy_orthogonal_classifier' not in k:
            k = k.replace('encoder.', '').replace('backbone.', '').replace('module.', '')
        if k in own and tuple(own[k].shape) != tuple(v.shape):
            dropped.append((k, tuple(v.shape), tuple(own[k].shape)))
            continue
        clean[k] = v
    trunk = [k for k in own if not k.startswith(("loss.", "stn.", "output_layer."))]
    hit = [k for k in trunk if k in clean]
    for k, a, b in dropped:
        print(f"=> SSL teacher: skipping {k}: checkpoint {a} vs model {b}")
    if len(hit) < min_matched * len(trunk):
        arch = "fvit" if hasattr(backbone, "ac_patch_size") else "mynet"      # (--net VITs is ViTs_face_overlap: lafs_train.py --arch fvit)
        raise RuntimeError(f"{path}: only {len(hit)} of the backbone's {len(trunk)} trunk tensors are in ckpt['teacher'] "
                           f"(first missing: {[k for k in trunk if k not in clean][:3]}); is this a checkpoint of another architecture? "
                           f"LAFS pre-training must use --arch {arch} for its teacher to initialise this model")
    print(f"=> loaded SSL teacher: {len(hit)}/{len(trunk)} trunk tensors;", backbone.load_state_dict(clean, strict=False))


def load_landmark_branch(backbone, path):
    """load_part_checkpoint_landmark(pretrain_name=['stn', 'output']) (train_largescale.py:659-661): copy the tensors whose
    key starts with stn. / output_layer. from a stage-1 checkpoint."""
    sd = torch.load(path, map_location="cpu", weights_only=False)
    sd = sd.get("model", sd)
    part = {}
    for k, v in sd.items():
        k = k[len("module."):] if k.startswith("module.") else k
        if k.startswith(("stn.", "output_layer.")):
            part[k] = v
    print("=> landmark branch:", len(part), "tensors;", backbone.load_state_dict(part, strict=False))


class _WithTensorRecords:
    """FaceRecordDataset + one tensor-chain record per sample, drawn in the DataLoader worker that decodes it from that worker's
    own torch generator (seeded from the worker's torch seed, which the DataLoader derives from its base seed and the worker id),
    as the reference's torchvision transforms draw from each worker's torch RNG."""

    def __init__(self, ds, seed):
        self.ds, self.seed = ds, seed                  # `seed` only serves num_workers=0 (no worker seed to derive from)
        self._gen, self._pid = None, None

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, index):
        from .face_tensor_aug import sample_one
        item = self.ds[index]
        if len(item) == 3:              # undecoded (recordio.undecoded): the records need only H and W, which the plan carries
            buf, label, plan = item
            if plan is not None:
                H, W = plan.height, plan.width
            else:                       # not a stream the device takes: Pillow reads the size from the header
                import io
                from PIL import Image
                W, H = Image.open(io.BytesIO(buf)).size
        else:
            arr, label = item
            H, W = arr.shape[0], arr.shape[1]
        if self._gen is None or self._pid != os.getpid():
            worker = torch.utils.data.get_worker_info()
            self._gen = torch.Generator().manual_seed(worker.seed if worker is not None else self.seed)
            self._pid = os.getpid()
        rec = sample_one(self._gen, H, W)
        return (buf, label, plan, rec) if len(item) == 3 else (arr, label, rec)


class RecordIOFaces:
    """--data_path/train.rec -> (uint8 [B,3,H,W] device batch, int64 labels, tensor-chain records or None), one pass over this
    rank's shard per epoch (lafs_train.epoch_shard, DistributedSampler semantics: every rank gets len // world samples)."""

    def __init__(self, path, batch, device, seed, num_workers, rank, world, num_class, tensor_records=False, decode="pillow"):
        from .recordio import FaceRecordDataset
        rec = os.path.join(path, "train.rec")
        self.ds = FaceRecordDataset(rec)
        self.reverse_channels = "ms1m" not in rec      # image_iter.py:320
        self.all_seq = list(self.ds.seq)
        self.rank, self.world, self.seed = rank, world, seed
        self.per_rank = len(self.all_seq) // world
        self.batch, self.device, self.workers, self.num_class = batch, device, num_workers, num_class
        self.tensor_records = tensor_records
        if decode not in ("pillow", "device"):
            raise ValueError("decode must be 'pillow' or 'device'")
        self.decoder = None
        if decode == "device":
            from .jpeg import DeviceJpegDecoder
            self.decoder = DeviceJpegDecoder(device)
        self.epoch = 0
        self.set_epoch(0)
        print(f"Data loaded: there are {len(self.all_seq)} images ({self.per_rank} per rank).")

    def set_epoch(self, epoch):
        from .lafs_train import epoch_shard
        self.epoch = int(epoch)
        mine = epoch_shard(len(self.all_seq), self.rank, self.world, self.seed, self.epoch)
        self.ds.seq = [self.all_seq[i] for i in mine]

    def __len__(self):
        return self.per_rank // self.batch

    def __iter__(self):
        import numpy as np
        from .face_tensor_aug import RECORD
        g = torch.Generator().manual_seed(self.seed * 1000003 + self.rank * 1009 + self.epoch)
        from .recordio import undecoded
        base = undecoded(self.ds) if self.decoder is not None else self.ds
        ds = _WithTensorRecords(base, int(torch.randint(0, 2 ** 62, (1,), generator=g))) if self.tensor_records else base

        def collate(items):
            y = torch.tensor([it[1] for it in items], dtype=torch.int64)
            recs = np.stack([it[-1] for it in items]).astype(RECORD) if self.tensor_records else None
            if self.decoder is not None:                 # the bytes and their plans: decoded on the device below
                return ([it[0] for it in items], [it[2] for it in items]), y, recs
            x = torch.from_numpy(np.stack([it[0] for it in items])).permute(0, 3, 1, 2).contiguous()
            return x, y, recs

        loader = torch.utils.data.DataLoader(ds, batch_size=self.batch, shuffle=True, num_workers=self.workers, drop_last=True,
                                             collate_fn=collate, pin_memory=(torch.device(self.device).type == "cuda"), generator=g)
        for x, y, recs in loader:
            top = int(y.max()) if int(y.min()) >= 0 else int(y.min())
            if not 0 <= top < self.num_class:
                raise ValueError(f"{self.ds.rec.rec_path}: label {top} is outside [0, --num_class={self.num_class})")
            x = self.decoder(*x) if self.decoder is not None else x.to(self.device, non_blocking=True)
            yield x, y.to(self.device, non_blocking=True), recs


def verify(args, evaluator, engine, vers, highest_acc, backbone, epoch, batch):
    """Evaluate every set (on every rank), print the reference's lines on rank 0 and save a checkpoint when need_save says so
    (reference :925-959)."""
    main_proc = utils.is_main_process()
    if main_proc:
        print("Perform Evaluation on", [v[0] for v in vers], ", and Save Checkpoints...")
    acc = []
    for name, images, issame in vers:
        t = time.time()
        res = evaluator(images, issame, engine=engine)
        if main_proc:
            from .verification import report
            report(name, batch + 1, res)
            print(f"[{name}] {len(issame)} pairs evaluated in {time.time() - t:.2f} s")
        acc.append(res[0])
    if main_proc and need_save(acc, highest_acc):
        torch.save({"module." + k: v for k, v in backbone.state_dict().items()},
                   os.path.join(args.outdir, f"Backbone_{checkpoint_stem(args)}_Epoch_{epoch + 1}_Batch_{batch + 1}_Time_{get_time()}_checkpoint.pth"))


def main(args):
    check_net_args(args)
    utils.init_distributed_mode(args)
    cfg = get_config(args)
    utils.fix_random_seeds(cfg["SEED"])
    device = torch.device("cuda", args.gpu)
    world = utils.get_world_size()
    sharded = args.head == "PartialFC"
    arc = (args.partial_margin if sharded else args.head) == "ArcFace"
    ada = args.head == "AdaFace"
    backbone = build_backbone(args)
    if args.model_dir:
        load_ssl_teacher(backbone, args.model_dir)
    if (args.landmark_ckpt or args.pretrain_path) and (args.with_land or not args.pre_land):      # (mode A: the path is the teacher's)
        load_landmark_branch(backbone, args.landmark_ckpt or args.pretrain_path)
    teacher = build_landmark_teacher(args)
    head = None
    if sharded:
        from .partial_fc import PartialFC
        head = PartialFC(768, args.num_class, args.batch_size, sample_rate=args.sample_rate, s=64.0, m=0.5 if arc else 0.4,
                         margin_type=1 if arc else 0, device=device, seed=cfg["SEED"])
    engine = FinetuneEngine(backbone, args.batch_size, acc_step=cfg["acc_step"], mixup_alpha=args.mixup,
                            mixup_prob=args.mixup_prob if mixing_active(args) else 0.0,
                            s=64.0, m=0.5 if arc else 0.4, margin_type=2 if ada else 1 if arc else 0, device=device, sharded_head=head,
                            ada_h=args.adaface_h, ada_t_alpha=args.adaface_t_alpha,
                            cutmix_alpha=args.cutmix, cutmix_minmax=args.cutmix_minmax, switch_prob=args.mixup_switch_prob,
                            mix_mode=args.mixup_mode, label_smoothing=args.smoothing, landmark_teacher=teacher, keep_land=args.keep_land)
    # train_largescale.py:472:  lr = acc_step / 480 * lr * sqrt(world * BATCH_SIZE / 336) * 336
    base_lr = cfg["acc_step"] / 480.0 * args.lr * math.sqrt(world * args.batch_size / 336.0) * 336
    n_it = args.steps_per_epoch
    gen = torch.Generator(device=device).manual_seed(cfg["SEED"] + utils.get_rank())
    rand_au = None
    if args.rand_au:                    # the loader's per-sample PIL RandAugment as ONE launch per batch (randaug.py / csrc/randaug.hip)
        from .randaug import DeviceRandAugment
        rand_au = DeviceRandAugment(args.rand_au_config, {"translate_const": 117}, seed=cfg["SEED"] + utils.get_rank())
    tensor_aug = None
    if args.random_resizecrop:          # the torchvision tensor chain as ONE launch per batch (face_tensor_aug.py / csrc/face_tensor_aug.hip)
        from .face_tensor_aug import FaceTensorAug
        tensor_aug = FaceTensorAug(seed=cfg["SEED"] + utils.get_rank())
    data = None
    if args.data == "recordio":
        data = RecordIOFaces(args.data_path, args.batch_size, device, cfg["SEED"], args.num_workers, utils.get_rank(), world,
                             args.num_class, tensor_records=args.random_resizecrop, decode=args.decode)
        n_it = len(data)
        if n_it == 0:
            raise ValueError(f"{args.data_path}: {data.per_rank} images per rank are fewer than one batch of {args.batch_size}")
    vers, evaluator, highest_acc, divisor = None, None, None, None
    if args.val_path:
        from .verification import VerificationEvaluator, get_val_data
        vers = get_val_data(args.val_path, args.target)
        highest_acc = [0.0 for _ in vers]
        n_data = len(data.all_seq) if data is not None else args.steps_per_epoch * args.batch_size * world
        divisor = ver_divisor(n_data, world, args.batch_size, cfg["acc_step"], args.ver_freq)
        evaluator = VerificationEvaluator(backbone, args.val_batch_size or args.batch_size, device, norm=args.val_norm,
                                          landmark_teacher=teacher)
    eval_step = 0
    batch = 0
    t0 = time.time()
    for epoch in range(args.epochs):
        if data is not None:
            data.set_epoch(epoch)
        batches = iter(data) if data is not None else None
        for it in range(n_it):
            recs = None
            if batches is not None:
                x, y, recs = next(batches)
            else:
                x = torch.randint(0, 256, (args.batch_size, 3, 112, 112), device=device, dtype=torch.uint8, generator=gen)
                y = torch.randint(0, args.num_class, (args.batch_size,), device=device, generator=gen)
            if args.rand_mirror:        # _rd = random.randint(0, 1) per sample, flip along the width
                flip = torch.randint(0, 2, (args.batch_size, 1, 1, 1), device=device, generator=gen).bool()
                x = torch.where(flip, x.flip(3), x)
            if data is not None and data.reverse_channels:
                x = x.flip(1)           # image_iter.py:320-321: _data[::-1] on CHW when 'ms1m' is not in the path
            if rand_au is not None:
                x = rand_au(x)
            if tensor_aug is not None:
                x = tensor_aug(x, records=recs)
            lr = warmup_cosine(base_lr, epoch + it / n_it, cfg["WARMUP_EPOCH"], args.epochs)
            land_w = None
            if args.keep_land:
                land_w = land_loss_control(epoch) if args.land_loss_weight is None else args.land_loss_weight
            loss = engine.step(x, y, lr=lr, weight_decay=args.weight_decay, land_weight=land_w)
            if it % 50 == 0:
                land = f" loss_land {float(engine.loss_land.item()):.6f}" if args.keep_land else ""      # (reference :914-915)
                if ada:                 # the running norm statistics, read where loss.item() synchronises anyway
                    mean_std = engine.ada_state.tolist()
                    land += f" ada_mean {mean_std[0]:.4f} ada_std {mean_std[1]:.4f}"
                print(f"Epoch {epoch} it {it}/{n_it} loss {float(loss.item()):.4f} lr {lr:.3e} "
                      f"{(epoch * n_it + it + 1) * args.batch_size * world / (time.time() - t0):.1f} samples/s{land}")
            if engine.micro % cfg["acc_step"] == 0:      # an optimizer step ran (reference :893)
                eval_step += 1
                if evaluator is not None and is_eval_step(eval_step, divisor):
                    verify(args, evaluator, engine, vers, highest_acc, backbone, epoch, batch)
            batch += 1
        if utils.is_main_process():
            torch.save({"module." + k: v for k, v in backbone.state_dict().items()},
                       os.path.join(args.outdir, f"Backbone_{checkpoint_stem(args)}_Epoch_{epoch + 1}.pth"))    # IJB loader expects 'module.' (IJB_evaluation.py:126)
    if dist.is_initialized():
        dist.destroy_process_group()
