"""python -m lafs_cvpr2024_amd.eval_linear --checkpoint ckpt.pth --data_path DIR: linear-probe accuracy of a lafs_train.py checkpoint.

The backbone is rebuilt from the checkpoint's own `args` and the `backbone.` keys of the chosen network (--checkpoint_key teacher |
student) are loaded strictly, as eval_knn does.  Every record of DIR/train.rec is embedded once in eval mode, the per-identity hold-out
split gives the training and the validation rows, and a linear classifier is trained on the frozen features by
lafs_cvpr2024_amd.linear_probe (--shots K: on the first K training records of every identity only).  One line is printed and
linear.json is written next to the checkpoint.  Single process."""
import argparse
import os

import torch

from . import knn, linear_probe
from .eval_knn import backbone_state_dict
from .utils import bool_flag

VIT_N_LAST_BLOCKS = 4                                     # DINO's eval_linear.py default for ViT-S


def get_args_parser():
    p = argparse.ArgumentParser("linear-probe evaluation of an SSL checkpoint on frozen features")
    p.add_argument("--checkpoint", required=True, type=str)
    p.add_argument("--checkpoint_key", default="teacher", type=str, choices=["teacher", "student"])
    p.add_argument("--data_path", required=True, type=str, help="directory with train.rec / train.idx")
    p.add_argument("--landmark_ckpt", default="", type=str,
                   help="state_dict of the frozen landmark CNN (--arch mynet); default: the checkpoint's own --landmark_ckpt")
    p.add_argument("--n_last_blocks", default=None, type=int,
                   help="cls tokens of the n last blocks are concatenated (default: 4 for the DINO ViTs, 1 for --arch mynet / fvit, "
                        "which take nothing else)")
    p.add_argument("--avgpool_patchtokens", default=False, type=bool_flag,
                   help="append the mean of the last block's patch tokens (DINO ViTs only)")
    p.add_argument("--epochs", default=100, type=int)
    p.add_argument("--lr", default=0.001, type=float, help="scaled by batch_size / 256, then cosine to 0 over the epochs")
    p.add_argument("--batch_size", default=1024, type=int)
    p.add_argument("--holdout", default=1, type=int, help="records per identity that become validation rows (the last ones)")
    p.add_argument("--shots", default=0, type=int, help="train on the first K records of every identity only (0: all)")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--max_images", default=0, type=int, help="use the first N records only (0: all)")
    p.add_argument("--decode", default="pillow", type=str, choices=["pillow", "device"])
    p.add_argument("--num_workers", default=4, type=int)
    return p


def resolve_n_last_blocks(args, arch):
    """--n_last_blocks as given, else the default of the checkpoint's arch: 1 for the face ViTs (mynet, fvit), 4 for the DINO ViTs."""
    if args.n_last_blocks is not None:
        return int(args.n_last_blocks)
    return 1 if arch in ("mynet", "fvit") else VIT_N_LAST_BLOCKS


def main(argv=None):
    args = get_args_parser().parse_args(argv)
    device = torch.device("cuda", torch.cuda.current_device())
    ck = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
    ca = ck["args"]
    n_last = resolve_n_last_blocks(args, ca.arch)
    if ca.arch in ("mynet", "fvit") and (n_last != 1 or args.avgpool_patchtokens):
        raise ValueError(f"--arch {ca.arch}: the probe takes the model's own output; --n_last_blocks > 1 and --avgpool_patchtokens are "
                         "defined for the DINO ViTs only")
    from .lafs_train import build_backbones, build_landmark_cnn
    backbone = build_backbones(ca)[1]                    # the teacher-side module (eval mode draws no DropPath either way)
    backbone.load_state_dict(backbone_state_dict(ck, args.checkpoint_key), strict=True)
    teacher = None
    if ca.arch == "mynet":
        teacher = build_landmark_cnn(args.landmark_ckpt or getattr(ca, "landmark_ckpt", "")).to(device).eval()
    records = knn.load_records(args.data_path, args.max_images)
    res = linear_probe.evaluate_backbone(backbone, records, args=ca, n_last_blocks=n_last, avgpool=args.avgpool_patchtokens,
                                         epochs=args.epochs, batch_size=args.batch_size, lr=args.lr, holdout=args.holdout,
                                         shots=args.shots, seed=args.seed, decode=args.decode, num_workers=args.num_workers,
                                         landmark_teacher=teacher, device=device)
    print(f"Linear probe: Top1 {res['top1']:.4f}, Top5 {res['top5']:.4f}, loss {res['loss']:.6f} "
          f"({res['n_class']} classes, {res['n_train']} / {res['n_val']})")
    out = os.path.join(os.path.dirname(os.path.abspath(args.checkpoint)), "linear.json")
    with open(out, "w") as f:
        f.write(linear_probe.result_json(res))
    return res


if __name__ == "__main__":
    main()
