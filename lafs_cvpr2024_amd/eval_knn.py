"""python -m lafs_cvpr2024_amd.eval_knn --checkpoint ckpt.pth --data_path DIR: weighted k-NN accuracy of a lafs_train.py checkpoint.

The backbone is rebuilt from the checkpoint's own `args` (arch, *_dims, fvit_window, patch_size), the `backbone.` keys of the chosen
network (--checkpoint_key teacher | student) are loaded strictly, every record of DIR/train.rec is embedded in eval mode, and the
per-identity hold-out split is classified by lafs_cvpr2024_amd.knn.  One line per k is printed and knn.json is written next to the
checkpoint.  Single process."""
import argparse
import os

import torch

from . import knn


def get_args_parser():
    p = argparse.ArgumentParser("weighted k-NN evaluation of an SSL checkpoint")
    p.add_argument("--checkpoint", required=True, type=str)
    p.add_argument("--checkpoint_key", default="teacher", type=str, choices=["teacher", "student"])
    p.add_argument("--data_path", required=True, type=str, help="directory with train.rec / train.idx")
    p.add_argument("--landmark_ckpt", default="", type=str,
                   help="state_dict of the frozen landmark CNN (--arch mynet); default: the checkpoint's own --landmark_ckpt")
    p.add_argument("--nb_knn", default="10,20,100,200", type=str)
    p.add_argument("--temperature", default=0.07, type=float)
    p.add_argument("--holdout", default=1, type=int, help="records per identity that become queries (the last ones)")
    p.add_argument("--max_images", default=0, type=int, help="use the first N records only (0: all)")
    p.add_argument("--batch_size", default=256, type=int)
    p.add_argument("--decode", default="pillow", type=str, choices=["pillow", "device"])
    p.add_argument("--num_workers", default=4, type=int)
    return p


def backbone_state_dict(checkpoint, key="teacher"):
    """The backbone's state dict out of a lafs_train.py checkpoint: network `key`, the DDP `module.` prefix dropped, the `backbone.`
    keys kept without their prefix (the DINO head's `head.` keys are left behind)."""
    if key not in checkpoint:
        raise KeyError(f"the checkpoint has no '{key}' (it holds {sorted(k for k in checkpoint if isinstance(k, str))})")
    out = {}
    for k, v in checkpoint[key].items():
        if k.startswith("module."):
            k = k[len("module."):]
        if k.startswith("backbone."):
            out[k[len("backbone."):]] = v
    if not out:
        raise KeyError(f"'{key}' holds no backbone.* keys")
    return out


def main(argv=None):
    args = get_args_parser().parse_args(argv)
    ks = knn.parse_ks(args.nb_knn)
    device = torch.device("cuda", torch.cuda.current_device())
    ck = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
    ca = ck["args"]
    from .lafs_train import build_backbones, build_landmark_cnn
    backbone = build_backbones(ca)[1]                    # the teacher-side module (eval mode draws no DropPath either way)
    backbone.load_state_dict(backbone_state_dict(ck, args.checkpoint_key), strict=True)
    teacher = None
    if ca.arch == "mynet":
        teacher = build_landmark_cnn(args.landmark_ckpt or getattr(ca, "landmark_ckpt", "")).to(device).eval()
    records = knn.load_records(args.data_path, args.max_images)
    res, n_bank, n_query = knn.evaluate_backbone(backbone, records, args=ca, ks=ks, temperature=args.temperature, holdout=args.holdout,
                                                 batch_size=args.batch_size, decode=args.decode, num_workers=args.num_workers,
                                                 landmark_teacher=teacher, device=device)
    print(f"k-NN on {args.data_path}: {n_bank} bank rows, {n_query} queries, T = {args.temperature}")
    for k, (t1, t5) in res.items():
        print(f"{k}-NN classifier result: Top1: {t1:.4f}, Top5: {t5:.4f}")
    out = os.path.join(os.path.dirname(os.path.abspath(args.checkpoint)), "knn.json")
    with open(out, "w") as f:
        f.write(knn.result_json(res, n_bank, n_query, args.temperature))
    return res


if __name__ == "__main__":
    main()
