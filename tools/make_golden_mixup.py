#!/usr/bin/env python3
"""F25: the reference's whole mixing recipe (util/mixup_my.py Mixup: batch / pair / elem modes, mixup, CutMix from lambda and from
a min/max ratio, switching, label smoothing) and what the fine-tune loss makes of its dense targets (CosFace's soft-label branch,
face_pre_pro/ViT_face.py:69-73, and the soft-target CE of train_largescale.py:820), produced by running the REFERENCE itself.

Imports the reference exactly as tools/make_golden.py does.  Per case: the np.random seed, the reference class's arguments, the input
batch, the mixed batch and dense target it returns, the per-row lambdas its own _mix_* functions return under the same seed, the
np.random state it leaves behind, and loss / d loss/d cos / d loss/d input of its CosFace on an embedding batch with that target.
Data only; no reference source travels with the repository.

Usage:  python tools/make_golden_mixup.py   (rewrites tests/golden/f25_mixup_modes.npz deterministically)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _import_reference, save  # noqa: E402

B, S, C, D = 8, 16, 50, 32
# name: (mode, mixup_alpha, cutmix_alpha, cutmix_minmax, prob, switch_prob, smoothing, seed)
CASES = {
    "batch_mixup_s0": ("batch", 0.8, 0.0, None, 1.0, 0.5, 0.0, 101),
    "batch_cutmix_s1": ("batch", 0.0, 1.0, None, 1.0, 0.5, 0.1, 102),
    "batch_switch_s1": ("batch", 0.8, 1.0, None, 1.0, 0.5, 0.1, 103),
    "batch_switch_b_s0": ("batch", 0.8, 1.0, None, 1.0, 0.5, 0.0, 114),
    "batch_minmax_s0": ("batch", 0.0, 0.0, (0.2, 0.8), 1.0, 0.5, 0.0, 104),
    "pair_mixup_s1": ("pair", 0.8, 0.0, None, 1.0, 0.5, 0.1, 105),
    "pair_cutmix_s0": ("pair", 0.0, 1.0, None, 1.0, 0.5, 0.0, 106),
    "pair_switch_s1": ("pair", 0.8, 1.0, None, 1.0, 0.5, 0.1, 107),
    "pair_minmax_s1": ("pair", 0.8, 0.0, (0.2, 0.8), 1.0, 0.5, 0.1, 108),
    "elem_mixup_s0": ("elem", 0.8, 0.0, None, 1.0, 0.5, 0.0, 109),
    "elem_cutmix_s1": ("elem", 0.0, 1.0, None, 1.0, 0.5, 0.1, 110),
    "elem_switch_s1": ("elem", 0.8, 1.0, None, 1.0, 0.5, 0.1, 111),
    "elem_minmax_s0": ("elem", 0.8, 0.0, (0.3, 0.9), 1.0, 0.5, 0.0, 112),
    "elem_switch_p05_s1": ("elem", 0.8, 1.0, None, 0.5, 0.5, 0.1, 115),
}


def main():
    _, _, _, ref_face, ref_mix = _import_reference()
    torch.set_num_threads(4)
    torch.manual_seed(25)
    out = {"names": np.array(sorted(CASES))}
    cf = ref_face.CosFace(D, C, None, s=64.0, m=0.4)
    emb = torch.randn(B, D)
    out["weight"], out["emb"] = cf.weight.detach().clone(), emb.clone()
    for name in sorted(CASES):
        mode, ma, ca, mm, prob, sw, eps, seed = CASES[name]
        mk = lambda: ref_mix.Mixup(mixup_alpha=ma, cutmix_alpha=ca, cutmix_minmax=mm, prob=prob, switch_prob=sw, mode=mode,
                                   label_smoothing=eps, num_classes=C)
        x_in = torch.randn(B, 3, S, S)
        y = torch.randint(0, C, (B,))
        y[B - 2] = y[1]                                   # one row whose partner carries its own class
        np.random.seed(seed)
        x_out, target = mk()(x_in.clone(), y, device="cpu")
        state = np.random.get_state()
        np.random.seed(seed)                              # the lambdas the class itself hands to mixup_target
        lam = getattr(mk(), "_mix_" + mode)(x_in.clone())
        lam = torch.full((B,), float(lam), dtype=torch.float64) if not torch.is_tensor(lam) else lam.view(B).double()
        # CosFace.forward keeps the cosine as an intermediate (F.linear's output): retain its gradient while the reference runs
        e = emb.clone().requires_grad_(True)
        cf.weight.grad = None
        F, kept = torch.nn.functional, []
        linear = F.linear

        def keep_linear(*a, **k):
            o = linear(*a, **k)
            o.retain_grad()
            kept.append(o)
            return o
        F.linear = keep_linear
        try:
            logits = cf(e, target)
        finally:
            F.linear = linear
        ce = torch.sum(-target * F.log_softmax(logits, dim=-1), dim=-1).mean()      # timm SoftTargetCrossEntropy, train_largescale.py:820
        ce.backward()
        assert len(kept) == 1
        cos = kept[0]
        pre = "c." + name + "."
        out.update({pre + "cfg": np.array([ma, ca, -1.0 if mm is None else mm[0], -1.0 if mm is None else mm[1], prob, sw, eps, seed],
                                          dtype=np.float64),
                    pre + "x_in": x_in, pre + "y": y, pre + "x_out": x_out, pre + "target": target, pre + "lam": lam,
                    pre + "rng_keys": state[1].astype(np.uint32), pre + "rng_pos": np.int64(state[2]),
                    pre + "logits": logits.detach(), pre + "ce": ce.detach(), pre + "cos": cos.detach(), pre + "gcos": cos.grad, pre + "gemb": e.grad,
                    pre + "gweight": cf.weight.grad.clone()})
        print(f"  {name}: lam {lam.numpy().round(3)} target row sums {target.sum(1).numpy().round(6)[:3]} ce {ce.item():.5f}")
    save("f25_mixup_modes", **out)


if __name__ == "__main__":
    main()
