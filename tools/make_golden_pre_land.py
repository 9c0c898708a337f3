#!/usr/bin/env python3
"""Generate tests/golden/f28_pre_land.npz by running the REFERENCE's `pre_land` / `keep_land` fine-tune step (train_largescale.py:
565-582 the frozen stage-1 teacher, :807-843 the step) on the CPU in fp32, in the manner of tools/make_golden.py (whose import recipe
and helpers it uses).  Data only: arrays and names, no reference source.

Configuration: Part-fViT dim 128, depth 2, heads 3, mlp 256, 16 classes, CosFace, B = 2, hard labels, nn.CrossEntropyLoss, both models
in eval mode (BatchNorm running statistics, no dropout, DropPath off).
  * trunk weights: the seeded tensors tests/golden/f13_partfvit_land.npz already stores (the same configuration), + a seeded class
    table stored here;
  * the backbone's own landmark CNN (mode B): det_fill; the frozen teacher's CNN: det_fill_random (so that the two disagree);
  * the batch: uint8, stored; both sides feed x = u8 / 255 * 2 - 1.
Stored per weight w in {0, 1, 1000} (mode B, `pre_land and keep_land`): loss, the CNN gradients of the F13 selection, every gradient
norm; once: land_label, theta, loss_land, the trunk gradients of the F13 selection (the landmark term does not reach them).  Mode A
(`pre_land` alone, a backbone without a branch fed the '(p1 p2 c)' patch vectors of the teacher's mosaic): embedding, loss, trunk
gradients, norms.  The schedule table land_loss_control(epoch), epochs 0..40, comes from EXECUTING the reference's own if / elif lines.
A gradient tensor of more than 8192 values is stored as every `rowstep.<key>`-th row of its [-1, last dim] view (a committed file may
not exceed 1 MiB); its full norm is in the norm table.

Usage:  python tools/make_golden_pre_land.py
"""
import os
import sys
import textwrap

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

KEEP_TRUNK = ["patch_to_embedding.weight", "pos_embedding", "transformer.layers.0.0.fn.fn.to_qkv.weight"]
KEEP_CNN = ["output_layer.1.weight", "output_layer.1.bias", "stn.features.0.0.weight", "stn.features.15.conv.7.weight"]
WEIGHTS = (0.0, 1.0, 1000.0)
MAX_STORED = 8192


def thin(t):
    """(every step-th row of the [-1, last dim] view, step)."""
    step = max(1, -(-t.numel() // MAX_STORED))
    return t.reshape(-1, t.shape[-1])[::step].contiguous(), step


def reference_schedule(ref_dir, epochs):
    """land_loss_control for each epoch by executing the reference's own lines (the if / elif chain between the loss_land assignment
    and the `loss=loss+...` line of train_largescale.py)."""
    lines = open(os.path.join(ref_dir, "train_largescale.py")).read().splitlines()
    first = next(i for i, ln in enumerate(lines) if ln.strip().startswith("if 13>=epoch>7"))
    last = next(i for i in range(first, len(lines)) if lines[i].strip().startswith("loss=loss+land_loss_control"))
    code = compile(textwrap.dedent("\n".join(lines[first:last])), "<reference schedule>", "exec")
    out = []
    for epoch in epochs:
        env = {"epoch": epoch}
        exec(code, env)
        out.append(float(env["land_loss_control"]))
    return np.array(out, dtype=np.float64)


def main():
    _, _, _, ref_face, _ = MG._import_reference()
    sys.path.insert(0, os.path.dirname(MG.OUT))
    from conftest import det_fill, det_fill_random, load_golden, sub
    torch.set_num_threads(4)
    f13 = load_golden("f13_partfvit_land")
    cfg = dict(GPU_ID=None, num_class=16, image_size=112, patch_size=8, dim=128, depth=2, heads=3, mlp_dim=256, dropout=0.0, emb_dropout=0.0)
    torch.manual_seed(28)
    class_table = torch.randn(16, 128) * 0.05
    u8 = torch.randint(0, 256, (2, 3, 112, 112), dtype=torch.uint8)
    labels = torch.tensor([5, 11])
    x = u8.float() / 255 * 2 - 1
    crit = torch.nn.CrossEntropyLoss()
    mse = torch.nn.MSELoss()

    def backbone(with_land):
        m = ref_face.ViT_face_landmark_patch8(loss_type="CosFace", with_land=with_land, **cfg)
        trunk = dict(sub(f13, "p."))
        trunk["loss.weight"] = class_table
        missing, unexpected = m.load_state_dict(trunk, strict=False)
        assert not unexpected and all(k.startswith(("stn.", "output_layer.")) for k in missing), (missing, unexpected)
        if with_land:
            det_fill(m.stn); det_fill(m.output_layer)
        return m.eval()

    # the teacher as train_largescale.py:565-582 builds it (its trunk-shaped tensors are never used)
    teacher = ref_face.face_landmark_4simmin_glo_loc(loss_type="CosFace", GPU_ID=None, num_class=30000, num_patches=196, image_size=112,
                                                     patch_size=8, dim=512, depth=12, heads=11, mlp_dim=2560, dropout=0.1, emb_dropout=0.1)
    det_fill_random(teacher.stn); det_fill_random(teacher.output_layer)
    teacher.eval()
    with torch.no_grad():
        land_label, mosaic = teacher(x)                                            # :808

    out = dict(u8=u8, labels=labels, class_table=class_table, land_label=land_label, weights=np.array(WEIGHTS),
               schedule=reference_schedule(MG.REF, range(41)))
    # ---- mode B (:815-843, acc_step = 1)
    for w in WEIGHTS:
        m = backbone(True)
        outputs, pred_land = m(x, labels)
        loss = crit(outputs, labels)
        loss_land = mse(land_label / 111.0, pred_land / 111.0)
        loss = loss + w * loss_land
        loss.backward()
        g = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
        tag = f"w{w:g}."
        out[tag + "loss"] = loss.detach()
        out[tag + "gnorms"] = np.array([float(g[k].norm()) for k in sorted(g)])
        for k in KEEP_CNN:
            out[tag + "g." + k], out["rowstep." + k] = thin(g[k])
        if w == WEIGHTS[0]:
            out["theta"], out["loss_land"], out["gnorm_keys"] = pred_land.detach(), loss_land.detach(), np.array(sorted(g))
            for k in KEEP_TRUNK:
                out["g." + k], out["rowstep." + k] = thin(g[k])
    # ---- mode A (:811-812): the backbone without a branch takes the '(p1 p2 c)' patch vectors of the teacher's mosaic
    b, c, S, _ = mosaic.shape
    vec = mosaic.view(b, c, S // 8, 8, S // 8, 8).permute(0, 2, 4, 3, 5, 1).reshape(b, (S // 8) ** 2, 8 * 8 * c)
    m = backbone(False)
    emb = m(vec)
    outputs, _ = m(vec, labels)
    loss = crit(outputs, labels)
    loss.backward()
    g = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    out.update({"a.emb": emb.detach(), "a.loss": loss.detach(), "a.gnorm_keys": np.array(sorted(g)),
                "a.gnorms": np.array([float(g[k].norm()) for k in sorted(g)])})
    for k in KEEP_TRUNK + ["loss.weight"]:
        out["a.g." + k], out["rowstep." + k] = thin(g[k])
    MG.save("f28_pre_land", **{k: (np.asarray(v) if isinstance(v, int) else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
