#!/usr/bin/env python3
"""Generate tests/golden/f31_lars.npz by running the REFERENCE's own LARS optimizer (utils.py, `class LARS`).

Runs only where the read-only reference checkout is present (LAFS_REFERENCE, default /root/reference), like tools/make_golden.py.
The reference's utils.py pulls in packages a CPU-only container may lack, so the class is not imported: the source lines of
`class LARS` -- from its `class` line to the next top-level statement -- are exec'ed straight out of the reference file at run time,
and the parameter groups are built by the source lines of `get_params_groups` the same way.  Nothing of the reference is stored here
or in the fixture, which holds only numbers.

F31: four float64 tensors ([5, 7], [11], [2, 3, 4] and an all-zero [4, 4]) in a module whose parameter groups are those
get_params_groups makes (ndim != 1 and not a bias: regularised), three steps with given gradients and a different (lr, wd) per step as
the training loop sets them (lr on both groups, weight_decay on the first: lafs_train.py:514-517).  Step 1 has wd = 0 and a zero
gradient on the [5, 7] matrix, so ||d|| = 0 there; the all-zero matrix has ||p|| = 0 at step 0.  Recorded: the initial parameters, the
gradients and (lr, wd) of every step, the parameters and `mu` after every step."""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("LAFS_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "f31_lars.npz")
SHAPES = {"w57": (5, 7), "v11": (11,), "w234": (2, 3, 4), "z44": (4, 4)}
SCHEDULE = [(0.3, 0.04), (0.2, 0.0), (0.1, 0.4)]            # (lr, wd) per step


def grab(src, head):
    """The top-level block of the reference file that starts with `head`, up to the next top-level statement."""
    i = next(k for k, l in enumerate(src) if l.startswith(head))
    j = next((k for k in range(i + 1, len(src)) if src[k] and not src[k][0].isspace() and not src[k].startswith("#")), len(src))
    return "\n".join(src[i:j])


def main():
    src = open(os.path.join(REF, "utils.py")).read().split("\n")
    ns = {"torch": torch}
    exec(grab(src, "class LARS("), ns)
    exec(grab(src, "def get_params_groups("), ns)
    torch.manual_seed(31)
    model = torch.nn.Module()
    for name, shape in SHAPES.items():
        init = torch.zeros(shape, dtype=torch.float64) if name == "z44" else 0.5 * torch.randn(shape, dtype=torch.float64)
        model.register_parameter(name, torch.nn.Parameter(init))
    groups = ns["get_params_groups"](model)
    assert [len(g["params"]) for g in groups] == [3, 1], "get_params_groups: regularised = the tensors with ndim != 1"
    opt = ns["LARS"](groups)
    out = {f"p0.{n}": p.detach().numpy().copy() for n, p in model.named_parameters()}
    out["lr"], out["wd"] = np.array([s[0] for s in SCHEDULE]), np.array([s[1] for s in SCHEDULE])
    out["momentum"], out["eta"] = np.array(opt.defaults["momentum"]), np.array(opt.defaults["eta"])
    for it, (lr, wd) in enumerate(SCHEDULE):
        for i, g in enumerate(opt.param_groups):             # lafs_train.py:514-517
            g["lr"] = lr
            if i == 0:
                g["weight_decay"] = wd
        for n, p in model.named_parameters():
            p.grad = torch.randn(p.shape, dtype=torch.float64) * (3.0 if n == "w234" else 1.0)
            if it == 1 and n == "w57":
                p.grad.zero_()
            out[f"g{it}.{n}"] = p.grad.numpy().copy()
        opt.step()
        for n, p in model.named_parameters():
            out[f"p{it + 1}.{n}"] = p.detach().numpy().copy()
            out[f"mu{it + 1}.{n}"] = opt.state[p]["mu"].numpy().copy()
    np.savez(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    sys.exit(main())
