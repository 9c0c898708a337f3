"""The arena and the case grid of tests/test_gpu_optim.py (lafs_grad_sumsq, lafs_clip_adamw_ema and their range forms), shared with
tests/test_oracle_rowops_host.py so that the CPU module judges exactly what the GPU runs."""
import torch

import fp64_bounds as fb
from fp64_bounds import CHUNK, SEG_DECAY, SEG_LAST_LAYER, SEG_LOW_DECAY, SEG_TRAINABLE, f32, f64
from gemm_cases import seed_of

# Tensors ragged at chunk boundaries: 4100 chunks take two trips of seg_sumsq_kernel's unrolled loop (8 x 256 chunks each) and a tail
CHUNKS = [1, 3, 1, 9, 2, 1, 4100, 2]
SHORT = [1000, 37, 5, 513, 1, 700, 333, 1023]            # elements the tensor's last chunk is short of (padding: zero in every buffer)
FLAGS = [SEG_DECAY | SEG_TRAINABLE, SEG_TRAINABLE, SEG_LOW_DECAY | SEG_TRAINABLE, SEG_DECAY | SEG_TRAINABLE,
         SEG_LOW_DECAY | SEG_DECAY | SEG_TRAINABLE, SEG_DECAY, SEG_LAST_LAYER | SEG_DECAY | SEG_TRAINABLE, SEG_TRAINABLE]
CLIP, GRAD_SCALE = 3.0, 0.5
# grad_scale x the gradient's norm per tensor: clipping bites on 1, 4, 6, 7 and not on 0, 3; tensor 2 sits on the knife edge
# (coefficient 1 to within its bound -- the only one); tensor 5 is not trainable
NORMS = [0.5, 8.0, None, 1.0, 20.0, 5.0, 7.0, 6.0]
KNIFE = 2
N_SEG, N_CHUNKS = len(CHUNKS), sum(CHUNKS)
GUARD = 2                                                # guard chunks (elements, for the per-tensor vectors) on both sides of every buffer
HYPER = dict(lr=5e-4, wd=0.04, beta1=0.9, beta2=0.999, eps=1e-8, ema=0.996, wd_low=0.02)


def opt_case(cid, step0, freeze, clip=CLIP, teacher=True, shadow=True):
    return dict(id=cid, step0=step0, freeze=freeze, clip=clip, teacher=teacher, shadow=shadow)


OPT_CASES = [opt_case("t1-frozen-last", 0, 1), opt_case("t2", 1, 0), opt_case("t1000-frozen-last", 999, 1), opt_case("t1", 0, 0),
             opt_case("clip-disabled", 1, 0, clip=0.0), opt_case("no-teacher", 1, 1, teacher=False), opt_case("no-shadow", 1, 0, shadow=False)]


def seg_starts():
    s = [0]
    for n in CHUNKS:
        s.append(s[-1] + n)
    return s


def hyper_vec(c):
    h = torch.zeros(16, dtype=f32)
    h[fb.HP_LR], h[fb.HP_WD], h[fb.HP_BETA1], h[fb.HP_BETA2], h[fb.HP_EPS] = HYPER["lr"], HYPER["wd"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"]
    h[fb.HP_CLIP], h[fb.HP_EMA_M], h[fb.HP_FREEZE_LAST], h[fb.HP_GRAD_SCALE], h[fb.HP_WD_LOW] = c["clip"], HYPER["ema"], c["freeze"], GRAD_SCALE, HYPER["wd_low"]
    return h


def arena_inputs(c):
    """The state of case c as fp64 CPU tensors of exactly representable fp32 values, [N_CHUNKS, 1024] each, padding zero: p, g, m, v,
    t (teacher); chunk_seg, flags, step (int32); hyper (fp32 [16]); mask (the logical elements)."""
    gen = torch.Generator()
    gen.manual_seed(seed_of("arena", c["id"]))
    rn = lambda: torch.randn(N_CHUNKS, CHUNK, generator=gen, dtype=f64)
    rf = lambda v: v.to(f32).double()
    st = seg_starts()
    chunk_seg = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(CHUNKS)])
    mask = torch.ones(N_CHUNKS, CHUNK, dtype=torch.bool)
    for i in range(N_SEG):
        mask[st[i + 1] - 1, CHUNK - SHORT[i]:] = False
    g = rn() * mask
    for i in range(N_SEG):
        seg = g[st[i]:st[i + 1]]
        # (the knife edge: clip / (norm + 1e-6) = 1; the fp32 rounding of the elements moves the norm by ~1e-8 of itself, the
        # coefficient's bound is ~1e-6)
        target = (CLIP - 1e-6 if NORMS[i] is None else NORMS[i]) / GRAD_SCALE
        seg *= target / seg.norm()
    p, t = 0.05 * rn(), 0.01 * rn()
    t = p + t
    m, v = 0.01 * rn(), (0.02 * rn()) ** 2
    if c["step0"] == 0:
        m, v = torch.zeros_like(m), torch.zeros_like(v)
    else:
        # sqrt(v) / sqrt(bc2) comparable to eps = 1e-8: a quarter chunk of tensor 3 without gradient
        a = st[3]
        g[a, :256] = 0
        v[a, :256] = 1e-16 * torch.rand(256, generator=gen, dtype=f64)
        m[a, :256] = 1e-9 * torch.randn(256, generator=gen, dtype=f64)
    d = {k: rf(x * mask) for k, x in (("p", p), ("g", g), ("m", m), ("v", v), ("t", t))}
    d.update(chunk_seg=chunk_seg, flags=torch.tensor(FLAGS, dtype=torch.int32), step=torch.full((N_SEG,), c["step0"], dtype=torch.int32),
             hyper=hyper_vec(c), mask=mask)
    return d


def expected(c, d, state=None):
    """(sumsq reference and bound, adamw_ema's dictionary) of one launch on d -- or on `state` (p, m, v, t, step of a previous launch)
    with d's gradients."""
    s = d if state is None else state
    hp = d["hyper"].double()
    ss, sse = fb.sumsq(d["g"], d["chunk_seg"], N_SEG, float(hp[fb.HP_GRAD_SCALE]))
    out = fb.adamw_ema(s["p"], d["g"], s["m"], s["v"], s["t"] if c["teacher"] else None, d["chunk_seg"], d["flags"], s["step"], ss, sse, hp)
    return (ss, sse), out
