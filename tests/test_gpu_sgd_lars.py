"""lafs_grad_sumsq_trust_range and lafs_clip_momentum_ema_range (csrc/optim.hip: --optimizer sgd / lars) against the fp64 restatement
of tests/sgd_lars_cases.py, element by element.

The arena is optim_cases' ragged one plus a decayed tensor with all-zero parameters and one with an all-zero gradient; every buffer
has guard chunks (guard elements for the per-tensor vectors) in front and behind, which must be bit-identical afterwards, and zero
padding, which must stay zero.  tests/test_sgd_lars_host.py shows on the CPU that the bounds mean something, that the restatement is
torch.optim.SGD / the reference's LARS, and that seeded faults fail."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from lafs_cvpr2024_amd import _lib  # noqa: E402
from lafs_cvpr2024_amd._lib import call  # noqa: E402

import fp64_bounds as fb  # noqa: E402
import sgd_lars_cases as sc  # noqa: E402
from fp64_bounds import CHUNK, bf16  # noqa: E402

DEV = "cuda"
G, N, S = sc.GUARD, sc.N_CHUNKS, sc.N_SEG
_INPUTS = {}
BY_ID = {c["id"]: c for c in sc.CASES}


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def inputs(c):
    """The case's CPU inputs, generated once (the 4.2 M-element arena is shared by the tests of a case id)."""
    if c["id"] not in _INPUTS:
        _INPUTS.clear()
        _INPUTS[c["id"]] = sc.arena_inputs(c)
    return _INPUTS[c["id"]]


class Arena:
    """Device buffers of a case: every per-element buffer is [G + N + G chunks], every per-tensor vector [G + S + G] elements, the three
    planes of chunk partials [G + 3 N + G]; `x[k]` is the view the kernels get, `buf[k]` the whole buffer."""

    def __init__(self, c, d):
        self.buf, self.x = {}, {}
        nan = float("nan")
        for k in ("p", "g", "m", "t"):
            self._add(k, d[k].flatten().float(), G * CHUNK, nan)
        self._add("pb", d["p"].flatten().to(bf16), G * CHUNK, nan)
        self._add("tb", d["t"].flatten().to(bf16), G * CHUNK, nan)
        self._add("chunk_seg", d["chunk_seg"], G, 0)
        self._add("chunk_part", torch.full((3 * N,), nan), G, nan)
        self._add("chunk_sumsq", torch.full((N,), nan), G, nan)
        self._add("flags", d["flags"], G, 0)
        self._add("step", d["step"], G, -77)
        self._add("sumsq", torch.full((S,), nan), G, nan)
        self._add("sumsq_adamw", torch.full((S,), nan), G, nan)
        self._add("trust", torch.full((S,), nan), G, nan)
        self.hyper = d["hyper"].to(DEV)
        self.c, self.lars = c, c["rule"] == "lars"
        self.guards = {k: self._guard(k) for k in self.buf}

    def _add(self, k, v, g, fill):
        b = torch.full((g + v.numel() + g,), fill, dtype=v.dtype, device=DEV)
        b[g:g + v.numel()] = v.to(DEV)
        self.buf[k], self.x[k] = b, b[g:g + v.numel()]

    def _guard(self, k):
        g = (self.buf[k].numel() - self.x[k].numel()) // 2
        return torch.cat([_bits(self.buf[k][:g]), _bits(self.buf[k][-g:])]).clone()

    def guards_intact(self, name):
        for k in self.buf:
            assert torch.equal(self._guard(k), self.guards[k]), f"{name}: a guard of `{k}` was written"

    def launch(self, lo=0, hi=S):
        """The kernel pair of the case's rule on the tensors [lo, hi)."""
        x, c, st = self.x, self.c, sc.seg_starts()
        if self.lars:
            call("lafs_grad_sumsq_trust_range", _p(x["p"]), _p(x["g"]), _p(x["chunk_seg"]), N, S, st[lo], st[hi], lo, hi, _p(x["flags"]), _p(self.hyper),
                 _p(x["chunk_part"]), _p(x["sumsq"]), _p(x["trust"]))
        else:
            call("lafs_grad_sumsq_range", _p(x["g"]), _p(x["chunk_seg"]), N, S, st[lo], st[hi], lo, hi, _p(self.hyper), _p(x["chunk_sumsq"]), _p(x["sumsq"]))
        t, tb = (x["t"], x["tb"]) if c["teacher"] else (None, None)
        call("lafs_clip_momentum_ema_range", sc.UPDATE[c["rule"]], _p(x["p"]), _p(x["g"]), _p(x["m"]), _p(t), _p(x["pb"] if c["shadow"] else None), _p(tb),
             _p(x["chunk_seg"]), N, st[lo], st[hi], _p(x["flags"]), _p(x["step"]), S, lo, hi, _p(x["sumsq"]), _p(x["trust"] if self.lars else None),
             _p(self.hyper))

    def state(self):
        """The kernel's own fp32 state, widened (the operands of its next launch)."""
        s = {k: self.x[k].double().view(N, CHUNK) for k in ("p", "m", "t")}
        s["step"] = self.x["step"].clone()
        return s

    def snapshot(self):
        return {k: _bits(b).clone() if b.is_floating_point() else b.clone() for k, b in self.buf.items()}


def judge(c, a, dd, state, before, name):
    """One launch pair of `a` (already run) against one fp64 step from `state`; `before`: the snapshot taken before it."""
    exp = sc.expected(c, dd, state)
    x = a.x
    worst = [fb.check(f"{name}: seg_sumsq", x["sumsq"], *exp["seg_sumsq"])[0]]
    if a.lars:
        worst.append(fb.check(f"{name}: seg_trust", x["trust"], *exp["seg_trust"])[0])
    assert torch.equal(x["step"].long(), exp["seg_step"]), f"{name}: seg_step {x['step'].tolist()}, expected {exp['seg_step'].tolist()}"
    V = lambda k: x[k].view(N, CHUNK)
    worst.append(fb.check(f"{name}: param", V("p"), *exp["param"])[0])
    worst.append(fb.check(f"{name}: mom", V("m"), *exp["mom"])[0])
    now = a.snapshot()
    if c["teacher"]:
        worst.append(fb.check(f"{name}: teacher", V("t"), *exp["teacher"])[0])
        fb.check(f"{name}: teacher_bf16", V("tb"), *exp["teacher16"], True)
    else:
        assert torch.equal(now["t"], before["t"]) and torch.equal(now["tb"], before["tb"]), f"{name}: teacher = NULL, yet a teacher buffer changed"
    upd_s = exp["seg_step"] != state["step"].long()
    if c["shadow"]:
        upd = upd_s[dd["chunk_seg"].long()][:, None]     # (a tensor that is not updated keeps its shadow as it was)
        ref, bound = exp["param16"]
        old = before["pb"][G * CHUNK:(G + N) * CHUNK].view(torch.bfloat16).view(N, CHUNK).double()
        fb.check(f"{name}: param_bf16", V("pb"), torch.where(upd, ref, old), torch.where(upd, bound, torch.zeros_like(bound)), True)
    else:
        assert torch.equal(now["pb"], before["pb"]), f"{name}: param_bf16 = NULL, yet the shadow changed"
    for k in ("g", "chunk_seg", "flags") + (() if a.lars else ("trust", "chunk_part")):
        assert torch.equal(now[k], before[k]), f"{name}: `{k}` was written"
    pad = ~dd["mask"]
    for k in ("p", "m", "t", "pb", "tb"):
        assert bool((V(k)[pad] == 0).all()), f"{name}: padding of `{k}` is no longer zero"
    # frozen and non-trainable tensors: bit-identical in param, mu, seg_step and the shadow, while their teacher still moves
    st = sc.seg_starts()
    skipped = [i for i in range(S) if not bool(upd_s[i])]
    assert skipped, "the arena has a non-trainable tensor"
    for i in skipped:
        sl = slice((G + st[i]) * CHUNK, (G + st[i + 1]) * CHUNK)
        for k in ("p", "m", "pb"):
            assert torch.equal(now[k][sl], before[k][sl]), f"{name}: tensor {i} takes no step, yet `{k}` changed"
        assert int(now["step"][G + i]) == int(before["step"][G + i])
        if c["teacher"]:
            assert not torch.equal(now["t"][sl], before["t"][sl]), f"{name}: the teacher of tensor {i} (no step) did not move"
    a.guards_intact(name)
    print(f"{name}: worst |err|/bound over the fp32 outputs {max(worst):.3f}")


@pytest.mark.parametrize("c", sc.CASES, ids=[c["id"] for c in sc.CASES])
def test_clip_momentum_ema(c):
    d = inputs(c)
    dd = {k: v.to(DEV) for k, v in d.items()}
    a = Arena(c, d)
    state, before = a.state(), a.snapshot()
    a.launch()
    torch.cuda.synchronize()
    judge(c, a, dd, state, before, c["id"])


def test_the_trust_reduction_writes_the_sumsq_of_grad_sumsq_range():
    """seg_sumsq of the LARS reduction is bit for bit that of lafs_grad_sumsq_range on the same gradients: the clip coefficient of a LARS
    step is that of an AdamW step."""
    c = BY_ID["lars-later"]
    a = Arena(c, inputs(c))
    x = a.x
    call("lafs_grad_sumsq_trust_range", _p(x["p"]), _p(x["g"]), _p(x["chunk_seg"]), N, S, 0, N, 0, S, _p(x["flags"]), _p(a.hyper), _p(x["chunk_part"]),
         _p(x["sumsq"]), _p(x["trust"]))
    call("lafs_grad_sumsq_range", _p(x["g"]), _p(x["chunk_seg"]), N, S, 0, N, 0, S, _p(a.hyper), _p(x["chunk_sumsq"]), _p(x["sumsq_adamw"]))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x["sumsq"]).all())
    assert torch.equal(_bits(x["sumsq"]), _bits(x["sumsq_adamw"])), (x["sumsq"].tolist(), x["sumsq_adamw"].tolist())
    assert torch.equal(_bits(x["chunk_part"][:N]), _bits(x["chunk_sumsq"])), "the g^2 plane is chunk_sumsq"
    a.guards_intact("sumsq equality")


@pytest.mark.parametrize("rule", ["sgd", "lars"])
def test_three_consecutive_launches(rule):
    """mu and seg_step carried over three launches, each against one fp64 step from the kernel's own previous fp32 state."""
    c = BY_ID[f"{rule}-t1-frozen-last"]
    d = inputs(c)
    dd = {k: v.to(DEV) for k, v in d.items()}
    a = Arena(c, d)
    for it in range(3):
        state, before = a.state(), a.snapshot()
        a.launch()
        torch.cuda.synchronize()
        judge(c, a, dd, state, before, f"{c['id']} launch {it + 1}")
    assert a.x["step"].tolist() == [3, 3, 3, 3, 3, 0, 0, 3, 3, 3]


@pytest.mark.parametrize("rule", ["sgd", "lars"])
def test_range_form_and_determinism(rule):
    """Updating the tensors [2, 5) leaves every buffer of the others -- their seg_trust and chunk partials too -- bit-identical and
    equals the whole-arena launch on those tensors bit for bit; two whole-arena launches on equal inputs are bitwise equal."""
    c = BY_ID[f"{rule}-later"]
    d = inputs(c)
    whole, again, part = Arena(c, d), Arena(c, d), Arena(c, d)
    start = whole.snapshot()
    lo, hi = 2, 5
    whole.launch(); again.launch(); part.launch(lo, hi)
    torch.cuda.synchronize()
    w, w2, p2 = whole.snapshot(), again.snapshot(), part.snapshot()
    st = sc.seg_starts()
    for k in whole.buf:
        assert torch.equal(w[k], w2[k]), f"two launches on equal inputs differ in `{k}`"
        n = whole.x[k].numel()
        if k == "chunk_part":                            # three planes of N chunks
            inside = torch.zeros(w[k].numel(), dtype=torch.bool, device=DEV)
            for plane in range(3):
                inside[G + plane * N + st[lo]:G + plane * N + st[hi]] = True
        else:
            unit = 1 if n in (S, N) else CHUNK
            a, b = ((G + lo), (G + hi)) if n == S else ((G + st[lo]) * unit, (G + st[hi]) * unit)
            inside = torch.zeros(w[k].numel(), dtype=torch.bool, device=DEV)
            inside[a:b] = True
        assert torch.equal(p2[k][inside], w[k][inside]), f"the range call differs from the whole-arena call inside its range in `{k}`"
        assert torch.equal(p2[k][~inside], start[k][~inside]), f"the range call wrote `{k}` outside its range"
    assert not torch.equal(p2["p"], start["p"]) and not torch.equal(p2["m"], start["m"])
    for a in (whole, again, part):
        a.guards_intact("range form")
    x = part.x
    with pytest.raises(_lib.LafsHipError, match="range outside the arena"):
        call("lafs_clip_momentum_ema_range", sc.UPDATE[rule], _p(x["p"]), _p(x["g"]), _p(x["m"]), None, None, None, _p(x["chunk_seg"]), N, 0, N + 1,
             _p(x["flags"]), _p(x["step"]), S, 0, S, _p(x["sumsq"]), _p(x["trust"]), _p(part.hyper))
