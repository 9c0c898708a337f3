"""CPU tests of the host-side logic (packing geometry, crop grouping, schedules, mixup, FLOP model)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from lafs_cvpr2024_amd import functional as Fn
from lafs_cvpr2024_amd.utils import MultiCropWrapper, cosine_scheduler
from oracle import optim as ooptim


def test_packed_geometry_two_resolution_groups():
    g = Fn.PackedGeometry(((4, 112), (6, 48)), 8, None)
    assert g.n_seq == 10 and g.n_tok == 4 * 197 + 6 * 37 and g.max_len == 197
    cu = g.cu_seqlens.tolist()
    assert cu[:5] == [0, 197, 394, 591, 788] and cu[-1] == g.n_tok and cu[5] == 788 + 37
    r2s = g.row2seq.tolist()
    assert r2s[0] == 0 and r2s[196] == 0 and r2s[197] == 1 and r2s[788] == 4 and r2s[-1] == 9
    assert g.tok_start == [0, 788] and g.seq_start == [0, 4] and g.npatch(0) == 196 and g.npatch(1) == 36


def test_multicrop_group_ends_matches_reference_rule():
    crops = [torch.zeros(2, 3, 112, 112)] * 2 + [torch.zeros(2, 3, 48, 48)] * 8
    assert MultiCropWrapper.group_ends(crops) == [2, 10]
    assert MultiCropWrapper.group_ends([torch.zeros(2, 196, 192)] * 2 + [torch.zeros(2, 36, 192)] * 3) == [2, 5]
    assert MultiCropWrapper.group_ends([torch.zeros(1, 3, 112, 112)]) == [1]


def test_cosine_scheduler_equals_reference_vectors():
    fx = load_golden("f6_schedules")
    np.testing.assert_allclose(cosine_scheduler(5e-4 * 64 / 256, 1e-6, 6, 11, warmup_epochs=2), fx["lr"].numpy(), rtol=1e-12)
    np.testing.assert_allclose(cosine_scheduler(0.996, 1, 6, 11), fx["mom"].numpy(), rtol=1e-12)
    np.testing.assert_allclose(cosine_scheduler(0.04, 0.4, 6, 11), ooptim.cosine_scheduler(0.04, 0.4, 6, 11), rtol=0)


def test_mixup_class_on_cpu_matches_reference():
    from lafs_cvpr2024_amd.util.mixup_my import Mixup
    fx = load_golden("f11_mixup")
    mix = Mixup(mixup_alpha=0.2, cutmix_alpha=0.0, prob=1.0, mode="batch", label_smoothing=0.0, num_classes=50)
    np.random.seed(11)
    x, t = mix(fx["x_in"].clone(), fx["y"], device="cpu")
    torch.testing.assert_close(x, fx["x_out"], rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(t, fx["target"], rtol=1e-6, atol=1e-7)


def test_bench_flop_model_matches_survey_numbers():
    import bench
    fl = bench.step_flops((384, 12, 6), 64, 8, 100000)
    assert abs(fl / 64 / 113.3e9 - 1) < 0.01            # 113.3 GFLOP per image


def test_finetune_lr_schedule_shape():
    from lafs_cvpr2024_amd.train_largescale import warmup_cosine
    assert warmup_cosine(1e-3, 0.0, 5, 34) == 0.0 and abs(warmup_cosine(1e-3, 5.0, 5, 34) - 1e-3) < 1e-12
    assert abs(warmup_cosine(1e-3, 34.0, 5, 34) - 1e-6) < 1e-12
    assert warmup_cosine(1e-3, 2.5, 5, 34) == ooptim.warmup_cosine_lr(1e-3, 2.5, 5, 34)


def test_partial_fc_shard_range_and_sampling():
    """PartialFC host logic (InsightFace partial_fc_v2 semantics): the shards tile the class range, positives always
    survive the negative sampling, and the remapped labels point at the right sampled centre."""
    from lafs_cvpr2024_amd.partial_fc import sample_classes, shard_range
    for C, W in ((10, 3), (2059906, 8), (7, 7), (100, 1)):
        spans = [shard_range(C, r, W) for r in range(W)]
        assert spans[0][0] == 0 and sum(n for _, n in spans) == C
        for (s0, n0), (s1, _) in zip(spans, spans[1:]):
            assert s0 + n0 == s1
    g = torch.Generator().manual_seed(0)
    labels = torch.tensor([5, 17, 17, 3, 40, 29, 11, 5])
    start, n_local = 10, 20                                   # this rank owns classes [10, 30)
    index, y = sample_classes(labels, start, n_local, 6, g)
    assert index.numel() == 6 and torch.equal(index, index.sort()[0]) and index.unique().numel() == 6
    own = (labels >= start) & (labels < start + n_local)
    assert torch.equal(y[~own], torch.full((int((~own).sum()),), -1, dtype=torch.int32))
    assert torch.equal(index[y[own].long()] + start, labels[own])
    # more positives than the sample budget: only the positives are kept
    index2, y2 = sample_classes(labels, start, n_local, 2, g)
    assert torch.equal(index2 + start, torch.tensor([11, 17, 29]))
    # sample_rate 1: identity
    index3, y3 = sample_classes(labels, start, n_local, n_local, g)
    assert torch.equal(index3, torch.arange(n_local)) and torch.equal(y3[own].long(), labels[own] - start)


def test_f15_checkpoint_layout_matches_reference_at_full_scale():
    """state_dict names AND shapes of the real configurations (ViT-S/8 + DINOHead(100000) student/teacher, DINOLoss, the
    with_land=True ViT-B fine-tune backbone with CosFace, the landmark CNN) equal the reference's: a checkpoint written by one
    side loads strictly on the other (lafs_train.py:451-460, train_largescale.py:639-661)."""
    import json
    import numpy as np
    import os
    from lafs_cvpr2024_amd import vision_transformer as vits
    from lafs_cvpr2024_amd.dino_loss import DINOLoss
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8, face_landmark_4simmin_glo_loc
    from lafs_cvpr2024_amd.utils import MultiCropWrapper
    path = os.path.join(os.path.dirname(__file__), "golden", "f15_checkpoint_manifests.npz")
    ref = json.loads(str(np.load(path, allow_pickle=False)["manifest"]))
    man = lambda m: {k: list(v.shape) for k, v in m.state_dict().items()}
    mine = {
        "student": man(MultiCropWrapper(vits.vit_small(patch_size=8, drop_path_rate=0.1),
                                        vits.DINOHead(384, 100000, use_bn=False, norm_last_layer=True))),
        "teacher": man(MultiCropWrapper(vits.vit_small(patch_size=8), vits.DINOHead(384, 100000, False))),
        "dino_loss": man(DINOLoss(100000, 10, 0.07, 0.04, 30, 41)),
        "finetune_backbone": man(ViT_face_landmark_patch8(loss_type="CosFace", GPU_ID=None, num_class=1000, image_size=112,
                                                          patch_size=8, dim=768, depth=12, heads=11, mlp_dim=2048, dropout=0.1,
                                                          emb_dropout=0.1, with_land=True)),
        "landmark_cnn": man(face_landmark_4simmin_glo_loc(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8,
                                                          dim=768, depth=12, heads=11, mlp_dim=2048)),
    }
    for name in ref:
        missing = sorted(set(ref[name]) - set(mine[name]))
        extra = sorted(set(mine[name]) - set(ref[name]))
        assert not missing and not extra, (name, missing[:5], extra[:5])
        bad = {k: (mine[name][k], v) for k, v in ref[name].items() if mine[name][k] != v}
        assert not bad, (name, dict(list(bad.items())[:5]))


def test_f12_finetune_weight_decay_groups_match_param_groups_lrd():
    """F12: the reference's own param_groups_lrd (train_largescale.py:122-173, exec'ed out of the reference file by
    tools/make_golden.py on a with_land Part-fViT) against finetune_decay_group: 1-D tensors 0, `stn*` matrices 5e-2, the rest 1e-1.
    (The per-group lr_scale = 0.58^k the reference also stores is recorded but never applied by torch.optim.AdamW.)"""
    import types
    from lafs_cvpr2024_amd.finetune_engine import LOW_WEIGHT_DECAY, finetune_decay_group
    fx = load_golden("f12_param_groups_lrd")
    wd_of = {"none": 0.0, "low": LOW_WEIGHT_DECAY, "decay": 1e-1}
    names = [str(n) for n in fx["names"]]
    assert len(names) == 185 and any(n.startswith("stn.") for n in names)
    for n, wd, nd in zip(names, fx["weight_decay"].tolist(), fx["ndim"].tolist()):
        p = types.SimpleNamespace(dim=lambda nd=nd: nd)
        assert wd_of[finetune_decay_group(n, p)] == pytest.approx(wd), (n, wd)
    assert {0.0, 0.05, 0.1} == {round(float(w), 6) for w in fx["weight_decay"].tolist()}


def test_recordio_epoch_shards_are_equal_disjoint_and_reshuffled():
    """Every rank must see the same number of samples per epoch (else the ranks run different step counts and the last all-reduce
    hangs) and the partition is re-drawn each epoch, like DistributedSampler.set_epoch (reference lafs_train.py:186-191, 440)."""
    from lafs_cvpr2024_amd.lafs_train import epoch_shard
    n, world = 1003, 8
    e0 = [epoch_shard(n, r, world, 7, 0) for r in range(world)]
    e1 = [epoch_shard(n, r, world, 7, 1) for r in range(world)]
    assert {len(s) for s in e0} == {n // world}
    flat = [i for s in e0 for i in s]
    assert len(set(flat)) == len(flat) == (n // world) * world
    assert e0[3] != e1[3] and sorted(i for s in e1 for i in s) != sorted(flat) or e0 != e1


def test_mynet_optimizer_index_order_is_the_reference_adamw_order():
    """checkpoint['optimizer'] of the reference's real configuration (--arch mynet): torch.optim.AdamW(get_params_groups(student))
    registers Part-fViT's CosFace `loss.weight` (requires_grad stays True in the reference, lafs_train.py:316-335, 385-392) in the
    regularised group although the SSL step never gives it a gradient (no state entry).  The engine freezes that tensor but must
    keep its index, or every later index shifts and a reference checkpoint cannot be resumed (and vice versa)."""
    import types
    from lafs_cvpr2024_amd.engine import LafsPretrainEngine
    from lafs_cvpr2024_amd.lafs_train import build_backbones
    from lafs_cvpr2024_amd.utils import get_params_groups
    from lafs_cvpr2024_amd.vision_transformer import DINOHead
    args = types.SimpleNamespace(arch="mynet", mynet_dims="64,2,2,128", mynet_dropout=0.1)
    sb, _, dim = build_backbones(args)
    student = MultiCropWrapper(sb, DINOHead(dim, 256, hidden_dim=64, bottleneck_dim=32, norm_last_layer=True))
    assert not sb.loss.weight.requires_grad                                  # frozen in the arena ...
    reg, noreg = LafsPretrainEngine._adamw_order(types.SimpleNamespace(student=student))
    assert "backbone.loss.weight" in reg                                      # ... but it keeps its index
    # the reference's view of the same model: loss.weight trainable, weight_g frozen by norm_last_layer
    sb.loss.weight.requires_grad_(True)
    groups = get_params_groups(student)
    by_id = {id(p): n for n, p in student.named_parameters()}
    assert [by_id[id(p)] for p in groups[0]["params"]] == reg
    assert [by_id[id(p)] for p in groups[1]["params"]] == noreg
    # a reference-style state_dict (no state for loss.weight) round-trips through torch's own loader with these group sizes
    opt = torch.optim.AdamW(groups)
    sd = opt.state_dict()
    assert [len(g["params"]) for g in sd["param_groups"]] == [len(reg), len(noreg)]


def test_gemm_route_selection_on_the_benchmark_shapes():
    """lafs_gemm_nt_route is host logic (no launch): which kernel form every long GEMM of the three measured workloads takes.
    0 = 128x128 tiles, 1 = K-resident, 3 = 128x384 wide tile (its tiles fit one round of the chip), 4 = 160-row tiles (one round of
    the 512 workgroup slots less than 128-row tiles would need), 5 = 192x256 tiles on one persistent workgroup per CU (plain epilogue,
    wide long-K shapes whose tiles fill whole rounds of the 256 CUs)."""
    import ctypes as C
    from lafs_cvpr2024_amd import _lib
    try:
        h = _lib.lib()
    except Exception as e:                                  # pragma: no cover
        pytest.skip(f"library not built: {e}")

    def route(M, N, K, epi, act=0):
        a = _lib.GemmNTArgs()
        a.M, a.N, a.K, a.epilogue, a.splits = M, N, K, epi, 1
        a.lda, a.ldb, a.ldc, a.ldc2, a.ldr, a.ldaux = K, K, N, N, N, N
        a.act = act
        a.A = a.B = a.C = a.C2 = a.resid = a.aux = 1 << 20          # (never dereferenced: the route is a function of shapes and presence)
        return int(h.lafs_gemm_nt_route(C.byref(a)))

    B16, GELU, RES, DG = _lib.EPI_BF16, _lib.EPI_BF16_GELU, _lib.EPI_RESID_F32, _lib.EPI_DGELU_BF16
    # ViT-S step (C2): two row chains of 25 216 / 18 944 rows
    assert route(25216, 1152, 384, B16) == 1 and route(18944, 1536, 384, GELU) == 1                  # K = 384: K-resident
    assert route(25216, 384, 1536, RES) == 3 and route(25216, 384, 1152, B16) == 3                    # 197 wide tiles: one round
    assert route(18944, 384, 1536, RES) == 0 and route(18944, 384, 1536, B16) == 0                    # 444 tiles: one round of 128x128
    assert route(44160, 384, 1536, B16) == 4                                                          # merged rows: 1035 -> 828 tiles
    # Part-fViT (ViT-B: C4 fine-tune at 25 216 rows, the mynet pair's chains)
    for epi, N, K in ((B16, 704, 768), (RES, 768, 2048), (RES, 768, 704), (GELU, 2048, 768)):
        assert route(25216, N, K, epi) == 4, (N, K, epi)                                              # 3 -> 2 / 7 -> 5 rounds
    assert route(25216, 768, 2048, B16) == 5 and route(25216, 768, 2112, B16) == 5                    # 160x256: 474 tiles = 1.85 rounds (K >= 1024)
    assert route(25216, 2112, 768, B16) == 5                                                          # 132 x 9 tiles of 192x256 = 4.6 rounds
    assert route(44160, 768, 2048, B16) == 5 and route(44160, 2112, 768, B16) == 5                    # merged rows: 753 / 2259 tiles of 176x256, 98 % full
    assert route(44160, 704, 768, B16) == 5
    # heavy epilogues (round 5: their operand loads batched in front of the stores): GELU' everywhere it fills the rounds, the
    # residual from three rounds on, the GELU pair that saves gelu'(u); the pair that writes u stays tiled
    assert route(44160, 2048, 768, DG) == 5 and route(25216, 2048, 768, DG) == 5
    assert route(44160, 768, 2048, RES) == 5 and route(44160, 768, 704, RES) == 5 and route(25216, 768, 2048, RES) == 4
    assert route(44160, 2048, 768, GELU, act=1) == 5 and route(25216, 2048, 768, GELU, act=1) == 5 and route(44160, 2048, 768, GELU) != 5
    assert route(18944, 768, 2048, B16) == 0                                                          # 888 tiles: 2 rounds either way
    assert route(1024, 768, 2048, B16) == 0


# ------------------------------------------------------------------------------------------------ lafs_gemm_nt's plan (host logic)
def _plan_lib():
    import os
    from lafs_cvpr2024_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):                   # pragma: no cover
        pytest.skip("library not built")
    return _lib, _lib.lib()                                 # (a library that is there but does not load is a failure, not a skip)


def _fake(off_bytes=0):
    return (1 << 20) + off_bytes                            # (never dereferenced: the plan reads shapes, strides, presence and alignment)


def _nt_args(_lib, M, N, K, epi, **kw):
    """A complete, contract-keeping request on fake 16-byte aligned pointers; kw overrides any field."""
    a = _lib.GemmNTArgs()
    a.M, a.N, a.K, a.epilogue, a.splits = M, N, K, epi, 1
    a.lda, a.ldb, a.ldc, a.ldc2, a.ldr, a.ldaux = K, K, N, N, N, N
    a.A = a.B = a.C = _fake()
    if epi == _lib.EPI_BF16_GELU:
        a.C2 = _fake()
    if epi == _lib.EPI_RESID_F32:
        a.resid = _fake()
    if epi == _lib.EPI_DGELU_BF16:
        a.aux = _fake()
    if epi == _lib.EPI_EMBED_F32:
        a.pos, a.npatch = _fake(), 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _plan(_lib, h, a):
    """(status, plan, route query) of one request."""
    import ctypes as C
    info = _lib.GemmNTPlanInfo()
    return int(h.lafs_gemm_nt_plan(C.byref(a), C.byref(info))), info, int(h.lafs_gemm_nt_route(C.byref(a)))


def _case_args(_lib, c, ctx):
    """The request tests/test_gpu_gemm.py builds for case c: column slices of wider buffers (gemm_cases.inp / Out), so every row
    stride exceeds the logical width and the bases sit 16 or 32 bytes into an aligned row."""
    import gemm_cases as gc
    M, N, K, epi = c["M"], c["N"], c["K"], c["epi"]
    ld = lambda off, w, pad: (off + w + pad + 7) // 8 * 8
    a = _lib.GemmNTArgs()
    a.M, a.N, a.K, a.epilogue, a.splits, a.act = M, N, K, epi, c["splits"], 1 if c["form"] == "save" else c["act"]
    a.A, a.B, a.lda, a.ldb = _fake(16), _fake(16), ld(8, K, 8), ld(8, K, 8)
    a.C, a.ldc = _fake(32 if epi in gc.F32_EPIS else 16), ld(8, N, 8)
    a.operand_f16 = 1 if c["half"] else 0
    if c["bias"]:
        a.bias = _fake()
    if c["drop_p"] > 0:
        a.drop_p, a.drop_seed, a.drop_row0 = c["drop_p"], 1, c["drop_row0"]
        a.drop_step = None if c["drop_step"] is None else _fake()
    if epi == gc.EPI_DGELU_BF16 or (epi == gc.EPI_BF16_ACT and c["aux"]):
        a.aux, a.ldaux = _fake(16), ld(8, N, 16)
    if epi == gc.EPI_RESID_F32:
        a.resid, a.ldr = (a.C, a.ldc) if c["alias"] else (_fake(16), ld(4, N, 4))
        if c["scale"] is not None:
            a.seq_scale, a.row2seq = _fake(), _fake()
    if epi == gc.EPI_EMBED_F32:
        a.pos, a.npatch = _fake(), c["npatch"]
    if epi == gc.EPI_BF16_GELU:
        a.C2, a.ldc2 = _fake(32), ld(16, N, 8)
        if c["form"] == "noC":
            a.C = None
    a.ctx = ctx
    return a


class _Contexts:
    """lafs_ctx handles by option set.  lafs_ctx_create needs a device: without one every non-default option set is None."""

    def __init__(self, h):
        self.h, self.made = h, {}

    def get(self, opts):
        key = tuple(sorted(opts.items()))
        if key not in self.made:
            ctx = self.h.lafs_ctx_create(0) if torch.cuda.is_available() else None
            for k, v in (opts.items() if ctx else ()):
                assert self.h.lafs_ctx_set(ctx, k, v) == 0
            self.made[key] = ctx
        return self.made[key]

    def close(self):
        for ctx in self.made.values():
            if ctx:
                self.h.lafs_ctx_destroy(ctx)


def test_gemm_plan_runs_the_route_and_instantiation_every_grid_case_names():
    """tests/test_gpu_gemm.py holds `every route and instantiation` to fp64: here the plan lafs_gemm_nt itself runs (lafs_gemm_nt_plan)
    is held to what each case id says it is meant for -- the route, and where the id ends in <WM,BK[,WN[,F16[,MB]]]> (defaults WN 2,
    F16 false, MB 4) the tile (WM*MB*16 x WN*64), the stage depth BK, the WM*WN*64 threads and the fp16 flag; a forced gemm_big
    geometry by its tile rows.  Cases with LAFS_OPT_* values need a context, which needs a device: without one they are passed over,
    30 of the grid's cases at the most (those whose `opts` is set) -- never a case on default options."""
    import re
    import gemm_cases as gc
    _lib, h = _plan_lib()
    ctxs = _Contexts(h)
    n_opts = sum(c["opts"] is not None for c in gc.NT_CASES)
    assert n_opts == 30
    passed_over, tagged = 0, 0
    try:
        for c in gc.NT_CASES:
            ctx = None
            if c["opts"] is not None:
                ctx = ctxs.get(c["opts"])
                if ctx is None:
                    passed_over += 1
                    continue
            rc, p, route = _plan(_lib, h, _case_args(_lib, c, ctx))
            assert rc == 0, (c["id"], rc, h.lafs_last_error())
            assert c["route"] is not None and p.route == route == c["route"], (c["id"], p.route, route)
            assert p.workgroups > 0 and p.workgroups % p.k_slices == 0, c["id"]
            assert p.k_slices == (len(gc.nt_slices(c["K"], c["splits"])) if c["epi"] in (gc.EPI_F32, gc.EPI_ATOMIC_F32) else 1), c["id"]
            tag = re.search(r"<([^>]*)>$", c["id"])
            if tag:
                assert c["route"] in (0, 3, 4), c["id"]         # (the tags name instantiations of the tiled kernel)
                t = tag.group(1).split(",") + ["2", "false", "4"][len(tag.group(1).split(",")) - 2:]
                wm, bk, wn, f16, mb = int(t[0]), int(t[1]), int(t[2]), t[3] == "true", int(t[4])
                got = (p.tile_m, p.tile_n, p.stage_k, p.threads, bool(p.f16))
                assert got == (wm * mb * 16, wn * 64, bk, wm * wn * 64, f16), (c["id"], got)
                tagged += 1
            forced = re.search(r"NT_BIG([2-5])", c["id"])
            if forced:
                assert (p.tile_m, p.tile_n) == ({2: 192, 3: 256, 4: 176, 5: 160}[int(forced.group(1))], 256), (c["id"], p.tile_m)
    finally:
        ctxs.close()
    assert passed_over <= n_opts and (passed_over == 0 or not torch.cuda.is_available())
    assert tagged >= 235                                    # (every tagged case on default options; 249 with a device)


def test_gemm_route_and_plan_refuse_what_lafs_gemm_nt_refuses():
    """Both queries run lafs_gemm_nt's own validation: every refusal gives the same negative code from both and sets lafs_last_error.
    The third request is the one the K-resident path used to launch (seq_scale read through a NULL row2seq): it is tested only here."""
    _lib, h = _plan_lib()
    F32, RES, GELU, B16 = _lib.EPI_F32, _lib.EPI_RESID_F32, _lib.EPI_BF16_GELU, _lib.EPI_BF16
    no_r2s = dict(seq_scale=_fake(), row2seq=None)
    cases = [
        ("K must be a multiple of 32", _nt_args(_lib, 128, 128, 48, B16)),
        ("null operand", _nt_args(_lib, 128, 128, 64, B16, A=None)),
        ("seq_scale needs row2seq", _nt_args(_lib, 2100, 192, 384, RES, **no_r2s)),              # K-resident shape
        ("seq_scale needs row2seq", _nt_args(_lib, 44160, 768, 2048, RES, **no_r2s)),            # gemm_big shape
        ("seq_scale needs row2seq", _nt_args(_lib, 257, 136, 96, RES, **no_r2s)),                # tiled shape
        ("GELU epilogue needs C2", _nt_args(_lib, 128, 128, 64, GELU, C2=None)),
        ("takes no bias", _nt_args(_lib, 128, 128, 128, F32, splits=2, bias=_fake())),
        ("fp16 operands", _nt_args(_lib, 128, 128, 64, RES, operand_f16=1)),
        ("drop_p must be in", _nt_args(_lib, 128, 128, 64, RES, drop_p=1.0)),
        ("ldc must be a multiple of 8", _nt_args(_lib, 128, 120, 64, B16, ldc=124)),
    ]
    import ctypes as C
    empty = _nt_args(_lib, 0, 128, 64, B16)
    for why, a in cases:
        # (the queries leave the text of an earlier refusal standing on success: a different refusal in front of each query, so that
        # the text read after it can only be its own)
        for query in (lambda r: h.lafs_gemm_nt_route(C.byref(r)), lambda r: h.lafs_gemm_nt_plan(C.byref(r), C.byref(_lib.GemmNTPlanInfo()))):
            assert query(empty) < 0 and "empty problem" in h.lafs_last_error().decode()
            rc = int(query(a))
            text = h.lafs_last_error().decode()
            assert rc == -2 and why in text and "empty problem" not in text, (why, rc, text)
    # the same shapes with row2seq are routed: the refusals above are about the missing operand, not the shapes
    with_r2s = dict(seq_scale=_fake(), row2seq=_fake())
    assert [_plan(_lib, h, _nt_args(_lib, M, N, K, RES, **with_r2s))[2] for M, N, K in ((2100, 192, 384), (44160, 768, 2048), (257, 136, 96))] == [1, 5, 0]
    # an unknown epilogue keeps its own code and text
    rc, _, route = _plan(_lib, h, _nt_args(_lib, 128, 128, 64, 11))
    assert rc == route == -1 and "unknown epilogue 11" in h.lafs_last_error().decode()


def test_gemm_route_equals_the_plans_route_on_random_requests():
    """lafs_gemm_nt_route has no logic of its own: on seeded random requests -- valid and broken, every epilogue, K splits, fp16, and
    option sets where a context can be made -- it returns the plan's route, or the plan's negative code."""
    import random
    _lib, h = _plan_lib()
    rnd = random.Random(20240611)
    ctxs = _Contexts(h)
    opt_sets = [{}, {_lib.OPT_KRES_MASK: 0}, {_lib.OPT_NT_WIDE: 0}, {_lib.OPT_NT_TALL: 0}, {_lib.OPT_NT_BIG: 0}, {_lib.OPT_NT_BIG: 3}, {_lib.OPT_NT_BIG: 5}]
    seen, refused = set(), 0
    try:
        for _ in range(600):
            M = rnd.choice([rnd.randint(1, 300), rnd.randint(1, 9000), rnd.choice([2048, 4096, 8192, 16400, 18944, 20500, 25216, 26048, 44160])])
            N = rnd.choice([rnd.randint(1, 2200), rnd.choice([64, 192, 384, 384, 384, 500, 512, 768, 1016, 1024, 1152, 1536, 2048, 2112])])
            K = rnd.choice([32 * rnd.randint(1, 70)] * 5 + [rnd.choice([96, 384, 512, 640, 704, 768, 1024, 1344, 1536, 2048])] * 10 + [48])
            epi = rnd.choice(list(range(8)) * 4 + [9])
            a = _nt_args(_lib, M, N, K, epi, ldc=(N + 7) // 8 * 8, ldc2=(N + 7) // 8 * 8, ldr=(N + 3) // 4 * 4, ldaux=(N + 7) // 8 * 8)
            a.splits = rnd.choice([1, 1, 2, 3, 1000]) if epi in (_lib.EPI_F32, _lib.EPI_ATOMIC_F32) else rnd.choice([1] * 9 + [2])
            a.operand_f16 = int(rnd.random() < 0.1)
            a.act = rnd.randint(0, 1) if epi in (_lib.EPI_BF16_GELU, _lib.EPI_DGELU_BF16) else rnd.randint(0, 4)
            a.drop_p = rnd.choice([0.0] * 8 + [0.1, 1.0])
            a.bias = rnd.choice([None, _fake()])
            if epi == _lib.EPI_RESID_F32:
                a.seq_scale, a.row2seq = rnd.choice([(None, None), (_fake(), _fake()), (_fake(), None)])
            if epi == _lib.EPI_BF16_GELU and rnd.random() < 0.3:
                a.C = None
            if rnd.random() < 0.1:                          # break one more thing
                setattr(a, *rnd.choice([("A", None), ("B", _fake(4)), ("lda", K + 4), ("C", _fake(8)), ("ldc", 124), ("drop_row0", -1), ("M", 0)]))
            a.ctx = ctxs.get(rnd.choice(opt_sets))
            rc, p, route = _plan(_lib, h, a)
            assert rc <= 0 and route == (p.route if rc == 0 else rc), (M, N, K, epi, rc, route, p.route)
            seen.add(route if rc == 0 else "refused")
            refused += rc < 0
    finally:
        ctxs.close()
    assert {0, 1, 3, 4, 5, "refused"} <= seen and 60 <= refused <= 300, (seen, refused)


# ------------------------------------------------------------------------------------------------ the trunk passes' plan (host logic)
_B14 = ((28, 197), (112, 37))                               # 2 x 14 global + 8 x 14 local crops: 5516 + 4144 token rows


def _trunk_desc(_lib, dim=384, mlp=1536, groups=_B14, n_groups=None, heads=None, ctx=None, **kw):
    """A contract-keeping trunk descriptor on fake pointers (never dereferenced: the plan reads shapes, options and presence)."""
    d = _lib.TrunkDesc()
    d.dim, d.heads, d.mlp, d.depth = dim, heads or dim // 64, mlp, 2
    d.inner = d.heads * 64
    d.n_seq, d.n_tok, d.max_len = sum(n for n, _ in groups), sum(n * l for n, l in groups), max(l for _, l in groups)
    d.cu_seqlens = d.row2seq = d.master = d.shadow = _fake()
    d._blocks = (_lib.BlockOffsets * 2)()
    d.blocks = d._blocks
    d.n_groups = len(groups) if n_groups is None else n_groups
    for gi, (n, l) in enumerate(groups[:d.n_groups]):
        d.group_n_seq[gi], d.group_max_len[gi] = n, l
    d.ctx = ctx
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _trunk_plan(_lib, h, d, save):
    import ctypes as C
    p = _lib.TrunkPlanInfo()
    rc = int(h.lafs_trunk_plan(C.byref(d), save, C.byref(p)))
    assert rc == 0, (rc, h.lafs_last_error())
    assert h.lafs_trunk_row_ranges(C.byref(d)) == p.n_ranges
    return p


def _rp(r, *names):
    return tuple(getattr(r, n) for n in (names or [n for n, _ in r._fields_]))


_PLACE = ("row0", "rows", "group", "seq0", "n_seq", "stream")
_FLAGS = ("fwd_fused", "fwd_ln2_inside", "fwd_next_ln1", "fwd_proj_inside", "bwd_fused", "bwd_ln2_inside")
_PARTS = ("ln1_parts", "ln2_parts")


def test_trunk_plan_without_a_context_one_case_per_rule():
    """lafs_trunk_plan is what lafs_trunk_forward / _backward run (csrc/engine.hip: plan).  With ctx == NULL it makes no HIP call:
    default options, no side streams -- hence ONE range even with two groups of 5516 and 4144 rows, and attention never forked."""
    _lib, h = _plan_lib()
    whole = (0, 9660, 0, 0, 140, 0)
    for save in (0, 1):
        # dim 384, mlp 1536, no dropout: fused forward (LayerNorm 2 inside, the next block's LayerNorm 1 written) and backward
        # (LayerNorm 2's backward launched); the projection stays a GEMM.  256 = the LayerNorm backward's cap of 4096 / 16 workgroups
        p = _trunk_plan(_lib, h, _trunk_desc(_lib), save)
        assert (p.n_ranges, p.attention, p.mlp_merged) == (1, _lib.ATTN_PER_GROUP, 0)
        assert _rp(p.range[0]) == _rp(p.whole) == whole + (1, 1, 1, 0, 1, 0) + (256, 256), _rp(p.range[0])
        # nothing fused: another width (12 heads; 8 rows per LayerNorm-backward workgroup: 4096 / 8 = 512 slots) ...
        p = _trunk_plan(_lib, h, _trunk_desc(_lib, dim=768, mlp=2048), save)
        assert _rp(p.range[0]) == _rp(p.whole) == whole + (0,) * 6 + (512, 512) and p.n_ranges == 1
        # ... element dropout ...
        p = _trunk_plan(_lib, h, _trunk_desc(_lib, dropout_p=0.1), save)
        assert _rp(p.range[0]) == whole + (0,) * 6 + (256, 256)
        # ... a hidden width above 1536 or below 128
        for mlp in (1600, 64):
            assert _rp(_trunk_plan(_lib, h, _trunk_desc(_lib, mlp=mlp), save).range[0], *_FLAGS) == (0,) * 6, mlp
        # the attention form: one launch over all sequences without groups or with one, else one per group on the caller's stream
        one = ((28, 197),)
        assert _trunk_plan(_lib, h, _trunk_desc(_lib, n_groups=0), save).attention == _lib.ATTN_ONE_LAUNCH
        assert _trunk_plan(_lib, h, _trunk_desc(_lib, groups=one), save).attention == _lib.ATTN_ONE_LAUNCH
        p = _trunk_plan(_lib, h, _trunk_desc(_lib, groups=one), save)
        assert _rp(p.range[0], *_PLACE) == (0, 5516, 0, 0, 28, 0) and _rp(p.range[0], *_FLAGS) == (1, 1, 1, 0, 1, 0)
        assert _trunk_plan(_lib, h, _trunk_desc(_lib), save).attention == _lib.ATTN_PER_GROUP


def test_trunk_queries_refuse_what_the_passes_refuse():
    """Every refusal of the descriptor check comes back from lafs_trunk_plan (-2), lafs_trunk_row_ranges (-1) and
    lafs_trunk_workspace_bytes (-1) alike, with its text."""
    import ctypes as C
    _lib, h = _plan_lib()
    g1 = _trunk_desc(_lib)
    g1.group_n_seq[1] = 0
    g2 = _trunk_desc(_lib)
    g2.group_max_len[0] = 198
    cases = [
        ("null descriptor", None),
        ("dims must be multiples of 64", _trunk_desc(_lib, dim=100, heads=2)),
        ("dims must be multiples of 64", _trunk_desc(_lib, mlp=1000)),
        ("dims must be multiples of 64", _trunk_desc(_lib, inner=320)),
        ("bad geometry", _trunk_desc(_lib, depth=0)),
        ("bad geometry", _trunk_desc(_lib, max_len=257)),
        ("null pointer in descriptor", _trunk_desc(_lib, master=None)),
        ("null pointer in descriptor", _trunk_desc(_lib, row2seq=None)),
        ("dropout_p must be in [0, 1)", _trunk_desc(_lib, dropout_p=1.0)),
        ("at most 4 sequence groups", _trunk_desc(_lib, n_groups=5)),
        ("bad sequence group", g1),
        ("bad sequence group", g2),
        ("sequence groups must cover n_seq", _trunk_desc(_lib, n_seq=141)),
    ]
    ref = lambda d: None if d is None else C.byref(d)
    queries = (lambda d: h.lafs_trunk_plan(ref(d), 1, C.byref(_lib.TrunkPlanInfo())), lambda d: h.lafs_trunk_row_ranges(ref(d)),
               lambda d: h.lafs_trunk_workspace_bytes(ref(d), 1))
    other = _trunk_desc(_lib, n_tok=0)                      # (a different refusal in front of each query: the text read is its own)
    for why, d in cases:
        for query, code in zip(queries, (-2, -1, -1)):
            assert query(other) == code and "bad geometry" in h.lafs_last_error().decode()
            if "geometry" in why:
                assert query(cases[1][1]) == code
            rc, text = int(query(d)), h.lafs_last_error().decode()
            assert rc == code and why in text, (why, rc, text)
    assert h.lafs_trunk_plan(C.byref(_trunk_desc(_lib)), 1, None) == -2 and "null plan" in h.lafs_last_error().decode()
    assert h.lafs_trunk_workspace_bytes(C.byref(_trunk_desc(_lib)), 1) > 0


def test_trunk_plan_with_options_by_hand_and_its_invariants():
    """The plan under LAFS_OPT_ROW_CHAINS / _SIDE_STREAMS / _MLP_FUSED, written out by hand: one case per rule of csrc/engine.hip's
    plan.  Options need a context, which needs a device: without one all of these cases are passed over and counted -- the rules a
    NULL context reaches are held by the test above."""
    _lib, h = _plan_lib()
    L = _lib
    RC, SS, MF = L.OPT_ROW_CHAINS, L.OPT_SIDE_STREAMS, L.OPT_MLP_FUSED
    FWD, SAVE, BWD, LN2, LN2B, MERGE, NEXT, PRJ, PRJS = (L.MLP_FUSED_FWD, L.MLP_FUSED_FWD_SAVE, L.MLP_FUSED_BWD, L.MLP_FUSED_LN2, L.MLP_FUSED_LN2_BWD,
                                                        L.MLP_FUSED_MERGE_CHAINS, L.MLP_FUSED_NEXT_LN1, L.MLP_FUSED_PROJ_FWD, L.MLP_FUSED_PROJ_FWD_SAVE)
    DEF = L.MLP_FUSED_DEFAULT
    assert DEF == 79 and (FWD, SAVE, BWD, LN2, LN2B, MERGE, NEXT, PRJ, PRJS) == (1, 2, 4, 8, 16, 32, 64, 128, 256)
    two = [(0, 5516, 0, 0, 28, 0), (5516, 4144, 1, 28, 112, 1)]
    four = [(0, 2758, 0, 0, 14, 0), (2758, 2758, 0, 14, 14, 1), (5516, 2072, 1, 28, 56, 2), (7588, 2072, 1, 84, 56, 3)]
    one = [(0, 9660, 0, 0, 140, 0)]
    PG, FK = L.ATTN_PER_GROUP, L.ATTN_PER_GROUP_FORKED
    on, off = (1, 1, 1, 0, 1, 0), (0,) * 6
    # (options, descriptor, save) -> (ranges, attention, merged, flags of every range, (ln1_parts, ln2_parts) per range or None)
    cases = [
        # the row ranges
        ({}, {}, 1, two, PG, 0, on, [(256, 256), (256, 256)]),
        ({RC: 1}, {}, 1, one, FK, 0, on, [(256, 256)]),
        ({RC: 4}, {}, 1, four, PG, 0, on, [(173, 173), (173, 173), (130, 130), (130, 130)]),
        ({SS: 0}, {}, 1, one, PG, 0, on, None),
        ({SS: 0, RC: 4}, {}, 0, one, PG, 0, on, None),
        ({RC: 1}, dict(groups=((28, 197),)), 1, [(0, 5516, 0, 0, 28, 0)], L.ATTN_ONE_LAUNCH, 0, on, None),
        # both sides of the 4096-row threshold, either group
        ({}, dict(groups=((32, 128), (64, 64))), 1, [(0, 4096, 0, 0, 32, 0), (4096, 4096, 1, 32, 64, 1)], PG, 0, on, None),
        ({}, dict(groups=((32, 128), (65, 63))), 1, [(0, 8191, 0, 0, 97, 0)], FK, 0, on, None),
        ({RC: 4}, dict(groups=((35, 117), (64, 64))), 1, [(0, 8191, 0, 0, 99, 0)], FK, 0, on, None),
        # a group of one sequence (at most 256 rows: below the threshold) stays with the other in one range, four chains or not
        ({RC: 4}, dict(groups=((1, 197), (112, 37))), 1, [(0, 4341, 0, 0, 113, 0)], FK, 0, on, None),
        # the fused bits alone ...
        ({MF: 0}, {}, 1, two, PG, 0, off, None),
        ({MF: FWD}, {}, 0, two, PG, 0, (1, 0, 0, 0, 0, 0), None),
        ({MF: FWD}, {}, 1, two, PG, 0, off, None),
        ({MF: SAVE}, {}, 1, two, PG, 0, (1, 0, 0, 0, 0, 0), None),
        ({MF: SAVE}, {}, 0, two, PG, 0, off, None),
        ({MF: BWD}, {}, 1, two, PG, 0, (0, 0, 0, 0, 1, 0), None),
        ({MF: LN2 | LN2B | NEXT | PRJ | PRJS}, {}, 1, two, PG, 0, off, None),                # nothing without the launch they ride on
        ({MF: FWD | SAVE | NEXT}, {}, 1, two, PG, 0, (1, 0, 1, 0, 0, 0), None),
        # ... LayerNorm 2's backward inside: 128-row units, one slot each
        ({MF: DEF | LN2B}, {}, 1, two, PG, 0, (1, 1, 1, 0, 1, 1), [(256, 44), (256, 33)]),
        ({MF: (DEF | LN2B) & ~BWD}, {}, 1, two, PG, 0, (1, 1, 1, 0, 0, 0), [(256, 256), (256, 256)]),
        # ... the merged MLP launch: MERGE_CHAINS switches NEXT_LN1 off, merged or not
        ({MF: DEF | MERGE}, {}, 1, two, PG, 1, (1, 1, 0, 0, 1, 0), None),
        ({MF: DEF | MERGE, RC: 1}, {}, 1, one, FK, 0, (1, 1, 0, 0, 1, 0), None),
        ({MF: BWD | MERGE}, {}, 1, two, PG, 0, (0, 0, 0, 0, 1, 0), None),
        ({MF: DEF | MERGE | PRJ | PRJS}, {}, 1, two, PG, 1, (1, 1, 0, 0, 1, 0), None),
        # ... the projection in front: per pass, only with LayerNorm 2 inside and inner == dim
        ({MF: DEF | PRJ | PRJS}, {}, 0, two, PG, 0, (1, 1, 1, 1, 1, 0), None),
        ({MF: DEF | PRJ | PRJS}, {}, 1, two, PG, 0, (1, 1, 1, 1, 1, 0), None),
        ({MF: DEF | PRJ}, {}, 1, two, PG, 0, on, None),
        ({MF: DEF | PRJS}, {}, 0, two, PG, 0, on, None),
        ({MF: (DEF | PRJ | PRJS) & ~LN2}, {}, 1, two, PG, 0, (1, 0, 1, 0, 1, 0), None),
        ({MF: DEF | PRJ | PRJS}, dict(heads=5), 1, two, PG, 0, on, None),
    ]
    ctxs = _Contexts(h)
    passed_over = 0
    try:
        for i, (opts, dkw, save, ranges, attn, merged, flags, parts) in enumerate(cases):
            ctx = ctxs.get(opts)
            if ctx is None:
                passed_over += 1
                continue
            p = _trunk_plan(_lib, h, _trunk_desc(_lib, ctx=ctx, **dkw), save)
            assert (p.n_ranges, p.attention, p.mlp_merged) == (len(ranges), attn, merged), (i, p.n_ranges, p.attention, p.mlp_merged)
            assert [_rp(p.range[k], *_PLACE) for k in range(p.n_ranges)] == ranges, i
            assert all(_rp(p.range[k], *_FLAGS) == flags for k in range(p.n_ranges)), (i, [_rp(p.range[k], *_FLAGS) for k in range(p.n_ranges)])
            assert parts is None or [_rp(p.range[k], *_PARTS) for k in range(p.n_ranges)] == parts, (i, [_rp(p.range[k], *_PARTS) for k in range(2)])
            assert _rp(p.whole, *_PLACE) == (0, sum(r[1] for r in ranges), 0, 0, sum(r[4] for r in ranges), 0), i
            if merged or p.n_ranges == 1:
                assert _rp(p.whole, *_FLAGS[:4]) == flags[:4], i
        # invariants over the whole grid of options, shapes and passes
        shapes = [{}, dict(dim=128, mlp=512), dict(dropout_p=0.1), dict(heads=5), dict(n_groups=0), dict(groups=((4, 197), (16, 37))),
                  dict(groups=((32, 128), (65, 63))), dict(groups=((28, 197),))]
        n_plans = 0
        for chains in (1, 2, 4):
            for side in (0, 1):
                for mf in (0, FWD, SAVE, BWD, 15, DEF, DEF | LN2B, DEF | MERGE, DEF | PRJ | PRJS, 511, 511 & ~MERGE, 511 & ~LN2, 511 & ~BWD):
                    ctx = ctxs.get({RC: chains, SS: side, MF: mf})
                    if ctx is None:
                        continue
                    for dkw in shapes:
                        for save in (0, 1):
                            d = _trunk_desc(_lib, ctx=ctx, **dkw)
                            p = _trunk_plan(_lib, h, d, save)
                            n_plans += 1
                            rs = [p.range[k] for k in range(p.n_ranges)]
                            assert 1 <= p.n_ranges <= (chains if side else 1)
                            assert rs[0].row0 == 0 and rs[-1].row0 + rs[-1].rows == d.n_tok == p.whole.rows           # the ranges tile [0, n_tok) ...
                            assert all(a.row0 + a.rows == b.row0 and a.seq0 + a.n_seq == b.seq0 for a, b in zip(rs, rs[1:]))
                            assert rs[0].seq0 == 0 and rs[-1].seq0 + rs[-1].n_seq == d.n_seq
                            if p.n_ranges > 1:                                                                      # ... from sequence boundaries
                                assert all(r.rows == r.n_seq * d.group_max_len[r.group] and r.stream == k for k, r in enumerate(rs))
                            assert (p.attention == L.ATTN_ONE_LAUNCH) == (d.n_groups <= 1)
                            assert (p.attention == FK) == (d.n_groups > 1 and p.n_ranges == 1 and side == 1)
                            assert not p.mlp_merged or (p.n_ranges > 1 and mf & MERGE and p.whole.fwd_fused)
                            for r in rs + [p.whole]:
                                assert not r.fwd_next_ln1 or (r.fwd_fused and not p.mlp_merged and mf & NEXT and not mf & MERGE)
                                assert not r.fwd_proj_inside or (r.fwd_ln2_inside and d.inner == d.dim and not p.mlp_merged)
                                assert not r.fwd_ln2_inside or r.fwd_fused
                                assert not r.bwd_ln2_inside or (r.bwd_fused and mf & LN2B)
                                assert not (r.fwd_fused or r.bwd_fused) or (d.dim == 384 and d.dropout_p == 0)
                                assert r.ln1_parts == h.lafs_layernorm_bwd_parts(r.rows, d.dim)
                                assert r.ln2_parts == (h.lafs_mlp_fused_ln_parts(r.rows) if r.bwd_ln2_inside else r.ln1_parts)
        assert n_plans == (3 * 2 * 13 * len(shapes) * 2 if torch.cuda.is_available() else 0)
    finally:
        ctxs.close()
    assert len(cases) == 30 and passed_over == (0 if torch.cuda.is_available() else len(cases))
