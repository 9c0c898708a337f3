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
