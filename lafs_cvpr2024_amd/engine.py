"""Fused LAFS pre-training step (reference lafs_train.py:513-613) for one MI355X rank.

    teacher fwd (global crops) -> student fwd (all crops, one packed pass) -> fused DINO loss fwd+bwd ->
    head bwd -> [RCCL all-reduce of head grads + center sum, overlapped with] trunk bwd -> [all-reduce trunk grads] ->
    per-tensor clip + AdamW + teacher EMA + bf16 shadow refresh (one launch) -> center EMA

Everything between the brackets is captured once into hipGraphs (static buffers, hyper-parameters in a device
buffer that is refreshed by one async H2D copy per step), so a step costs one graph launch on a single rank, and one per
stretch between two collectives on several, instead of ~1500 kernel launches from Python.  The step is written once, as a
generator that yields where a collective sits (_step); collectives stay outside the graphs and run through torch.distributed
("nccl" = RCCL).
"""
import math
from functools import partial

import numpy as np
import os

import torch
import torch.distributed as dist

from . import _lib, functional as Fn, ops
from .arena import ParamArena
from .distributed import BnStatExchange, FlatReducer
from .ops import _p, call
from .utils import PinnedRing, capture_stretches
from .vision_transformer import VisionTransformer, attach_arena, _is_matrix_for_dgrad


def _is_partfvit(m):
    from .face_pre_pro.ViT_face import ViT_face_landmark_patch8
    return isinstance(m, ViT_face_landmark_patch8)


def _is_fvit(m):
    from .face_pre_pro.ViT_face import ViTs_face_overlap
    return isinstance(m, ViTs_face_overlap)


# The reference converts both networks to SyncBatchNorm before it wraps them (lafs_train.py:362-364): fViT's BatchNorm1d head then
# normalises with the statistics of the cls rows of ALL ranks.  lafs_bn1d_groups_fwd sees one rank's rows; the cross-rank form
# (lafs_bn1d_groups_stats / _sync_fwd / _bwd_sums / _sync_bwd with two small collectives between them) is behind `sync_bn`.
FVIT_MULTI_RANK = ("fViT pre-training on more than one rank needs SyncBatchNorm statistics across the ranks (reference "
                   "lafs_train.py:362-364): pass sync_bn=True (lafs_train.py --sync_bn true), or run --arch fvit on a single rank")

# The same conversion reaches the two BatchNorm1d of a DINOHead(use_bn=True): on several ranks the reference's head normalises its
# hidden activations with the statistics of all ranks.  The fused head kernels (lafs_bn1d_gelu_fwd / _bwd) see one rank's rows and
# have no cross-rank form yet; `sync_bn` covers fViT's own head only and does not lift this.
HEAD_BN_MULTI_RANK = ("a DINO head with BatchNorm (use_bn_in_head) on more than one rank needs SyncBatchNorm statistics across the ranks "
                      "(the reference converts both networks, lafs_train.py:362-364), which the head kernels do not exchange yet "
                      "(--sync_bn covers fViT's own head only): run --use_bn_in_head true on a single rank")

f32, bf16 = torch.float32, torch.bfloat16

# --optimizer (reference lafs_train.py:92-93, 399-404).  momentum and eta are constants of the reference, not flags:
# torch.optim.SGD(params_groups, lr=0, momentum=0.9) and the defaults of utils.LARS (utils.py:557)
OPTIMIZERS = ('adamw', 'sgd', 'lars')
SGD_MOMENTUM, LARS_ETA = 0.9, 0.001
# the per-tensor state key each optimizer's state_dict holds, by which a state_dict's kind is told
_STATE_KEY = {'adamw': 'exp_avg', 'sgd': 'momentum_buffer', 'lars': 'mu'}


def _interp_matrix(grid_src, grid_dst, device):
    """Dense matrix of torch's bicubic F.interpolate from a g x g grid to an r x r grid with the reference's
    scale_factor = (r + 0.1) / g (vision_transformer.py:184-191): a fixed linear map, built once by pushing the
    identity through the same torch op, so pos tokens (and their gradient) become one small matmul."""
    n = grid_src * grid_src
    eye = torch.eye(n, device=device).view(1, n, grid_src, grid_src)
    sf = (grid_dst + 0.1) / grid_src
    out = torch.nn.functional.interpolate(eye, scale_factor=(sf, sf), mode="bicubic")
    assert out.shape[-1] == grid_dst and out.shape[-2] == grid_dst
    return out.view(n, grid_dst * grid_dst).t().contiguous()            # [r*r, g*g]


class LafsPretrainEngine:
    def __init__(self, student, teacher, dino_loss, batch_size, n_local=8, global_size=112, local_size=48,
                 clip_grad=3.0, freeze_last_layer=1, use_graph=True, device=None, grad_slices=4, sync_bn=False,
                 optimizer='adamw', koleo_weight=0.0):
        self.device = torch.device(device if device is not None else ("cuda", torch.cuda.current_device()))
        self.student, self.teacher, self.dino_loss = student, teacher, dino_loss
        self.B, self.n_local, self.ncrops = batch_size, n_local, 2 + n_local
        self.clip_grad, self.freeze_last_layer = float(clip_grad or 0.0), freeze_last_layer
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        vit_s, vit_t = student.backbone, teacher.backbone
        # Two backbones: the DINO VisionTransformer (NCHW crops, bicubic-resampled position table) and Part-fViT,
        # ViT_face_landmark_patch8 -- the pair the reference actually pre-trains (lafs_train.py:300-335, arch 'mynet'): landmark
        # mosaics as [B, n, 192] patch tokens, position table sliced to n+1 rows, DropPath 0.1 + dropout 0.1 live in the student
        # AND the teacher (the reference never calls teacher.eval()).
        # fViT (ViTs_face_overlap) is the Part-fViT transformer behind an overlapping window embedding and with a BatchNorm1d head on
        # the cls rows: it shares every `facevit` choice below (sliced position table, constant DropPath, live dropout in both
        # networks); its own are the window geometry and the head, whose batch statistics and running-statistic updates are per crop
        # group (lafs_bn1d_groups_fwd) in BOTH networks -- the reference never calls teacher.eval() (lafs_train.py: no .eval() but :269),
        # so the teacher normalises its 2B global rows with batch statistics and updates its own running buffers.
        self.partfvit = _is_partfvit(vit_s)
        self.fvit = _is_fvit(vit_s)
        self.facevit = self.partfvit or self.fvit
        if not (isinstance(vit_s, VisionTransformer) or self.facevit) or type(vit_s) is not type(vit_t):
            raise _lib.LafsHipError("LafsPretrainEngine drives a VisionTransformer, a ViT_face_landmark_patch8 or a ViTs_face_overlap pair")
        if self.fvit and self.world > 1 and not sync_bn:
            raise _lib.LafsHipError(FVIT_MULTI_RANK)
        # DINOHead(use_bn=True): both heads run their BatchNorm1d pair in whatever mode the head module is in -- the reference never
        # calls teacher.eval(), so by default the teacher too normalises its 2B rows with batch statistics and steps its own buffers
        self.head_bn = bool(getattr(student.head, "use_bn", False))
        if self.head_bn != bool(getattr(teacher.head, "use_bn", False)):
            raise _lib.LafsHipError("student and teacher heads must both be built with, or both without, use_bn")
        if self.head_bn and self.world > 1:
            raise _lib.LafsHipError(HEAD_BN_MULTI_RANK)
        # The step (_step) is written once and yields wherever a collective has to sit between its kernels: captured, every stretch
        # between two yields is one hipGraph.  A single rank has no collective to place: it never yields, and the whole step is ONE
        # graph (five replay boundaries less); LAFS_ONE_GRAPH=0 gives it the multi-rank launch structure.
        self._one_graph = self.world == 1 and os.environ.get("LAFS_ONE_GRAPH", "1") != "0"
        # sync_bn (fViT pairs only): the head normalises every crop group with the statistics of the cls rows of ALL ranks.  The forward
        # is cut once more, around the exchange of the partial statistics (_forward), the head backward around the all-reduce of its two
        # sums (_seg_trunk_backward).  One rank has nobody to exchange with: it takes this form only where it runs the multi-rank
        # launch structure anyway, else the plain kernels -- the same bits.
        self.sync_bn = bool(sync_bn) and self.fvit and not self._one_graph
        self.n_fwd = 2 if self.sync_bn else 1                # graph segments of the forward
        self._bn_sums_live = False
        self._drop_fixed = {}
        if self.fvit and (vit_s.ac_patch_size, vit_s.patch_size, vit_s.pad) != (vit_t.ac_patch_size, vit_t.patch_size, vit_t.pad):
            raise _lib.LafsHipError("student and teacher fViT must embed with the same window")
        if self.partfvit and (vit_s.with_land or vit_t.with_land):
            raise _lib.LafsHipError("LAFS pre-training uses with_land=False backbones (the landmark CNN is the frozen front-end)")
        # --optimizer of the reference (lafs_train.py:399-404).  The choice is fixed here: it picks the kernel pair of _update_piece once
        # and which state buffers exist (sgd / lars keep exp_avg alone, as their momentum); nothing reads it during a step.
        if optimizer not in OPTIMIZERS:
            raise _lib.LafsHipError(f"optimizer {optimizer!r}: one of {', '.join(OPTIMIZERS)}")
        self.optimizer = optimizer
        self.sa = attach_arena(student, self.device, second_moment=optimizer == 'adamw')
        if optimizer == 'adamw' and self.sa.exp_avg_sq is None:
            raise _lib.LafsHipError("the student's arena was built without a second-moment buffer: it cannot run AdamW")
        if optimizer == 'lars':
            # utils.LARS decays and adapts the tensors with ndim != 1 (utils.py:573-576); the kernels key both on LAFS_SEG_DECAY,
            # which utils.get_params_groups' rule sets for exactly those tensors
            flags = self.sa.seg_flags.cpu().tolist()
            for name, p, f in zip(self.sa.names, self.sa.params, flags):
                if p.requires_grad and bool(f & _lib.SEG_DECAY) != (p.dim() != 1):
                    raise _lib.LafsHipError(f"optimizer 'lars': {name} has {p.dim()} dimensions but its weight-decay flag is "
                                            f"{'set' if f & _lib.SEG_DECAY else 'clear'}; LARS decays and adapts exactly the tensors with ndim != 1")
            self.seg_trust = torch.ones(self.sa.n_seg, device=self.device, dtype=f32)
            self.chunk_part = self.sa.scratch("lars_chunk_part", 3 * self.sa.n_chunks)
        # the library's side streams / events / kernel options of THIS engine (created now: nothing is created inside a capture;
        # two engines share no stream or event).  The environment's A/B switches are read by _lib.Ctx, not by the library.
        self.ctx = _lib.Ctx(self.device)
        # Both trunks are read through their cls rows alone (head on x[:, 0]): the last block runs on those rows behind its qkv GEMM
        # (lafs_trunk_desc::cls_only_last; the plan keeps trunks with element dropout dense).  LAFS_CLS_ONLY_LAST=0: dense, for A/B.
        self.cls_only_last = _lib.Ctx.env_cls_only_last()
        # The row chains (long / short sequences on two streams) pay on the ViT-S trunk, whose K = 384 kernels leave CUs idle; the
        # Part-fViT trunk's wide GEMMs run on one-workgroup-per-CU persistent tiles (gemm_big.hip) that want the whole chip and the
        # merged 44 160 rows (753 tiles of 176x256 = 2.94 rounds): `mynet` pair 36.1 ms with two chains, 35.4-35.5 with one.
        # fViT runs the same wide trunk and follows that default; the choice has not been measured for fViT.
        if self.facevit and "LAFS_ROW_CHAINS" not in os.environ:
            self.ctx.set(_lib.OPT_ROW_CHAINS, 1)
        self.ta = getattr(teacher, "_lafs_arena", None)
        if self.ta is None:
            for p in teacher.parameters():
                p.requires_grad = False
            self.ta = ParamArena(teacher, self.device, with_grad=False, transposed=None)
            object.__setattr__(teacher, "_lafs_arena", self.ta)
            for name, m in teacher.named_modules():
                if hasattr(m, "_bind_arena"):
                    m._bind_arena(self.ta, name + "." if name else "")
        for b in teacher.buffers():                  # (fViT's running statistics: the kernels update them in place)
            b.data = b.data.to(self.device)
        if self.sa.names != self.ta.names or self.sa.size != self.ta.size:
            raise _lib.LafsHipError("student and teacher must have identical parameter layouts")
        self.sa.ctx = self.ta.ctx = self.ctx
        dino_loss.to(self.device)
        if self.world > 1:                       # DDP's initial parameter broadcast (reference lafs_train.py:375)
            bn = [b for m in (vit_s.mlp_head[0], vit_t.mlp_head[0]) for b in m.buffers()] if self.fvit else []      # (DDP: buffers too)
            for t in [self.sa.master, self.ta.master, dino_loss.center] + bn:
                dist.broadcast(t, 0)
            self.sa.refresh_shadows(); self.ta.refresh_shadows()
        self.K = student.head.out_dim
        self.Kpad = (self.K + 127) // 128 * 128
        B, D = batch_size, (vit_s.dim if self.facevit else vit_s.embed_dim)
        window = (vit_s.ac_patch_size, vit_s.patch_size, vit_s.pad) if self.fvit else None      # nn.Unfold(k, stride, padding)
        self.geom_s = Fn.geometry([(2 * B, global_size), (n_local * B, local_size)] if n_local else [(2 * B, global_size)], self.device,
                                  window=window)
        self.geom_t = Fn.geometry([(2 * B, global_size)], self.device, window=window)
        self.spec_s, self.spec_t = vit_s._spec, vit_t._spec
        self.head_prefix_s, self.head_prefix_t = student.head._prefix, teacher.head._prefix
        # bicubic resampling matrices for the stored position table (Part-fViT: plain slices, no resampling)
        self.grids = [global_size // 8] + ([local_size // 8] if n_local else [])
        if self.fvit:                                # windows per side: 14 and 6 for 112 / 48 px at 12 / 8 / 4
            self.grids = [ops.unfold_windows(s, *window) for s in [global_size] + ([local_size] if n_local else [])]
            if self.B * (self.world if self.sync_bn else 1) < 2:
                raise _lib.LafsHipError("fViT's BatchNorm1d head needs more than one row per crop group: batch_size >= 2 "
                                        "(with sync_bn: batch_size x ranks >= 2)")
            self.bn_s, self.bn_t = vit_s.mlp_head[0], vit_t.mlp_head[0]
        if self.facevit:
            if vit_s.num_patches < self.grids[0] ** 2:
                raise _lib.LafsHipError("pos_embedding is shorter than the global crops' token count")
            self.interp = [None for _ in self.grids]
        else:
            g = int(math.isqrt(vit_s.pos_embed.shape[1] - 1))
            self.interp = [None if r == g else _interp_matrix(g, r, self.device) for r in self.grids]
        # element dropout (Part-fViT: 0.1 live in student AND teacher, the reference never calls teacher.eval()): counter-based masks
        # whose seed is (network seed + 7919 * hyper[HP_STEP]), the step read on the DEVICE inside the kernels exactly as the
        # DropPath draw reads it -- a captured graph draws new masks on every replay, and the masks are indexed by absolute token
        # rows, so the row chains stay legal
        self.has_dropout = self.facevit and (vit_s.dropout_rate > 0 or vit_s.emb_dropout_rate > 0 or
                                              vit_t.dropout_rate > 0 or vit_t.emb_dropout_rate > 0)
        self.dropout_seed_s, self.dropout_seed_t = 0x5EED, 0x7EAC4E5       # independent masks in the two networks
        # static buffers
        dev = self.device
        self.hyper = torch.zeros(_lib.HP_COUNT, device=dev, dtype=f32)
        self.hyper_ring = PinnedRing((_lib.HP_COUNT,), f32)   # the host runs steps ahead of the GPU: never reuse a pinned
        self.temps = torch.zeros(2, device=dev, dtype=f32)    # staging buffer whose copy may still be pending
        self.temps_ring = PinnedRing((2,), f32)
        # The last layer of both heads + the DINO loss + the centre sums as ONE fused group of launches (csrc/dino_head_loss.hip): the
        # logits are formed twice on the MFMA instead of written once and read twice (0.9 GB and ~0.2 ms per step at C2).  Needs the
        # DINOHead's default bottleneck (256) and at most 64 images per rank; LAFS_FUSED_HEAD=0 keeps the unfused kernels (A/B runs,
        # and what the tests that look at the logits themselves use: `logits_s` / `logits_t` only exist there).
        bott = student.head.last_layer.weight_v.shape[1]
        self.fused_head = (bott == 256 and 2 * B <= 128 and os.environ.get("LAFS_FUSED_HEAD", "1") != "0")
        self._logits_s = None if self.fused_head else torch.zeros(self.ncrops * B, self.Kpad, device=dev, dtype=f32)
        self._logits_t = None if self.fused_head else torch.zeros(2 * B, self.Kpad, device=dev, dtype=f32)
        self._head_states = None
        self.head_ws = (torch.empty(_lib.lib().lafs_dino_head_loss_workspace(self.ncrops, B, self.K), device=dev, dtype=f32)
                        if self.fused_head else None)
        self.dlogits = torch.zeros(self.ncrops * B, self.Kpad, device=dev, dtype=bf16)
        self.loss = torch.zeros(1, device=dev, dtype=f32)
        # KoLeo regulariser of DINOv2 (csrc/koleo.hip; nothing of it in the reference, PARITY UNPINNED) on the backbone's cls features of
        # the student's two global crops, one group of B rows per crop: loss = dino_loss + koleo_weight (L_0 + L_1).  Its gradient is
        # added to dfeat between the head backward and the trunk backward (_forward).  The neighbours are searched inside this rank's
        # batch, as DINOv2 searches them, so no collective is added.  Weight 0: no buffer, no launch -- the step of an engine without it.
        self.koleo_weight = float(koleo_weight)
        if not self.koleo_weight >= 0.0:
            raise _lib.LafsHipError(f"koleo_weight {koleo_weight!r}: a weight >= 0 (0 = off; DINOv2 uses 0.1)")
        self.koleo = None
        if self.koleo_weight > 0:
            if B < 2:
                raise _lib.LafsHipError("koleo_weight > 0 needs batch_size >= 2: every row's nearest neighbour is another row of its crop")
            self.koleo = torch.zeros(2, device=dev, dtype=f32)
            self.koleo_nn = torch.zeros(2 * B, device=dev, dtype=torch.int32)
            self.koleo_ws = ops.koleo_workspace(2, B, D, dev)
        self._feat_s = None
        self.loss_ws = torch.empty(_lib.lib().lafs_dino_loss_workspace(self.ncrops, B, self.K), device=dev, dtype=f32)
        self.colsum = torch.zeros(self.K, device=dev, dtype=f32)
        self.in_global_all = torch.zeros(2 * B, 3, global_size, global_size, device=dev)
        self.in_local_all = torch.zeros(max(n_local, 1) * B, 3, local_size, local_size, device=dev)
        self.in_global = list(self.in_global_all.split(B))
        self.in_local = list(self.in_local_all.split(B))[:n_local]
        # DropPath scales are drawn by lafs_droppath_scales from (seed, hyper[HP_STEP]): new masks on every graph replay without
        # an ATen RNG kernel; keep probabilities per block on the device, None when every rate is 0
        def keep_probs(v):
            rates = [v.drop_path_rate] * v.depth if self.facevit else list(v.drop_path_rates)
            return torch.tensor([1.0 - r for r in rates], device=dev, dtype=f32) if any(rates) else None
        self.keep_s, self.keep_t = keep_probs(vit_s), keep_probs(vit_t)
        self.drop_s = torch.empty(vit_s.depth, 2, self.geom_s.n_seq, device=dev, dtype=f32)
        self.drop_t = torch.empty(vit_t.depth, 2, self.geom_t.n_seq, device=dev, dtype=f32)
        self.drop_seed = 0x0D20FA7
        # resampled position tables (static: [1 + r*r, D] per crop size and network)
        self.pos_s = [torch.empty(r * r + 1, D, device=dev, dtype=f32) for r in self.grids]
        self.pos_t = [torch.empty(self.grids[0] ** 2 + 1, D, device=dev, dtype=f32)]
        # tensors whose gradient is WRITTEN by its first producer (block weights: wgrad fold with accumulate = 0; last layer:
        # weight-norm backward): the per-step zeroing skips them (lafs_zero_chunks)
        flags = self.sa.seg_flags.cpu().tolist()
        over = {nm[k] for nm in self.spec_s.trunk.block_names for k in ("w_qkv", "w_proj", "w_fc1", "w_fc2")}
        over.add(self.head_prefix_s + "last_layer.weight_v")
        for i, name in enumerate(self.sa.names):
            # (a frozen tensor's gradient is never written nor read: nothing to zero either)
            if name in over or not self.sa.params[i].requires_grad:
                flags[i] |= _lib.SEG_OVERWRITTEN
        self.sa.seg_flags.copy_(torch.tensor(flags, dtype=torch.int32))
        # gradient ranges for the two all-reduces: [trunk | head]
        self.head_start = min(o for n, o in self.sa.offsets.items() if n.startswith(self.head_prefix_s))
        self.depth = vit_s.depth
        self.pos_name = self.spec_s.pos
        # the trunk backward is cut into `grad_slices` graph segments (blocks depth-1 .. 0 in equal runs) so that each run's
        # gradients are already on the wire (RCCL) while the next run is computed; only the last run's all-reduce is exposed
        ns = max(1, min(int(grad_slices), self.depth))
        self.cuts = [self.depth - (self.depth * k) // ns for k in range(ns + 1)]            # e.g. depth 12, 4 slices: 12 9 6 3 0
        off = lambda blk: self.sa.offsets[self.spec_s.trunk.block_names[blk]["ln1_g"]] if blk > 0 else 0
        self.cut_offsets = [off(c) for c in self.cuts[1:]]                                   # arena offset where each run starts
        self.reducer = FlatReducer()
        if self.sync_bn:
            # student and teacher partials in one buffer (one collective); the groups' row counts over all ranks
            self.bn_x = BnStatExchange([len(self.geom_s.groups), len(self.geom_t.groups)], D, dev, self.reducer)
            self.bn_total_s = [n * self.world for n, _ in self.geom_s.groups]
            self.bn_total_t = [n * self.world for n, _ in self.geom_t.groups]
        if self.world > 1:
            # LAFS_COMM_CUS=n (opt-in, default 0) shrinks the K-resident GEMM's grid by 2 n workgroups while gradients are on the
            # wire.  It does not reserve CUs (the dispatcher still spreads the remaining workgroups over the chip) and has never been
            # A/B-measured beside RCCL kernels, so it stays off until a multi-GPU box shows a gain.
            self.ctx.set(_lib.OPT_COMM_CUS, int(os.environ.get("LAFS_COMM_CUS", "0")))
        # Update pieces: ranges of the arena in the order their gradients become final -- the DINO head (31 of 53 M parameters at C2)
        # after the head backward, then each run of blocks after its segment of the trunk backward.  A piece's per-tensor norms,
        # clip + AdamW + teacher EMA + shadow refresh run on a stream of their own at the START of a later segment, beside that
        # segment's GEMM-heavy work, instead of as a serial HBM-bound tail of the step (the reference's optimizer.step() /
        # EMA loop, lafs_train.py:606-613, touches nothing the backward still reads: a block's weights are dead once its
        # gradients exist).  Data-parallel runs give every piece one segment of slack for its all-reduce.
        bounds = [self.sa.size, self.head_start] + list(self.cut_offsets)
        self.pieces = [(bounds[i + 1], bounds[i]) for i in range(len(bounds) - 1) if bounds[i] > bounds[i + 1]]
        seg_at = {self.sa.offsets[n]: i for i, n in enumerate(self.sa.names)}
        seg_at[self.sa.size] = self.sa.n_seg
        self.piece_segs = [(seg_at[lo], seg_at[hi]) for lo, hi in self.pieces]
        chunk_seg = self.sa.chunk_seg.cpu()
        for (lo, hi), (s_lo, s_hi) in zip(self.pieces, self.piece_segs):        # a piece is whole tensors: its first / last chunk carry its first / last segment
            assert lo % _lib.CHUNK == 0 and hi % _lib.CHUNK == 0 and 0 <= s_lo < s_hi <= self.sa.n_seg
            assert int(chunk_seg[lo // _lib.CHUNK]) == s_lo and int(chunk_seg[hi // _lib.CHUNK - 1]) == s_hi - 1, (lo, hi, s_lo, s_hi)
        n_segments = self.n_fwd + len(self.cuts)            # forward (two with sync_bn), the runs of the trunk backward, the final update
        self.n_segments = n_segments
        slack = 1 if self.world > 1 else 0
        serial = os.environ.get("LAFS_OPT_OVERLAP", "1") == "0"          # A/B knob: every piece in the final segment
        self.piece_runs_at = [n_segments - 1 if serial else min(p + self.n_fwd + slack, n_segments - 1) for p in range(len(self.pieces))]
        self._piece_tokens = [[] for _ in self.pieces]       # the reducer's tokens of the step in flight
        self._center_tok = None
        self.opt_stream = None if os.environ.get("LAFS_SINGLE_STREAM") == "1" else torch.cuda.Stream(device=self.device)
        # large frozen tensors (Part-fViT's 30000 x 768 CosFace table: 92 MB of zeros per step on the wire otherwise) are cut out
        # of the all-reduced ranges; small frozen ones (weight_g) ride along rather than splitting a collective
        self._frozen_runs = [(self.sa.offsets[n], self.sa.offsets[n] + (p.numel() + _lib.CHUNK - 1) // _lib.CHUNK * _lib.CHUNK)
                             for n, p in zip(self.sa.names, self.sa.params) if not p.requires_grad and p.numel() >= (1 << 20)]
        # teacher forward / weight-gradient GEMMs run on a second stream; LAFS_SINGLE_STREAM=1 serialises everything (profiling)
        self.side_stream = None if os.environ.get("LAFS_SINGLE_STREAM") == "1" else torch.cuda.Stream(device=self.device)
        self._update_range = {'adamw': self._update_adamw, 'sgd': self._update_sgd, 'lars': self._update_lars}[optimizer]
        self.use_graph = use_graph
        self._graphs = None
        self._st = {}
        self.step_count = 0

    def _logits(self, which):
        """The last step's logits [rows, Kpad] (f32).  With the fused head they are never stored: formed here on demand from the
        last layer's saved operands (tests / diagnostics only)."""
        if not self.fused_head:
            return self._logits_s if which == 0 else self._logits_t
        if self._head_states is None:
            raise _lib.LafsHipError("no step has run yet")
        st = self._head_states[which]
        return ops.gemm_nt(st.zn, st.wn, _lib.EPI_F32, n_cols=st.Kpad)

    @property
    def koleo_value(self):
        """koleo_weight (L_0 + L_1) of the last step as a device scalar: what the step added to the DINO loss in self.loss."""
        if self.koleo is None:
            raise _lib.LafsHipError("koleo_value: the engine was built with koleo_weight 0")
        return self.koleo_weight * self.koleo.sum()

    logits_s = property(lambda self: self._logits(0))
    logits_t = property(lambda self: self._logits(1))

    # ------------------------------------------------------------------ pieces (all capturable)
    def _pos_tokens(self, arena, spec, bufs):
        pe = arena.view(arena.master, spec.prefix + spec.pos).view(-1, spec.trunk.dim)
        out = []
        for M, r, buf in zip(self.interp, self.grids, bufs):
            if self.facevit:
                out.append(pe[:r * r + 1])                 # pos_embedding[:, :n+1] (reference ViT_face.py:766, fViT :1590)
            elif M is None:
                out.append(pe)
            else:                                          # bicubic resampling as its fixed linear map, one small launch
                call("lafs_pos_interp_fwd", _p(pe), _p(M), _p(buf), M.shape[0], M.shape[1], spec.trunk.dim)
                out.append(buf)
        return out

    def set_droppath_scales(self, student=None, teacher=None):
        """Parity hook: use the given stochastic-depth scales ([depth, 2, n_seq] of 0 or 1/keep, sequences in packed order: global
        crops first) instead of drawing them on the device -- the tests hand the engine the masks the reference drew (F17).  None
        restores the device draw.  Must be set before the step is captured."""
        if self._graphs is not None:
            raise _lib.LafsHipError("set_droppath_scales after the step has been captured")
        dev = lambda t, like: None if t is None else t.to(self.device, f32).reshape(like.shape).contiguous()
        self._drop_fixed = {0: dev(student, self.drop_s), 1: dev(teacher, self.drop_t)}

    def _drop_scales(self, keep, out, salt):
        fixed = self._drop_fixed.get(salt)
        if fixed is not None:
            out.copy_(fixed)
            return out
        if keep is None:
            return None
        call("lafs_droppath_scales", _p(keep), out.shape[0], out.shape[2], (self.drop_seed + salt) & 0xFFFFFFFF,
             _p(self.hyper[_lib.HP_STEP:]), _p(out))
        return out

    def _dropout_cfg(self, vit, seed):
        """(p_trunk, p_embedding, seed, device step counter) of a Part-fViT network in training mode, else None."""
        if not self.facevit or not vit.training or (vit.dropout_rate == 0.0 and vit.emb_dropout_rate == 0.0):
            return None
        return (vit.dropout_rate, vit.emb_dropout_rate, seed, self.hyper[_lib.HP_STEP:])

    def _fork_side(self):
        """(main stream, side stream), the side stream waiting for the main one: the teacher runs there beside the student."""
        cur = torch.cuda.current_stream()
        # LAFS_TEACHER_SERIAL=1: lab knob, the teacher in front of the student on the main stream
        serial = self.side_stream is None or os.environ.get("LAFS_TEACHER_SERIAL") == "1"
        side = cur if serial else self.side_stream
        side.wait_stream(cur)
        return cur, side

    def _teacher_head(self, feat_t, st_t):
        if feat_t is None:                             # BatchNorm with the statistics of all ranks: the exchange buffer holds them now
            feat_t = Fn.vit_forward_sync_bn(self.ta, self.spec_t, st_t, self.bn_x.all(1), self.bn_total_t)
        if self.fvit and self.teacher.backbone.training:   # one forward of one group (device add: no host sync, capturable)
            self.bn_t.num_batches_tracked.add_(1)
        return Fn.head_forward(self.ta, self.head_prefix_t, feat_t, self.K, save=False, logits=self._logits_t, skip_logits=self.fused_head)[1]

    def _student_head(self, feat_s, st_v):
        self._bn_sums_live = feat_s is None            # (then the head backward too goes through sums of all ranks)
        if feat_s is None:
            feat_s = Fn.vit_forward_sync_bn(self.sa, self.spec_s, st_v, self.bn_x.all(0), self.bn_total_s)
        if self.fvit and self.student.backbone.training:   # the reference's forward runs the head once per crop group (:1556-1569)
            self.bn_s.num_batches_tracked.add_(len(self.geom_s.groups))
        self._feat_s = feat_s                          # what the head receives: the KoLeo term reads its first 2B rows
        return Fn.head_forward(self.sa, self.head_prefix_s, feat_s, self.K, save=True, logits=self._logits_s, skip_logits=self.fused_head)[1]

    def _forward(self):
        """The forward, up to the student's head backward (a generator, see _step): both trunks, both heads, loss.  With sync_bn it
        yields once, between the trunks and the BatchNorm of their cls rows, where the partial statistics of the ranks have to meet."""
        sa, ta, vit, vit_t = self.sa, self.ta, self.student.backbone, self.teacher.backbone
        call("lafs_zero_chunks", _p(sa.grad), _p(sa.chunk_seg), _p(sa.seg_flags), sa.n_chunks, _lib.SEG_OVERWRITTEN)
        if self.sync_bn:
            self.bn_x.clear()
        # with sync_bn a network in training mode stops at the partial statistics of its cls rows (feat None), written into this rank's
        # slot of the zeroed exchange buffer; one in eval mode needs no exchange and runs through
        slot = lambda i, v: self.bn_x.slot(i) if self.sync_bn and v.training else None
        cur, side = self._fork_side()
        with torch.cuda.stream(side):                  # teacher: two global views, no activations kept
            pos_t = self._pos_tokens(ta, self.spec_t, self.pos_t)[:1]
            drop_t = self._drop_scales(self.keep_t, self.drop_t, 1) if vit_t.training else None   # rate 0 for the DINO ViT teacher
            feat_t, st_t = Fn.vit_forward(ta, self.spec_t, self.geom_t, [self.in_global_all], pos_t, drop_t, save=False,
                                          dropout=self._dropout_cfg(vit_t, self.dropout_seed_t), bn_training=vit_t.training,
                                          bn_partial=slot(1, vit_t), cls_only_last=self.cls_only_last)[:2]
            if not self.sync_bn:                       # uncut: trunk -> head on the side stream, which never waits for the student
                st_ht = self._teacher_head(feat_t, st_t)
        drop = self._drop_scales(self.keep_s, self.drop_s, 0) if vit.training else None
        imgs = [self.in_global_all] + ([self.in_local_all] if self.n_local else [])      # student: all views in one packed pass
        feat_s, st_v = Fn.vit_forward(sa, self.spec_s, self.geom_s, imgs, self._pos_tokens(sa, self.spec_s, self.pos_s), drop, save=True,
                                      dropout=self._dropout_cfg(vit, self.dropout_seed_s), wgrad_overwrite=True,
                                      wgrad_workgroups=int(os.environ.get("LAFS_WGRAD_WG", 200)) if self.side_stream is not None else 0,
                                      bn_training=vit.training, bn_partial=slot(0, vit), cls_only_last=self.cls_only_last)[:2]
        if self.sync_bn:
            cur.wait_stream(side)
            yield lambda: self.reducer.wait([self.bn_x.gather()])      # one collective on the step's critical path
            cur, side = self._fork_side()
            with torch.cuda.stream(side):
                st_ht = self._teacher_head(feat_t, st_t)
        st_h = self._student_head(feat_s, st_v)
        cur.wait_stream(side)
        dfeat = self._head_loss_backward(st_h, st_ht)
        if self.koleo is not None:                     # + koleo_weight d(L_0 + L_1)/dfeat on the global crops' rows (packed first)
            B = self.B
            ops.koleo(self._feat_s[:2 * B], 2, B, grad_scale=self.koleo_weight, dx=dfeat[:2 * B], accumulate=True, loss=self.koleo,
                      nn=self.koleo_nn, ws=self.koleo_ws)
        if self._bn_sums_live:                         # this rank's two sums of the BatchNorm backward
            Fn.vit_backward_bn_sums(sa, self.spec_s, st_v, dfeat, self.bn_x.sums)
        self._st = dict(vit=st_v, dfeat=dfeat)

    def _seg_forward(self):
        """The forward run eagerly (tests)."""
        for act in self._forward():
            act()

    def _head_loss_backward(self, st_h, st_ht):
        """Last layer of both heads, DINO loss forward + backward, center column sums, student head backward.  Returns dfeat."""
        sa, B = self.sa, self.B
        if self.fused_head:
            # last layer of both heads + loss forward + dL/dlogits + center column sums, the logits never stored
            ops.dino_head_loss(st_h.zn, st_ht.zn, st_h.wn, st_ht.wn, self.dino_loss.center.view(-1), self.ncrops, self.K,
                               float(self.dino_loss.student_temp), 0.04, grad=self.dlogits, loss=self.loss, colsum=self.colsum,
                               ws=self.head_ws, dev_temps=self.temps)
        else:
            # loss forward + dL/dlogits in the same two passes; center column sums of the raw teacher logits
            ops.dino_loss_fwd_bwd(self._logits_s, self._logits_t, self.dino_loss.center.view(-1), self.ncrops,
                                  float(self.dino_loss.student_temp), 0.04, K=self.K, grad=self.dlogits, ws=self.loss_ws,
                                  loss=self.loss, dev_temps=self.temps)
            call("lafs_colsum_f32", _p(self._logits_t), self.Kpad, 2 * B, self.K, _p(self.colsum))
        train_g = self.student.head.last_layer.weight_g.requires_grad
        self._head_states = (st_h, st_ht)
        return Fn.head_backward(sa, self.head_prefix_s, st_h, self.dlogits, train_g=train_g, overwrite_last=True)

    def _seg_trunk_backward(self, k):
        """Run k of the trunk backward: blocks cuts[k]-1 .. cuts[k+1]; run 0 starts with the final norm, the last run ends with
        the patch embedding and the position table."""
        sa = self.sa
        if k == 0:
            sync = self.sync_bn and self._bn_sums_live       # (the sums of all ranks: all-reduced between the segments)
            self._st["g"] = Fn.vit_backward_begin(sa, self.spec_s, self._st["vit"], self._st["dfeat"],
                                                  bn_sums=self.bn_x.sums if sync else None, bn_total=self.bn_total_s if sync else None)
        Fn.vit_backward_layers(self._st["vit"], self._st["g"], self.cuts[k], self.cuts[k + 1], wgrad_stream=self.side_stream)
        if k == len(self.cuts) - 2:
            gpe = sa.view(sa.grad, self.spec_s.prefix + self.pos_name).view(-1, self.spec_s.trunk.dim)
            # a table that is used as stored (Part-fViT slices, or a crop size equal to the table's grid) takes its gradient rows
            # directly; a resampled one goes through the transposed interpolation map
            direct = [gpe[:r * r + 1] if (self.facevit or M is None) else None for M, r in zip(self.interp, self.grids)]
            dpos = Fn.vit_backward_end(sa, self.spec_s, self._st["vit"], self._st["g"], dpos_out=direct)
            for M, dp, dr in zip(self.interp, dpos, direct):
                if dr is None:
                    call("lafs_pos_interp_bwd", _p(dp), _p(M), _p(gpe), M.shape[0], M.shape[1], self.spec_s.trunk.dim)

    def _update_piece(self, p):
        """Per-tensor gradient norms, clip + update rule + teacher EMA + bf16 shadows for the tensors of update piece p."""
        (lo, hi), (s_lo, s_hi) = self.pieces[p], self.piece_segs[p]
        self._update_range(lo // _lib.CHUNK, hi // _lib.CHUNK, s_lo, s_hi)

    def _update_adamw(self, c_lo, c_hi, s_lo, s_hi):
        sa, ta = self.sa, self.ta
        call("lafs_grad_sumsq_range", _p(sa.grad), _p(sa.chunk_seg), sa.n_chunks, sa.n_seg, c_lo, c_hi, s_lo, s_hi, _p(self.hyper),
             _p(sa.chunk_sumsq), _p(sa.seg_sumsq))
        call("lafs_clip_adamw_ema_range", _p(sa.master), _p(sa.grad), _p(sa.exp_avg), _p(sa.exp_avg_sq), _p(ta.master),
             _p(sa.shadow), _p(ta.shadow), _p(sa.chunk_seg), sa.n_chunks, c_lo, c_hi, _p(sa.seg_flags), _p(sa.seg_step), sa.n_seg,
             s_lo, s_hi, _p(sa.seg_sumsq), _p(self.hyper))

    def _update_sgd(self, c_lo, c_hi, s_lo, s_hi):
        sa = self.sa
        call("lafs_grad_sumsq_range", _p(sa.grad), _p(sa.chunk_seg), sa.n_chunks, sa.n_seg, c_lo, c_hi, s_lo, s_hi, _p(self.hyper),
             _p(sa.chunk_sumsq), _p(sa.seg_sumsq))
        self._momentum_step(_lib.UPDATE_SGD, None, c_lo, c_hi, s_lo, s_hi)

    def _update_lars(self, c_lo, c_hi, s_lo, s_hi):
        sa = self.sa
        call("lafs_grad_sumsq_trust_range", _p(sa.master), _p(sa.grad), _p(sa.chunk_seg), sa.n_chunks, sa.n_seg, c_lo, c_hi, s_lo, s_hi,
             _p(sa.seg_flags), _p(self.hyper), _p(self.chunk_part), _p(sa.seg_sumsq), _p(self.seg_trust))
        self._momentum_step(_lib.UPDATE_LARS, self.seg_trust, c_lo, c_hi, s_lo, s_hi)

    def _momentum_step(self, kind, trust, c_lo, c_hi, s_lo, s_hi):
        sa, ta = self.sa, self.ta
        call("lafs_clip_momentum_ema_range", kind, _p(sa.master), _p(sa.grad), _p(sa.exp_avg), _p(ta.master), _p(sa.shadow), _p(ta.shadow),
             _p(sa.chunk_seg), sa.n_chunks, c_lo, c_hi, _p(sa.seg_flags), _p(sa.seg_step), sa.n_seg, s_lo, s_hi, _p(sa.seg_sumsq),
             _p(trust), _p(self.hyper))

    def _seg_update(self):
        call("lafs_center_ema", _p(self.dino_loss.center), _p(self.colsum), self.K, 1.0 / (2 * self.B * self.world),
             float(self.dino_loss.center_momentum))

    def _with_pieces(self, k, body):
        """Segment k = `body` with the update pieces scheduled at k: on their own stream beside the body (forked at the start, joined
        at the end: the pattern hipGraph captures), or -- in the final segment -- in line, followed by the W^T shadow refresh."""
        here = [p for p, at in enumerate(self.piece_runs_at) if at == k]
        last = k == self.n_segments - 1
        cur = torch.cuda.current_stream()
        if here and not last and self.opt_stream is not None:
            self.opt_stream.wait_stream(cur)
            with torch.cuda.stream(self.opt_stream):
                for p in here:
                    self._update_piece(p)
            body()
            cur.wait_stream(self.opt_stream)
            return
        body()
        for p in here:
            self._update_piece(p)
        if last:
            self.sa.refresh_transposed()

    # ------------------------------------------------------------------ step
    def _step(self):
        """The device side of the step, once, in execution order.  A generator: on an engine with collectives to place (not _one_graph)
        it yields wherever the host has work between two kernels, and what it yields is that work, a callable -- all-reduces to launch,
        then the stream-side waits for what the next stretch reads.  _capture makes one hipGraph of every stretch between two yields
        (n_segments of them); without graphs step() drives the generator itself."""
        cut = not self._one_graph
        yield from self._forward()
        if cut:
            yield self._after_forward
        for k in range(len(self.cuts) - 1):
            self._with_pieces(self.n_fwd + k, lambda: self._seg_trunk_backward(k))
            if cut:
                yield partial(self._after_backward_run, k)
        self._with_pieces(self.n_segments - 1, self._seg_update)

    def _after_forward(self):
        # the BatchNorm backward's sums go out FIRST, the trunk backward waits for them alone; head gradients + center sums follow and
        # are on the wire (RCCL) while the trunk backward runs (arena order: [embed | blocks 0..depth-1 | norm | head])
        bn_tok = self.bn_x.reduce_sums() if self._bn_sums_live else None
        self._piece_tokens[0] = self._reduce_range(*self.pieces[0])
        self._center_tok = self.reducer.launch(self.colsum)
        self.reducer.wait([bn_tok])
        self._await(self.n_fwd)

    def _after_backward_run(self, k):
        if 1 + k < len(self.pieces):                     # this run's gradients go out as soon as its stretch has been enqueued
            self._piece_tokens[1 + k] = self._reduce_range(*self.pieces[1 + k])
        self._await(self.n_fwd + k + 1)

    def _await(self, k):
        """In front of stretch k the stream waits for what it reads: the update stretch for the center sums, an update piece for its
        reduced gradients."""
        if k == self.n_segments - 1:
            self.reducer.wait([self._center_tok])
        for p, at in enumerate(self.piece_runs_at):
            if at == k:
                self.reducer.wait(self._piece_tokens[p])

    def _capture(self):
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                       # warm-up outside capture (lazy inits, caches): the whole step, no host work
            for _ in self._step():
                pass
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        # (collectives between the graphs mean a process group, whose watchdog thread is alive during the capture)
        self._stretches, _ = capture_stretches(self._step(), thread_local=not self._one_graph)
        self._graphs = [g for g, _ in self._stretches]

    def set_inputs(self, crops):
        """crops: list of 2 global + n_local local crops (any device), copied into the static NCHW input buffers.  Each is an
        NCHW image or, as the reference feeds its Part-fViT pair (lafs_train.py:538-569), a [B, n, 192] tensor of '(p1 p2 c)'
        patch vectors of the landmark mosaic -- the same pixels in another order, re-indexed here."""
        for dst, src in zip(self.in_global + self.in_local, crops):
            if src.dim() == 3:
                src = Fn.unpatchify_grad(src, _lib.PATCH_ORDER_HWC)
            dst.copy_(src, non_blocking=True)

    def step(self, crops=None, *, lr, wd, momentum, teacher_temp, epoch, beta1=0.9, beta2=0.999, eps=1e-8):
        """One optimisation step.  Returns the device scalar loss (no host sync)."""
        if crops is not None:
            self.set_inputs(crops)
        def fill_hyper(h):
            h[_lib.HP_LR], h[_lib.HP_WD], h[_lib.HP_BETA1], h[_lib.HP_BETA2], h[_lib.HP_EPS] = lr, wd, beta1, beta2, eps
            h[_lib.HP_CLIP], h[_lib.HP_EMA_M] = self.clip_grad, momentum
            h[_lib.HP_FREEZE_LAST] = 1.0 if epoch < self.freeze_last_layer else 0.0
            h[_lib.HP_GRAD_SCALE] = 1.0 / self.world        # DDP mean of the summed gradients
            h[_lib.HP_STEP] = float(self.step_count % (1 << 24))
            h[_lib.HP_MOMENTUM], h[_lib.HP_LARS_ETA] = SGD_MOMENTUM, LARS_ETA

        def fill_temps(t):
            t[0], t[1] = float(self.dino_loss.student_temp), teacher_temp

        self.hyper_ring.upload(self.hyper, fill_hyper)
        self.temps_ring.upload(self.temps, fill_temps)
        if self.use_graph and self._graphs is None:
            saved = self._snapshot()
            self._capture()
            self._restore(saved)
            self.hyper_ring.upload(self.hyper, fill_hyper)
        if self.use_graph:                       # the host's work (collectives) sits between the graphs
            for g, act in self._stretches:
                g.replay()
                if act is not None:
                    act()
        else:
            for act in self._step():
                act()
        self.reducer.wait_all()
        self.step_count += 1
        return self.loss

    def _reduce_range(self, lo, hi):
        """Asynchronous SUM all-reduce of grad[lo:hi) minus the large frozen tensors inside it; returns the reducer's tokens."""
        return [self.reducer.launch(self.sa.grad[a:b]) for a, b in self._trainable_runs(lo, hi)]

    def _trainable_runs(self, lo, hi):
        runs, cur = [], lo
        for a, b in sorted(self._frozen_runs):
            if b <= cur or a >= hi:
                continue
            if a > cur:
                runs.append((cur, min(a, hi)))
            cur = max(cur, b)
        if cur < hi:
            runs.append((cur, hi))
        return runs

    # warm-up/capture executes real optimisation steps on whatever is in the buffers: snapshot and restore the state -- fViT's
    # BatchNorm buffers (running_mean, running_var, num_batches_tracked of both networks) included, which those passes update, and
    # those of a BatchNorm DINO head (head_forward steps them, the counters by a device add inside the captured forward)
    def _state_tensors(self):
        sa, ta = self.sa, self.ta
        bn = [b for m in ((self.bn_s, self.bn_t) if self.fvit else ()) for b in (m.running_mean, m.running_var, m.num_batches_tracked)]
        if self.head_bn:                             # the four BatchNorm1d of the two heads (mlp.1 / mlp.4)
            bn += [b for net in (self.student, self.teacher) for b in net.head.buffers()]
        moments = [sa.exp_avg] + ([sa.exp_avg_sq] if sa.exp_avg_sq is not None else [])        # (sgd / lars: one state buffer)
        return [sa.master] + moments + [sa.seg_step, ta.master, self.dino_loss.center] + bn

    def _snapshot(self):
        return [t.clone() for t in self._state_tensors()], torch.cuda.get_rng_state(self.device)

    def _restore(self, saved):
        tensors, rng = saved
        sa, ta = self.sa, self.ta
        for dst, src in zip(self._state_tensors(), tensors):
            dst.copy_(src)
        sa.refresh_shadows()
        ta.refresh_shadows()
        torch.cuda.set_rng_state(rng, self.device)

    # ------------------------------------------------------------------ checkpoint helpers (reference layout)
    def _adamw_order(self):
        """Parameter names in torch.optim.AdamW(utils.get_params_groups(student)) index order: the regularised group first
        (>= 2-D non-bias tensors), then the rest, each in named_parameters order (reference lafs_train.py:385-392,
        utils.py:662-673).  The reference registers every tensor with requires_grad=True -- including Part-fViT's CosFace
        `loss.weight`, which the SSL step never touches (gradient None: AdamW keeps no state for it, but it holds an index in the
        regularised group).  Here such a tensor is frozen in the arena and marked `_lafs_optimizer_registered` by
        build_backbones: it keeps its index and never gets a state entry."""
        reg, noreg = [], []
        for name, p in self.student.named_parameters():
            if p.requires_grad or getattr(p, "_lafs_optimizer_registered", False):
                (noreg if (name.endswith(".bias") or p.dim() == 1) else reg).append(name)
        return reg, noreg

    def _kind_of_state_dict(self, sd):
        """'adamw' | 'sgd' | 'lars' | None (cannot tell: no state entries and unknown group keys)."""
        for st in sd["state"].values():
            for kind, key in _STATE_KEY.items():
                if key in st:
                    return kind
        keys = set().union(*[set(g) for g in sd["param_groups"]]) if sd["param_groups"] else set()
        return 'adamw' if 'betas' in keys else 'lars' if 'eta' in keys else 'sgd' if 'nesterov' in keys else None

    def optimizer_state_dict(self):
        """The state_dict the reference's optimizer would have at this point -- the format the reference stores under
        checkpoint['optimizer'] and restores with optimizer.load_state_dict (lafs_train.py:428-463, utils.py:152-184).
          adamw  torch.optim.AdamW(get_params_groups(student)): per-parameter {step, exp_avg, exp_avg_sq}
          sgd    torch.optim.SGD(..., lr=0, momentum=0.9):       per-parameter {momentum_buffer, step}
          lars   utils.LARS(...):                                per-parameter {mu, step}
        An entry exists only for a tensor that has been stepped, like torch: the last layer has none while it is frozen.  `step`
        (the tensor's seg_step) is no key of torch's SGD or the reference's LARS, which both ignore it; with it a resume here
        continues the DropPath sequence exactly."""
        sa = self.sa
        reg, noreg = self._adamw_order()
        steps = sa.seg_step.cpu().tolist()
        h = self.hyper.cpu().tolist()
        state = {}
        for idx, name in enumerate(reg + noreg):
            t = steps[sa.names.index(name)]
            if t > 0:
                shape = sa.params[sa.names.index(name)].shape
                if self.optimizer == 'adamw':
                    state[idx] = {"step": torch.tensor(float(t)), "exp_avg": sa.view(sa.exp_avg, name, shape).detach().cpu().clone(),
                                  "exp_avg_sq": sa.view(sa.exp_avg_sq, name, shape).detach().cpu().clone()}
                else:
                    state[idx] = {_STATE_KEY[self.optimizer]: sa.view(sa.exp_avg, name, shape).detach().cpu().clone(),
                                  "step": torch.tensor(float(t))}
        if self.optimizer == 'adamw':
            common = {"lr": h[_lib.HP_LR], "betas": (h[_lib.HP_BETA1] or 0.9, h[_lib.HP_BETA2] or 0.999), "eps": h[_lib.HP_EPS] or 1e-8,
                      "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None}
        elif self.optimizer == 'sgd':
            # lr, momentum, dampening, weight_decay, nesterov + whatever keys the installed torch adds (maximize, foreach, ...)
            common = dict(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0, momentum=SGD_MOMENTUM).defaults, lr=h[_lib.HP_LR])
        else:
            common = {"lr": h[_lib.HP_LR], "weight_decay": 0.0, "momentum": SGD_MOMENTUM, "eta": LARS_ETA, "weight_decay_filter": None,
                      "lars_adaptation_filter": None}
        groups = [dict(common, weight_decay=h[_lib.HP_WD], params=list(range(len(reg)))),
                  dict(common, weight_decay=0.0, params=list(range(len(reg), len(reg) + len(noreg))))]
        return {"state": state, "param_groups": groups}

    def load_optimizer_state_dict(self, sd):
        """Inverse of optimizer_state_dict; also accepts a checkpoint written by the reference itself (same format).  The reference's
        SGD / LARS entries carry no step count: their tensors get seg_step = 1 (stepped at least once) and the caller sets
        step_count from the epoch (lafs_train.py here)."""
        if "state" not in sd or "param_groups" not in sd:
            raise _lib.LafsHipError("checkpoint['optimizer'] is not a torch.optim.AdamW state_dict (keys: %s)" % sorted(sd))
        kind = self._kind_of_state_dict(sd)
        if kind is not None and kind != self.optimizer:
            raise _lib.LafsHipError(f"checkpoint['optimizer'] is the state of optimizer '{kind}', this engine was built with "
                                    f"optimizer '{self.optimizer}'")
        sa = self.sa
        reg, noreg = self._adamw_order()
        names = reg + noreg
        sizes = [len(g["params"]) for g in sd["param_groups"]]
        if sizes != [len(reg), len(noreg)]:
            raise _lib.LafsHipError(f"optimizer param_groups of sizes {sizes} do not fit this model ({len(reg)} regularised + "
                                    f"{len(noreg)} other tensors)")
        sa.exp_avg.zero_(); sa.seg_step.zero_()
        if sa.exp_avg_sq is not None:
            sa.exp_avg_sq.zero_()
        steps = sa.seg_step.cpu()
        flat = [i for g in sd["param_groups"] for i in g["params"]]
        key = _STATE_KEY[self.optimizer]
        for pos, idx in enumerate(flat):
            st = sd["state"].get(idx)
            if st is None or st.get(key) is None:            # (torch's SGD stores momentum_buffer = None for a tensor it never stepped)
                continue
            name = names[pos]
            shape = sa.params[sa.names.index(name)].shape
            sa.view(sa.exp_avg, name, shape).copy_(st[key])
            if self.optimizer == 'adamw':
                sa.view(sa.exp_avg_sq, name, shape).copy_(st["exp_avg_sq"])
            steps[sa.names.index(name)] = int(float(st["step"])) if "step" in st else 1
        sa.seg_step.copy_(steps)
        # the per-step DropPath masks are seeded with the step count: continue the sequence of the interrupted run
        self.step_count = int(steps.max()) if steps.numel() else 0
