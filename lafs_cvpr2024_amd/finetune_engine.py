"""Fused Part-fViT / fViT + CosFace fine-tune micro-step (reference train_largescale.py:785-891) on the HIP kernels.

    u8 batch -> (x/255*2-1) + batch mixup (one kernel) -> [trainable landmark CNN -> theta -> patch gather] -> Part-fViT trunk ->
    L2-normalised embedding x L2-normalised class centres (MFMA GEMM) -> fused margin + softmax + soft-target CE (the dense [B, C]
    mixup target is never built: it has <= 2 non-zeros per row) -> backward -> every `acc_step` micro-steps: AdamW over the flat arena.
The rest of the reference's mixing recipe (CutMix, pair / elem modes, label smoothing: util/mixup_my.py, train_largescale.py:383-395)
runs through lafs_mix_normalize and lafs_margin_softmax_ce_mix_bf16, driven by one parameter row per sample that is uploaded per
micro-step and read by the kernels when they run; with the reference's defaults the step launches exactly what it launched before.

Round 4: every per-step tensor is allocated once, no ATen kernel is left in a micro-step (labels, DropPath masks, operand
transposes, the image gradient re-indexing and the gradient zeroing are lafs_* launches), the mixup lambda / step counter are read
from device memory, and the whole micro-step is ONE hipGraph (two captured variants: the first micro-step of an accumulation
window WRITES the block and class-table weight gradients instead of accumulating into a zeroed 1 GB arena).

Round 6, data-parallel runs (reference: DistributedDataParallel(broadcast_buffers=True), train_largescale.py:676-677): parameters and
buffers are broadcast from rank 0 at construction; the micro-steps of an accumulation window that reduce nothing are the same single
graph as on one rank (deferred weight gradients included), and the window's LAST micro-step -- whose gradient slices go out over RCCL
as the backward retires them -- is captured as one hipGraph per segment with the FlatReducer launches between the replays, exactly as
LafsPretrainEngine does.  Only the class-sharded head keeps the eager form (its collectives sit inside the head itself).

Landmark teacher (reference `pre_land` / `keep_land`, train_largescale.py:435-437, 565-582, 807-843): a frozen stage-1 CNN, run in line
on the mixed batch as an inference plan, either supplies the patches the trunk is fed (mode A: backbone without a branch) or labels
the batch for the backbone's own branch (mode B: lafs_landmark_mse between the gather's backward and the CNN's; the epoch's weight is
read from the hyper-parameter vector, so the captured micro-step serves every epoch).  Without a teacher nothing changes.

fViT (ViTs_face_overlap, `--net VITs`): the same step with the overlapping window embedding (lafs_unfold_bf16 in front of the embedding
GEMM, the window geometry) and the BatchNorm1d head on the cls rows (lafs_bn1d_fwd / lafs_bn1d_bwd: batch statistics and the running-
statistic update in training mode, running statistics in eval mode); no landmark branch.  `num_batches_tracked` is counted on the
host, one per training micro-step, and added to the buffer when a state_dict is taken (flush_batches_tracked).  Data-parallel: every
rank normalises with its own batch statistics, as the reference's plain DDP does (no SyncBatchNorm).
"""
import os

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, functional as Fn, ops
from .face_pre_pro.ViT_face import AdaFace, ViT_face_landmark_patch8, ViTs_face_overlap
from .distributed import FlatReducer
from .ops import _p, call
from .utils import PinnedRing, capture_stretches
from .vision_transformer import attach_arena

f32, bf16 = torch.float32, torch.bfloat16


LOW_WEIGHT_DECAY = 5e-2


def finetune_decay_group(name, param):
    """Weight-decay class of a fine-tune parameter, as param_groups_lrd assigns it (reference train_largescale.py:139-149):
    1-D tensors do not decay, the landmark CNN's matrices (`stn*`) decay at 5e-2, everything else at the configured rate
    (1e-1).  The `lr_scale` the reference also stores per group is never applied by torch's AdamW."""
    if param.dim() == 1:
        return "none"
    return "low" if name.startswith("stn") else "decay"


class FinetuneEngine:
    def __init__(self, backbone: ViT_face_landmark_patch8, batch_size, acc_step=3, mixup_alpha=0.2, mixup_prob=0.1,
                 s=64.0, m=0.4, margin_type=0, image_size=112, device=None, sharded_head=None, use_graph=None,
                 cutmix_alpha=0.0, cutmix_minmax=None, switch_prob=0.5, mix_mode="batch", label_smoothing=0.0,
                 landmark_teacher=None, keep_land=False, ada_h=0.333, ada_t_alpha=0.01):
        """margin_type 0 = CosFace (the reference), 1 = ArcFace (parity unpinned), on the dense `backbone.loss.weight` head; 2 = AdaFace
        (parity unpinned; `backbone.loss` must be an AdaFace, m = 0.4): lafs_adaface_margins forms a margin pair per row from the
        embedding norms behind lafs_l2norm_fwd and moves the module's `batch_mean` / `batch_std` buffers -- whose storage it is handed --
        once per training micro-step (ada_h: the norm-to-margin slope, ada_t_alpha: the statistics' EMA rate); dense head only;
        `sharded_head` (a partial_fc.PartialFC) replaces it by the class-sharded head (CosFace: mixup targets as on the dense head).
        use_graph: None = capture the micro-step whenever it is capturable (single rank, dense head; LAFS_FT_GRAPH=0 disables).
        cutmix_alpha / cutmix_minmax / switch_prob / mix_mode / label_smoothing: util.mixup_my.Mixup's arguments of the same meaning
        (train_largescale.py:528-531).  Any of them away from the reference's default (0, None, -, 'batch', 0) selects the per-row
        kernels; label smoothing needs the dense CosFace head.
        landmark_teacher / keep_land: the reference's `pre_land` / `keep_land` (train_largescale.py:435-437, 565-582, 807-836).  The
        teacher is any module with `.stn` and `.output_layer` (face_landmark_4simmin_glo_loc); its weights are frozen HERE into an
        inference plan (eval mode, not in the optimizer).  keep_land=False (mode A, a backbone with with_land=False): the teacher's
        landmarks gather the patches the trunk is fed, no gradient flows into them.  keep_land=True (mode B, with_land=True): the
        backbone keeps its own branch, whose landmarks are regressed onto the teacher's (lafs_landmark_mse, weight `land_weight` of
        micro_step): `loss` includes weight / acc_step * loss_land, `loss_land` holds the unweighted mean."""
        if mix_mode not in ("batch", "pair", "elem"):
            raise _lib.LafsHipError(f"mix_mode must be 'batch', 'pair' or 'elem', not {mix_mode!r}")
        if not 0.0 <= label_smoothing < 1.0:
            raise _lib.LafsHipError("label_smoothing must lie in [0, 1)")
        if label_smoothing > 0.0 and sharded_head is not None:
            raise _lib.LafsHipError("label smoothing on the class-sharded head is not supported (a smoothed target over a sampled class "
                                    "subset is not defined here): use the dense CosFace head")
        if margin_type not in (0, 1, 2):
            raise _lib.LafsHipError("margin_type must be 0 (CosFace), 1 (ArcFace) or 2 (AdaFace)")
        if margin_type == 2 and sharded_head is not None:
            raise _lib.LafsHipError("AdaFace (margin_type 2) runs on the dense head: its class-sharded form is not built")
        if label_smoothing > 0.0 and margin_type == 2:
            raise _lib.LafsHipError("label smoothing needs the CosFace margin: AdaFace has no margin for a dense target")
        if label_smoothing > 0.0 and margin_type != 0:
            raise _lib.LafsHipError("label smoothing needs the CosFace margin: ArcFace has no margin for a dense target")
        if keep_land and landmark_teacher is None:
            raise _lib.LafsHipError("keep_land regresses the backbone's landmarks onto a teacher's: it needs a landmark_teacher")
        if landmark_teacher is not None:
            if isinstance(backbone, ViTs_face_overlap):
                raise _lib.LafsHipError("a landmark teacher needs Part-fViT (ViT_face_landmark_patch8): fViT embeds overlapping windows of "
                                        "the image, not landmark patches")
            own = bool(getattr(backbone, "with_land", False))
            if keep_land and not own:
                raise _lib.LafsHipError("keep_land=True supervises the backbone's own landmark branch: it needs with_land=True")
            if not keep_land and own:
                raise _lib.LafsHipError("a landmark teacher without keep_land feeds the trunk the teacher's patches: the backbone must "
                                        "have no branch of its own (with_land=False)")
            if not (hasattr(landmark_teacher, "stn") and hasattr(landmark_teacher, "output_layer")):
                raise _lib.LafsHipError("the landmark teacher needs `.stn` and `.output_layer` (face_landmark_4simmin_glo_loc)")
        if not isinstance(backbone, (ViT_face_landmark_patch8, ViTs_face_overlap)) or (sharded_head is None and not hasattr(backbone, "loss")):
            raise _lib.LafsHipError("FinetuneEngine drives ViT_face_landmark_patch8 or ViTs_face_overlap with loss_type='CosFace', or "
                                    "either of them with a sharded head")
        if sharded_head is None and (margin_type == 2) != isinstance(backbone.loss, AdaFace):
            raise _lib.LafsHipError("margin_type 2 and a backbone built with loss_type='AdaFace' go together: the engine updates that "
                                    f"module's batch_mean / batch_std (margin_type {margin_type}, loss {type(backbone.loss).__name__})")
        if batch_size % 8:
            raise _lib.LafsHipError("FinetuneEngine needs a batch size that is a multiple of 8 (16-byte rows in the class-gradient GEMM)")
        self.device = torch.device(device if device is not None else ("cuda", torch.cuda.current_device()))
        self.model, self.B, self.acc_step = backbone, batch_size, acc_step
        self.fvit = isinstance(backbone, ViTs_face_overlap)          # window embedding + BatchNorm1d head, no landmark branch
        self.with_land = bool(getattr(backbone, "with_land", False))
        self.mixup_alpha, self.mixup_prob = mixup_alpha, mixup_prob
        self.label_smoothing = float(label_smoothing)
        # per-row mixing (CutMix, pair / elem modes, smoothing): the reference's own class draws the parameters
        self.mix_rows = cutmix_alpha > 0.0 or cutmix_minmax is not None or mix_mode != "batch" or label_smoothing > 0.0
        self.mixer = None
        if self.mix_rows:
            from .util.mixup_my import Mixup
            self.mixer = Mixup(mixup_alpha=mixup_alpha, cutmix_alpha=cutmix_alpha, cutmix_minmax=cutmix_minmax, prob=mixup_prob,
                               switch_prob=switch_prob, mode=mix_mode, label_smoothing=label_smoothing)
        self.s, self.m, self.margin_type = float(s), float(m), margin_type
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.arena = attach_arena(backbone, self.device)
        self.arena.set_decay_groups(finetune_decay_group)
        self.ctx = _lib.Ctx(self.device)                 # this engine's side streams / events / kernel options (lafs_ctx)
        self.arena.ctx = self.ctx
        self.cnn_flush = None
        self.bn_forward = 0                              # fViT: training forwards of the BatchNorm1d head since the last flush (below)
        if self.world > 1:
            # DDP's construction-time broadcast of parameters AND buffers from rank 0 (train_largescale.py:676-677; before the landmark
            # plan below takes its references to the BatchNorm statistics).  DDP also re-broadcasts the buffers before every forward:
            # in training mode the BatchNorm layers normalise with batch statistics, the running statistics are only written, and
            # only rank 0 saves checkpoints (train_largescale.py:899-910) -- rank 0's buffers evolve as under DDP and the other ranks'
            # copies are never read; sync_buffers() makes every rank hold rank 0's values (before an evaluation on all ranks).
            dist.broadcast(self.arena.master, 0)
            self.arena.refresh_shadows()
            self.sync_buffers()
        self.head = sharded_head
        # AdaFace: the kernel's `state` operand IS the storage of loss.batch_mean / loss.batch_std, so a state_dict holds the live values
        self.ada_h, self.ada_t_alpha = float(ada_h), float(ada_t_alpha)
        self.ada_state = backbone.loss.state_storage() if margin_type == 2 else None
        self.C = backbone.loss.out_features if sharded_head is None else 8
        self.Cpad = (self.C + 127) // 128 * 128
        self.D = backbone.dim
        self.S = image_size
        self.geom = Fn.geometry([(batch_size, image_size)], self.device,
                                window=(backbone.ac_patch_size, backbone.patch_size, backbone.pad) if self.fvit else None)
        if self.fvit and self.geom.npatch(0) > backbone.num_patches:
            raise _lib.LafsHipError(f"a {image_size}-pixel image unfolds into {self.geom.npatch(0)} windows, the position table holds "
                                    f"{backbone.num_patches}")
        dev, a, m, B, D = self.device, self.arena, backbone, batch_size, self.D
        self.hyper = torch.zeros(_lib.HP_COUNT, device=dev, dtype=f32)
        self.hyper_ring = PinnedRing((_lib.HP_COUNT,), f32)     # asynchronous upload; a pageable copy would block the host
        self._hp = {}                                            # host copy of the hyper-parameters (every upload rewrites the whole vector)
        if self.mix_rows:                                        # the micro-step's parameter rows (lafs_hip.h LAFS_MIX_*), uploaded the same way
            self.mix_tab = torch.zeros(batch_size, _lib.MIX_WORDS, device=dev, dtype=torch.int32)
            self.mix_ring = PinnedRing((batch_size, _lib.MIX_WORDS), torch.int32)
        # data parallelism (reference: DDP bucketed all-reduce overlapped with backward, train_largescale.py:676-677, 867): on the
        # last micro-step of an accumulation window the flat gradient goes out over RCCL in slices AS THE BACKWARD RETIRES
        # THEM -- the 0.6 GB margin head first (it is final before the trunk backward starts), then runs of blocks from the top,
        # last the embedding / landmark-CNN range -- and optimizer_step only waits.  Reducing once per window instead of once
        # per micro-step is the same sum (no_sync semantics).
        self.reducer = FlatReducer()
        self.grad_slices = 4
        names = m._spec.trunk.block_names
        self.block0 = a.offsets[names[0]["ln1_g"]]
        self.block_off = [a.offsets[n["ln1_g"]] for n in names] + [a.offsets[m._spec.prefix + m._spec.final_g]]
        self.wname = m._spec.prefix + "loss.weight"
        self.head_off = a.offsets[self.wname] if (sharded_head is None) else a.size
        self._reduced = False
        # tensors whose gradient is WRITTEN by its producer on the first micro-step of an accumulation window (block weights: wgrad
        # fold with accumulate = 0; class table: weight-norm backward): that micro-step zeroes only the others (lafs_zero_chunks)
        flags = a.seg_flags.cpu().tolist()
        over = {nm[k] for nm in names for k in ("w_qkv", "w_proj", "w_fc1", "w_fc2")}
        if sharded_head is None:
            over.add(self.wname)
        for i, name in enumerate(a.names):
            if name in over:
                flags[i] |= _lib.SEG_OVERWRITTEN
        a.seg_flags.copy_(torch.tensor(flags, dtype=torch.int32))
        # ---- static buffers of a micro-step
        S = image_size
        self.in_u8 = torch.zeros(B, 3, S, S, device=dev, dtype=torch.uint8)
        self.y1 = torch.zeros(B, device=dev, dtype=torch.int32)
        self.x = torch.empty(B, 3, S, S, device=dev, dtype=f32)
        self.img_in = torch.empty(B, 3, S, S, device=dev, dtype=f32)
        self.loss = torch.zeros(1, device=dev, dtype=f32)
        self.g_buf = torch.empty(self.geom.n_tok, D, device=dev, dtype=f32)
        self.x_in = torch.empty(self.geom.n_tok, D, device=dev, dtype=f32)
        self.x_out = torch.empty(self.geom.n_tok, D, device=dev, dtype=f32)
        self.demb = torch.empty(B, D, device=dev, dtype=f32)
        self.drop = (torch.empty(m.depth, 2, self.geom.n_seq, device=dev, dtype=f32) if m.drop_path_rate else None)
        self.keep = (torch.full((m.depth,), 1.0 - m.drop_path_rate, device=dev, dtype=f32) if m.drop_path_rate else None)
        self.drop_seed = 0x0F17E
        self.pos_rows = a.view(a.master, m._spec.prefix + "pos_embedding").view(-1, D)[: self.geom.npatch(0) + 1]
        self.dpos_rows = a.view(a.grad, m._spec.prefix + "pos_embedding").view(-1, D)[: self.geom.npatch(0) + 1]
        if sharded_head is None:
            self.ones = torch.ones(self.C, device=dev, dtype=f32)
            self.cos = torch.empty(B, self.Cpad, device=dev, dtype=f32)
            self.dcos = torch.zeros(B, self.Cpad, device=dev, dtype=bf16)
            self.dcos_t = torch.zeros(self.Cpad, B, device=dev, dtype=bf16)
            self.wn = torch.empty(self.Cpad, D, device=dev, dtype=bf16)
            self.inv_w = torch.empty(self.C, device=dev, dtype=f32)
            self.dwn = torch.empty(self.Cpad, D, device=dev, dtype=f32)
            self.row_ws = torch.empty(B, device=dev, dtype=f32)
            self.part_ws = torch.empty(B * (48 if self.mix_rows else 32), device=dev, dtype=f32)
            self.xn = torch.empty(B, D, device=dev, dtype=bf16)
            self.xn_t = torch.empty(D, B, device=dev, dtype=bf16)
            self.inv_x = torch.empty(B, device=dev, dtype=f32)
            self.row_margin = torch.empty(B, 2, device=dev, dtype=f32) if margin_type == 2 else None      # AdaFace (g_ang, g_add)
            self.dxn = torch.empty(B, D, device=dev, dtype=f32)
            self.dxn_ws = ops.wgrad_workspace(self.Cpad, B, D, dev)                 # d(emb_n): reduction over the classes
            self.dwn_ws = None if B % 32 == 0 else ops.wgrad_workspace(B, self.Cpad, D, dev)
        self.dmosaic = torch.empty(B, 3, S, S, device=dev, dtype=f32) if self.with_land else None
        self.dth, self.th, self.emb = None, None, None
        # frozen stage-1 teacher (pre_land): its inference plan runs in line on the main stream, on the mixed batch `x`, no jitter, no
        # selection (train_largescale.py:807-812); `land_label` is its min-max scaled theta in [0, 111]
        self.teacher, self.keep_land, self.land_label, self.loss_land, self._land_fixed = None, bool(keep_land), None, None, None
        self.land_weight = 1000.0                        # (the reference's weight of epoch 0 until micro_step is given one)
        if landmark_teacher is not None:
            from .landmark_cnn import HipLandmarkCNN
            self.teacher = HipLandmarkCNN(landmark_teacher, dev)
            self.land_n = self.teacher.n_out // 2
            if 64 * self.land_n != S * S or (keep_land and self.land_n != m.row_num * m.row_num):
                raise _lib.LafsHipError(f"the teacher regresses {self.land_n} landmarks: its 8 x 8 patches do not tile the trunk's "
                                        f"{S}-pixel input" + (" / the backbone's branch regresses another number" if keep_land else ""))
            self.land_label = torch.zeros(B, self.land_n, 2, device=dev, dtype=f32)
            self.loss_land = torch.zeros(1, device=dev, dtype=f32)
        self.micro = 0                                   # micro-steps taken (seeds the per-step masks)
        self._since_opt = 0                              # ... since the last optimizer step
        # optimizer_step leaves the (dead) gradients in place: the next micro-step zeroes / overwrites them itself.  True restores
        # "gradients are zero after a step" for callers that inspect arena.grad / p.grad afterwards (a 1 GB memset per step at C4)
        self.zero_after_step = False
        # trainable landmark branch: the HIP plan (landmark_train.HipLandmarkTrainer) in training mode (BatchNorm batch statistics,
        # Dropout(0.5)) and in eval mode (running statistics as constants of the backward, no dropout); LAFS_FT_CNN=torch, for A/B
        # runs, takes the nn.Module on torch autograd
        self.cnn = None
        if self.with_land and os.environ.get("LAFS_FT_CNN", "hip") == "hip":
            from .landmark_train import HipLandmarkTrainer
            self.cnn = HipLandmarkTrainer(m, a, batch_size, image_size, device=dev)
            self.cnn.step_dev = self.hyper[_lib.HP_STEP:]
            m.register_state_dict_pre_hook(lambda *a_, **k_: self.cnn.flush_batches_tracked())
            self.cnn_flush = self.cnn.flush_batches_tracked
        # fViT's BatchNorm1d head: nn.BatchNorm1d.num_batches_tracked += 1 per training forward, counted here and flushed when a
        # state_dict is taken (as the landmark plan does): no ATen increment inside or beside a micro-step
        if self.fvit:
            m.register_state_dict_pre_hook(lambda *a_, **k_: self.flush_batches_tracked())
        # streams / graphs
        # (The blocks' weight gradients on a second stream INSIDE the chain were measured neutral at C4 -- 27.24 ms with, 27.03 without --
        # and removed in round 5: tools/lab/NOTES.md.  What pays is deferring them beside the landmark CNN's backward, below.)
        self.wgrad_workgroups = 0
        # Deferred weight gradients (single GPU, HIP landmark plan): the trunk backward launches only its input-gradient chain and keeps
        # every block's dY operands; the twelve grouped weight-gradient launches then run on a second stream BESIDE the landmark
        # CNN's backward -- ~300 small launch-latency-sized kernels that leave most of the chip idle -- capped to
        # LAFS_FT_DEFER_WG workgroups so that the CNN's kernels find free CUs.  Measured at C4 (tools/lab/NOTES.md): the same launches
        # cost 4.5 ms in front of the CNN backward and 2.75 ms beside it.  LAFS_FT_WGRAD_DEFER=0 restores the immediate form.
        # (data-parallel runs: on every micro-step of a window but the last, whose gradient slices leave as the backward retires them)
        self.defer = (self.cnn is not None and sharded_head is None
                      and os.environ.get("LAFS_SINGLE_STREAM") != "1" and os.environ.get("LAFS_FT_WGRAD_DEFER", "1") != "0")
        self.defer_stream = torch.cuda.Stream(device=dev) if self.defer else None
        if self.defer:
            self.wgrad_workgroups = int(os.environ.get("LAFS_FT_DEFER_WG", "128"))
        if use_graph is None:
            use_graph = os.environ.get("LAFS_FT_GRAPH", "1") != "0"
        self.use_graph = bool(use_graph) and sharded_head is None
        self._graphs, self._readout = {}, {}
        self._pool = None
        self._ws = None

    def flush_batches_tracked(self):
        """fViT: the head's num_batches_tracked += the training micro-steps run since the last flush (the counter only matters for
        state_dict parity -- the momentum is a constant -- so it is brought up to date when a state_dict is taken)."""
        if self.bn_forward:
            self.model.mlp_head[0].num_batches_tracked.add_(self.bn_forward)
            self.bn_forward = 0

    def sync_buffers(self):
        """Every rank takes rank 0's buffers (BatchNorm running statistics and counters of the landmark CNN / of fViT's head): what
        DDP's broadcast_buffers does in front of every forward (train_largescale.py:676-677)."""
        if self.world > 1:
            if self.cnn_flush is not None:
                self.cnn_flush()
            self.flush_batches_tracked()
            for b in self.model.buffers():
                dist.broadcast(b, 0)

    def _defer_now(self):
        """Deferred weight gradients on this micro-step?  Not on the one that completes a data-parallel window: its gradient
        ranges are handed to the collective run by run, so every block's weight gradients have to exist when its run ends."""
        return self.defer and not self._reduce_now()

    # ------------------------------------------------------------------ host side of a micro-step
    def draw_lambda(self):
        if np.random.rand() < self.mixup_prob:
            return float(np.random.beta(self.mixup_alpha, self.mixup_alpha))
        return 1.0

    def draw_mix(self):
        """(lam f32 [B], cut bool [B], box i32 [B, 4]) of this micro-step from util.mixup_my.Mixup.draw_params: the global np.random
        stream moves exactly as the reference's Mixup.__call__ moves it."""
        if not (self.mixup_alpha > 0.0 or self.mixer.cutmix_alpha > 0.0):
            return np.ones(self.B, np.float32), np.zeros(self.B, bool), np.zeros((self.B, 4), np.int32)
        return self.mixer.draw_params(self.B, (self.S, self.S))

    def _upload_mix(self, mix):
        """Validate one micro-step's per-row parameters and send them to the device table (pinned ring, outside the graph)."""
        B, S = self.B, self.S
        lam = np.array(np.broadcast_to(np.asarray(mix[0], dtype=np.float32), (B,)))      # (an own, writable copy)
        cut = np.zeros(B, bool) if mix[1] is None else np.broadcast_to(np.asarray(mix[1], dtype=bool), (B,))
        box = np.zeros((B, 4), np.int32) if mix[2] is None else np.broadcast_to(np.asarray(mix[2], dtype=np.int32), (B, 4))
        if not (np.all(lam >= 0.0) and np.all(lam <= 1.0)):
            raise _lib.LafsHipError("mixing lambdas must lie in [0, 1]")
        if np.any(box < 0) or np.any(box > S):
            raise _lib.LafsHipError(f"CutMix boxes must lie inside the {S}x{S} image")
        if self.head is not None and self.head.margin_type != 0:
            lam, cut = np.ones(B, np.float32), np.zeros(B, bool)      # ArcFace on the sharded head takes hard labels, unmixed images
        self._mix = (lam, cut, box)

        def fill(h):
            h.zero_()
            v = h.numpy()
            v[:, _lib.MIX_LAM] = lam.view(np.int32)
            v[:, _lib.MIX_CUT] = cut
            v[:, _lib.MIX_YL:_lib.MIX_XH + 1] = box
        self.mix_ring.upload(self.mix_tab, fill)

    def _upload_hyper(self, kw):
        self._hp.update(kw)

        def fill(h):
            h.zero_()
            for k, v in self._hp.items():
                h[k] = v
        self.hyper_ring.upload(self.hyper, fill)

    def _stage(self, inputs_u8, labels):
        """Copy the batch into the static buffers the captured step reads (no ATen math: one copy, one lafs_cast_i64_i32)."""
        if inputs_u8.shape != self.in_u8.shape or inputs_u8.dtype != torch.uint8:
            raise _lib.LafsHipError(f"expected a uint8 batch of shape {tuple(self.in_u8.shape)}")
        self.in_u8.copy_(inputs_u8, non_blocking=True)
        lab = labels if labels.is_cuda else labels.to(self.device, non_blocking=True)
        if lab.dtype == torch.int64:
            call("lafs_cast_i64_i32", _p(lab.contiguous()), _p(self.y1), self.B)
        else:
            self.y1.copy_(lab.to(torch.int32))

    def _capturable(self):
        m = self.model
        return self.use_graph and (not self.with_land or self.cnn is not None)

    def set_landmark_labels(self, labels):
        """Parity hook (as set_droppath_scales of the LAFS engine): use `labels` f32 [B, n, 2] as the teacher's landmarks instead of
        running its plan; None restores the plan.  Set it before the first capture: a captured micro-step keeps what it captured."""
        if self.teacher is None:
            raise _lib.LafsHipError("set_landmark_labels needs an engine built with a landmark_teacher")
        if self._graphs:
            raise _lib.LafsHipError("set_landmark_labels must be called before the micro-step is captured")
        if labels is None:
            self._land_fixed = None
            return
        if tuple(labels.shape) != tuple(self.land_label.shape):
            raise _lib.LafsHipError(f"expected landmark labels of shape {tuple(self.land_label.shape)}")
        self._land_fixed = labels.detach().to(self.device, f32).contiguous().clone()

    def _teacher_labels(self):
        """The frozen teacher on the mixed batch -> f32 [B, n, 2] landmarks in [0, 111] (a static buffer)."""
        if self._land_fixed is not None:
            return self._land_fixed
        t = self.teacher(self.x)
        call("lafs_landmark_theta", _p(t), self.B, self.land_n, None, 0.0, None, self.land_n, _p(self.land_label))
        return self.land_label

    def micro_step(self, inputs_u8, labels, lam=None, mix=None, land_weight=None):
        """One forward/backward on a uint8 NCHW batch.  Gradients accumulate in the arena (loss pre-divided by acc_step).
        lam: this micro-step's lambda instead of a draw (one blend lambda for the whole batch).  mix = (lam [B], cut [B] or None, box
        [B, 4] or None): explicit per-row parameters as Mixup.draw_params returns them (engines built with a per-row option only).
        The FIRST micro-step after an optimizer step overwrites / zeroes the gradients itself: between optimizer_step and the next
        micro_step, arena.grad and p.grad hold the previous window's (stale) gradients unless `zero_after_step` is set.
        land_weight: this epoch's land_loss_control (mode B); None keeps the last one.  It travels in the hyper-parameter vector and
        is read by the kernel when it runs: a new weight is no new capture."""
        a, m = self.arena, self.model
        a.ensure_fresh()
        if mix is not None and not self.mix_rows:
            raise _lib.LafsHipError("per-row mixing parameters need an engine built with cutmix / mix_mode / label_smoothing")
        if self.mix_rows:
            self._upload_mix(mix if mix is not None else ((lam, None, None) if lam is not None else self.draw_mix()))
            lam = 1.0                                    # (the scalar lambda of the batch-mode kernels is not read)
        else:
            lam = self.draw_lambda() if lam is None else float(lam)
        if self.head is not None and self.head.margin_type != 0:
            lam = 1.0                                    # ArcFace on the sharded head takes hard labels (parity unpinned either way)
        self._lam = lam
        self._stage(inputs_u8, labels)
        self._labels = labels
        # (the counter seeds the DropPath / dropout / CNN-dropout masks; fp32 holds integers exactly below 2^24: wrap like the LAFS engine)
        if land_weight is not None:
            self.land_weight = float(land_weight)
        hyper = {_lib.HP_MIX_LAM: lam, _lib.HP_STEP: float((self.micro + 1) % (1 << 24))}
        if self.teacher is not None and self.keep_land:
            hyper[_lib.HP_LAND_W] = self.land_weight
        self._upload_hyper(hyper)
        first = (self._since_opt == 0)                   # first micro-step since the last optimizer step: gradients are written, not accumulated
        if self._capturable():
            key = (first, bool(m.training), self._reduce_now())
            segs = self._graphs.get(key)
            if segs is None:
                segs = self._capture(first)
                self._graphs[key] = segs
                self._readout[key] = (self.th, self.emb)     # (every captured variant writes buffers of its own)
            self.th, self.emb = self._readout[key]
            for g, out in segs:                          # one graph per segment; the gradient range a segment completes goes out behind it
                g.replay()
                if out is not None:
                    self.reducer.launch(out)
            if key[2]:
                self._reduced = True
            if self._cnn_hip and m.training:             # nn.BatchNorm2d.num_batches_tracked: one training forward of the landmark CNN per replay
                self.cnn.n_forward += 1
        else:
            self._body(first)
        if self.fvit and m.training:                     # nn.BatchNorm1d.num_batches_tracked: one training forward per micro-step
            self.bn_forward += 1
        self.micro += 1
        self._since_opt += 1
        return self.loss

    def _warmup(self, first):
        """One eager micro-step body on a side stream BEFORE the first capture (as LafsPretrainEngine._capture does): code objects
        are loaded, kernel attributes set and the per-step workspaces (`_ws`, `dth`) allocated by the ordinary allocator instead of
        from inside a stream capture / the graph's private pool.  The state the body mutates -- gradients, the loss, the landmark
        CNN's BatchNorm running statistics and loss-scale state, the running statistics of fViT's head, AdaFace's norm statistics -- is
        snapshotted and put back (a first step counted twice would be a 10 % error of the statistics at momentum 0.1)."""
        a, cnn = self.arena, self.cnn
        bn = []
        if self.fvit:
            head = self.model.mlp_head[0]
            bn = [head.running_mean, head.running_var]
        if cnn is not None:
            bn += [t for s in [cnn.stem["bn"]] + [L[k] for L in cnn.blocks for k in ("bn1", "bn2", "bn3")] for t in (s["rm"], s["rv"]) if t is not None]
            bn.append(cnn.gscale)
        if self.ada_state is not None:
            bn.append(self.ada_state)
        saved = [t.clone() for t in [a.grad, self.loss] + bn]
        n_fwd = cnn.n_forward if cnn is not None else 0
        cur = torch.cuda.current_stream()
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            self._body(first)                            # (a window's last micro-step: its all-reduces really run, on every rank alike)
            self.reducer.wait_all()
        self._reduced = False
        cur.wait_stream(s)
        torch.cuda.synchronize()
        for dst, src in zip([a.grad, self.loss] + bn, saved):
            dst.copy_(src)
        if cnn is not None:
            cnn.n_forward = n_fwd
            cnn.step = max(cnn.step - 1, 0)
        self._warm = True

    def _capture(self, first):
        if not getattr(self, "_warm", False):
            self._warmup(first)
        if self.cnn is not None:
            self.cnn.mark_stale()                        # the operand refresh becomes part of the graph: every replay sees fresh weights
        # The body is a generator that yields the gradient range to all-reduce wherever a collective has to sit between kernels (only on
        # the last micro-step of a data-parallel window): every stretch between two yields becomes one hipGraph.
        segs, self._pool = capture_stretches(self._body_gen(first), self._pool, thread_local=self.world > 1)
        return segs

    # ------------------------------------------------------------------ the device side (capturable: lafs_* launches only)
    def _body(self, first):
        """Eager form: the segments back to back, each completed gradient range handed to the reducer as it appears."""
        for out in self._body_gen(first):
            self.reducer.launch(out)
        if self._reduce_now():
            self._reduced = True

    def _body_gen(self, first):
        a, m, B, D, dev = self.arena, self.model, self.B, self.D, self.device
        defer = self._defer_now()
        hp = self.hyper
        if first:                                        # gradient of everything no kernel overwrites <- 0
            call("lafs_zero_chunks", _p(a.grad), _p(a.chunk_seg), _p(a.seg_flags), a.n_chunks, _lib.SEG_OVERWRITTEN)
        if self.mix_rows:
            call("lafs_mix_normalize", _p(self.in_u8), _p(self.x), B, self.S, _p(self.mix_tab))
        else:
            call("lafs_mixup_normalize", _p(self.in_u8), _p(self.x), B, self.S, 1.0, _p(hp[_lib.HP_MIX_LAM:]))
        drop = None
        if m.training and self.drop is not None:         # Residual_droppath: the same rate on both branches of every layer (:106-112)
            call("lafs_droppath_scales", _p(self.keep), m.depth, self.geom.n_seq, self.drop_seed, _p(hp[_lib.HP_STEP:]), _p(self.drop))
            drop = self.drop
        dropout = None
        if m.training and (m.dropout_rate > 0.0 or m.emb_dropout_rate > 0.0):
            dropout = (m.dropout_rate, m.emb_dropout_rate, m._drop_seed0, hp[_lib.HP_STEP:])
        img_in, theta, th = self.x, None, None
        self._cnn_hip = self.with_land and self.cnn is not None
        land = self._land_now = self._teacher_labels() if self.teacher is not None else None
        if land is not None and not self.keep_land:      # mode A: the trunk is fed the teacher's patches; theta carries no gradient
            img_in = self.img_in
            call("lafs_patch_gather_fwd", _p(self.x), _p(land), B, self.S, self.land_n, _p(img_in))
        if self.with_land:
            # trainable landmark regressor -> one-launch patch gather (ViT_face.py:679-711)
            theta = self.cnn.forward(self.x) if self._cnn_hip else m.landmarks(self.x)
            m.theta = theta
            th = self.th = theta.detach().contiguous()   # (kept for read-out: the landmarks the gather used)
            img_in = self.img_in
            call("lafs_patch_gather_fwd", _p(self.x), _p(th), B, self.S, th.shape[1], _p(img_in))
        if self._ws is None:
            # (sized for the deferred form -- one operand slot per layer -- which also holds the immediate form's two)
            probe = Fn.make_trunk_desc(a, m._spec.trunk, self.geom, drop, with_grad=True, wgrad_defer=self.defer,
                                       wgrad_workgroups=self.wgrad_workgroups if self.defer else 0)
            self._ws = Fn.trunk_workspace(probe, True, dev)
        emb, st, _ = Fn.vit_forward(a, m._spec, self.geom, [img_in], [self.pos_rows], drop, save=True, dropout=dropout, ws=self._ws,
                                    x_in=self.x_in, x_out=self.x_out, wgrad_overwrite=first,
                                    wgrad_workgroups=self.wgrad_workgroups if defer else 0,
                                    wgrad_defer=defer, bn_training=m.training)
        self.emb = emb                                   # (kept for read-out)
        if self.head is not None:
            # class-sharded head: all-gather embeddings, local logits, exchanged softmax statistics, reduce-scatter of dE.
            # demb is the gradient of the GLOBAL-batch mean loss, so the later all-reduce of the backbone gradients is a SUM.
            # soft (mixup) targets as the reference's margin head always gets them (train_largescale.py:802): the partner of row b is
            # row B-1-b of this rank's batch (util/mixup_my.py:189-200), its weight 1 - lambda
            lam_h = self._lam
            if self.mix_rows:                            # CutMix / pair / elem modes: the shard kernels' per-row lambda
                lam_h = self.mix_tab.view(f32)[:, _lib.MIX_LAM] if bool((self._mix[0] != 1.0).any()) else 1.0     # (already uploaded)
            soft = torch.is_tensor(lam_h) or lam_h != 1.0    # (more than one rank: PartialFC takes the soft form on every rank, normalize_targets)
            loss, demb = self.head.forward_backward(emb, self._labels, grad_scale=1.0 / self.acc_step,
                                                    labels2=self._labels.flip(0) if soft else None, lam=lam_h)
            self.loss.copy_(loss.detach().view(1))
            yield from self._backward_trunk(st, demb, th, theta)
            return
        # ---- margin head (face_pre_pro/ViT_face.py:49-89 + timm SoftTargetCrossEntropy, train_largescale.py:820)
        call("lafs_l2norm_fwd", _p(emb), D, _p(self.xn), D, _p(self.inv_x), B, D)
        if self.margin_type == 2:                        # AdaFace: this batch's norms -> running statistics (training mode) -> a margin pair per row
            call("lafs_adaface_margins", _p(self.inv_x), B, _p(self.ada_state), self.ada_t_alpha, self.ada_h, self.m, 1 if m.training else 0,
                 _p(self.row_margin))
        call("lafs_weightnorm_fwd", _p(a.view(a.master, self.wname)), _p(self.ones), self.C, self.Cpad, D, _p(self.wn), None, self.Cpad,
             _p(self.inv_w))
        ops.gemm_nt(self.xn, self.wn, _lib.EPI_F32, out=self.cos, n_cols=self.Cpad)
        # margin + softmax + soft-target CE; d/dcos leaves as bf16 (the operand of the two class-gradient GEMMs); the mixup partner of
        # row b is row B-1-b, lambda comes from device memory
        if self.margin_type == 2:                        # one entry for both branches: the batch's lambda at stride 0, or the table's per row
            lam_rows, stride = (self.mix_tab, _lib.MIX_WORDS) if self.mix_rows else (hp[_lib.HP_MIX_LAM:], 0)
            call("lafs_margin_softmax_ce_ada_bf16", _p(self.cos), self.Cpad, B, self.C, _p(self.y1), None, _p(lam_rows), stride,
                 _p(self.row_margin), self.s, 1.0 / self.acc_step, _p(self.dcos), self.Cpad, _p(self.loss), _p(self.row_ws), _p(self.part_ws))
        elif self.mix_rows:                              # a lambda per row (read from the parameter table) and label smoothing
            call("lafs_margin_softmax_ce_mix_bf16", _p(self.cos), self.Cpad, B, self.C, _p(self.y1), None, _p(self.mix_tab), _lib.MIX_WORDS,
                 self.label_smoothing, self.s, self.m, self.margin_type, 1.0 / self.acc_step, _p(self.dcos), self.Cpad, _p(self.loss),
                 _p(self.row_ws), _p(self.part_ws))
        else:
            call("lafs_margin_softmax_ce_bf16", _p(self.cos), self.Cpad, B, self.C, _p(self.y1), None, 1.0, _p(hp[_lib.HP_MIX_LAM:]), self.s,
                 self.m, self.margin_type, 1.0 / self.acc_step, _p(self.dcos), self.Cpad, _p(self.loss), _p(self.row_ws), _p(self.part_ws))
        call("lafs_transpose_bf16", _p(self.dcos), B, self.Cpad, self.Cpad, _p(self.dcos_t), B)
        # d(emb_n) [B, D] = dcos @ Wn: reduction over the classes = the token axis of the wide-tile weight-gradient kernel (slices
        # + fold: no atomics, no zero fill)
        ops.wgrad(self.dcos_t, self.wn, self.dxn, accumulate=False, workspace=self.dxn_ws)
        # d(Wn) and the weight-norm backward of the class table (~0.55 ms of HBM-bound work at C4) gate nothing in the trunk backward:
        # with deferred weight gradients they follow those on the second stream, beside the landmark CNN's backward
        self._head_first = first
        if not (defer and self._cnn_hip and os.environ.get("LAFS_FT_DEFER_HEAD", "1") != "0"):
            self._head_param_grads()
            self._head_first = None
        call("lafs_l2norm_bwd", _p(emb), D, _p(self.dxn), D, _p(self.inv_x), _p(self.demb), D, B, D)
        if self._reduce_now():
            yield a.grad[self.head_off:]                         # margin head (+ anything behind it): final from here on
        yield from self._backward_trunk(st, self.demb, th, theta)

    def _head_param_grads(self):
        """d(Wn) [C, D] = dcos^T @ emb_n (reduction over the batch: an NT GEMM that writes the 633 MB matrix once) and the weight-norm
        backward into the class table's gradient (written on the first micro-step of a window, accumulated after)."""
        a, B, D = self.arena, self.B, self.D
        if self.dwn_ws is None:
            call("lafs_transpose_bf16", _p(self.xn), B, D, D, _p(self.xn_t), B)
            ops.gemm_nt(self.dcos_t, self.xn_t, _lib.EPI_F32, out=self.dwn)
        else:
            ops.wgrad(self.dcos, self.xn, self.dwn, accumulate=False, workspace=self.dwn_ws)
        call("lafs_weightnorm_bwd", _p(self.dwn), _p(a.view(a.master, self.wname)), _p(self.ones), _p(self.inv_w), self.C, D,
             _p(a.view(a.grad, self.wname)), None, 0 if self._head_first else 1)

    def _reduce_now(self):
        """True on the micro-step that completes an accumulation window of a data-parallel run."""
        return self.world > 1 and (self.micro + 1) % self.acc_step == 0

    def _trunk_layers_backward(self, st, demb):
        """Final norm + all blocks; with DP on the window's last micro-step in `grad_slices` runs, each run's gradient range
        handed to RCCL as soon as it has been enqueued (a generator: it yields those ranges)."""
        a, m = self.arena, self.model
        g = Fn.vit_backward_begin(a, m._spec, st, demb, g_buf=self.g_buf)
        self._g = g
        depth = m.depth
        if not self._reduce_now():
            Fn.vit_backward_layers(st, g, depth, 0)
            return
        ns = max(1, min(self.grad_slices, depth))
        cuts = [depth - (depth * k) // ns for k in range(ns + 1)]
        hi = self.head_off
        for k in range(ns):
            Fn.vit_backward_layers(st, g, cuts[k], cuts[k + 1])
            lo = self.block_off[cuts[k + 1]]
            if cuts[k + 1] > 0:                                  # the range below block 0 still waits for the embedding / CNN gradients
                yield a.grad[lo:hi]
                hi = lo
        self._hi_left = hi

    def _backward_trunk(self, st, demb, th, theta):
        a, m, B, D = self.arena, self.model, self.B, self.D
        reduce_now = self._reduce_now()
        yield from self._trunk_layers_backward(st, demb)
        g = self._g
        deferred = bool(st.desc.wgrad_defer)
        cur = torch.cuda.current_stream()
        if deferred and self._cnn_hip:                   # the blocks' weight gradients: beside everything from here to the end of the CNN backward
            self.defer_stream.wait_stream(cur)
            with torch.cuda.stream(self.defer_stream):
                Fn.vit_wgrad_layers(st, m.depth, 0)
                if getattr(self, "_head_first", None) is not None:
                    self._head_param_grads()
                    self._head_first = None
        elif deferred:                                   # (eval-mode model / torch CNN: nothing to hide them behind)
            Fn.vit_wgrad_layers(st, m.depth, 0)
        if self.with_land:
            _, dx = Fn.vit_backward_end(a, m._spec, st, g, want_dx=True, dpos_out=[self.dpos_rows])
            call("lafs_unpatchify_f32", _p(dx[0]), B, self.S, m._spec.patch_order, _p(self.dmosaic))
            if self.dth is None:
                self.dth = torch.empty_like(th)
            call("lafs_patch_gather_bwd", _p(self.x), _p(th), _p(self.dmosaic), B, self.S, th.shape[1], _p(self.dth), None)
            if self.teacher is not None:                 # mode B: + weight / acc_step * MSE(theta, teacher's) into the loss and into dth
                # (class-sharded head: its gradients are those of the GLOBAL-batch mean and are summed over the ranks, so a rank's mean
                # enters with 1 / world)
                gs = 1.0 / self.acc_step / (self.world if self.head is not None else 1)
                call("lafs_landmark_mse", _p(th), _p(self._land_now), B, th.shape[1], _p(self.hyper[_lib.HP_LAND_W:]), gs,
                     _p(self.loss_land), _p(self.loss), _p(self.dth))
            if self._cnn_hip:
                self.cnn.backward(self.dth)              # into the arena's stn.* / output_layer.* gradients
            else:
                theta.backward(self.dth)                 # torch autograd: p.grad are views of the arena
        else:
            Fn.vit_backward_end(a, m._spec, st, g, dpos_out=[self.dpos_rows])
        if deferred and self._cnn_hip:
            cur.wait_stream(self.defer_stream)
        if reduce_now:                                           # what is left: block 0's run + embedding + landmark CNN
            yield a.grad[: self._hi_left]

    # ------------------------------------------------------------------ optimizer
    def optimizer_step(self, lr, weight_decay=0.1, beta1=0.9, beta2=0.999, eps=1e-8):
        """AdamW over every tensor (decay only on >= 2-D tensors, train_largescale.py:122-173); all-reduces the flat gradient
        first when running data-parallel (the reference's DDP does it on every micro-step, :676-677)."""
        a = self.arena
        if self.world > 1:
            if self._reduced:
                self.reducer.wait_all()                          # launched slice by slice during the last backward
            else:
                dist.all_reduce(a.grad)                          # optimizer_step called outside the acc_step cadence
            self._reduced = False
        # dense head: every rank's loss is its local mean -> average; sharded head: gradients of the global mean -> sum
        gscale = 1.0 if self.head is not None else 1.0 / self.world
        self._upload_hyper({_lib.HP_LR: lr, _lib.HP_WD: weight_decay, _lib.HP_BETA1: beta1, _lib.HP_BETA2: beta2, _lib.HP_EPS: eps,
                            _lib.HP_GRAD_SCALE: gscale, _lib.HP_WD_LOW: LOW_WEIGHT_DECAY})
        if self.head is not None:
            self.head.optimizer_step(lr, weight_decay, beta1, beta2, eps)
        call("lafs_clip_adamw_ema", _p(a.master), _p(a.grad), _p(a.exp_avg), _p(a.exp_avg_sq), None, _p(a.shadow), None,
             _p(a.chunk_seg), a.n_chunks, _p(a.seg_flags), _p(a.seg_step), a.n_seg, _p(a.seg_sumsq), _p(self.hyper))
        a.refresh_transposed()
        if self.zero_after_step:
            ops.zero_(a.grad)
        if self.cnn is not None:
            self.cnn.mark_stale()                        # the master weights changed in place: new operand images next forward
        self._since_opt = 0

    def zero_grad(self):
        ops.zero_(self.arena.grad)
        self._since_opt = 0

    def step(self, inputs_u8, labels, lr, weight_decay=0.1, land_weight=None):
        """micro_step + optimizer step every acc_step micro-steps (train_largescale.py:842-891)."""
        loss = self.micro_step(inputs_u8, labels, land_weight=land_weight)
        if self.micro % self.acc_step == 0:
            self.optimizer_step(lr, weight_decay)
        return loss
