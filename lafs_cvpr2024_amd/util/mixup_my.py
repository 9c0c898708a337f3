"""Mixup / CutMix with the reference's interface (util/mixup_my.py:13-211): batch, pair and elem modes, CutMix boxes from
lambda or from a min/max ratio, switching between the two, label smoothing.  Every np.random call is made in the reference's
order, so under one seed the lambdas, boxes, decisions, mixed images and dense targets are the reference's.
`draw_params` draws one micro-step's parameters without touching an image: the fused fine-tune engine feeds them to
lafs_mix_normalize / lafs_margin_softmax_ce_mix_bf16 and never builds the dense target.  FastCollateMixup (:214-307) is not built."""
import numpy as np
import torch


def one_hot(x, num_classes, on_value=1., off_value=0., device='cuda'):
    x = x.long().view(-1, 1)
    return torch.full((x.size()[0], num_classes), off_value, device=device).scatter_(1, x, on_value)


def mixup_target(target, num_classes, lam=1., smoothing=0.0, device='cuda'):
    """Dense [B, C] soft target lam*onehot(y) + (1-lam)*onehot(flip(y)) (reference :18-24); lam a scalar or a [B, 1] tensor.
    The fused training engine never builds this matrix: it passes (y, flip(y), lam) to the margin-softmax kernels."""
    off = smoothing / num_classes
    on = 1. - smoothing + off
    return one_hot(target, num_classes, on, off, device) * lam + one_hot(target.flip(0), num_classes, on, off, device) * (1. - lam)


def _span_around(centre, extent, limit):
    """[centre - extent // 2, centre + extent // 2) cut off at the image border [0, limit]."""
    reach = extent // 2
    return np.clip(centre - reach, 0, limit), np.clip(centre + reach, 0, limit)


def rand_bbox(img_shape, lam, count=None):
    """CutMix box from lambda (reference :27-47): sides sqrt(1 - lam) of the image's, so that the box covers 1 - lam of it, around a
    centre that is uniform over the image (row first, then column: the order of the two draws is the reference's); what sticks out
    is cut off.  Returns (top, bottom, left, right), scalars or `count`-vectors."""
    height, width = img_shape[-2:]
    side = np.sqrt(1 - lam)
    centre_row = np.random.randint(0, height, size=count)
    centre_col = np.random.randint(0, width, size=count)
    return _span_around(centre_row, int(height * side), height) + _span_around(centre_col, int(width * side), width)


def rand_bbox_minmax(img_shape, minmax, count=None):
    """CutMix box from a (min, max) side ratio (reference :50-68): height and width uniform in [min, max) of the image's, then a
    corner such that the box lies inside.  Draw order: height, width, top, left."""
    low, high = minmax
    height, width = img_shape[-2:]
    box_h, box_w = (np.random.randint(int(n * low), int(n * high), size=count) for n in (height, width))
    top, left = (np.random.randint(0, n - used, size=count) for n, used in ((height, box_h), (width, box_w)))
    return top, top + box_h, left, left + box_w


def cutmix_bbox_and_lam(img_shape, lam, ratio_minmax=None, correct_lam=True, count=None):
    """(box, lambda): lambda becomes the share of the image the box leaves uncovered -- always for min/max boxes, which ignore the
    drawn lambda, and for lambda boxes when `correct_lam` (the border may have cut them; reference :71-81)."""
    from_ratio = ratio_minmax is not None
    box = rand_bbox_minmax(img_shape, ratio_minmax, count=count) if from_ratio else rand_bbox(img_shape, lam, count=count)
    if from_ratio or correct_lam:
        top, bottom, left, right = box
        lam = 1. - (bottom - top) * (right - left) / float(img_shape[-2] * img_shape[-1])
    return box, lam


def _paste(dst, src, box):
    """dst <- src inside box = (top, bottom, left, right), over all leading axes."""
    top, bottom, left, right = box
    dst[..., top:bottom, left:right] = src[..., top:bottom, left:right]


class Mixup:
    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch',
                 correct_lam=True, label_smoothing=0.1, num_classes=1000):
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = mixup_alpha, cutmix_alpha, cutmix_minmax
        if cutmix_minmax is not None:
            assert len(cutmix_minmax) == 2
            self.cutmix_alpha = 1.0                     # (reference :102-105: minmax boxes ignore lambda; alpha only has to be > 0)
        self.mix_prob, self.switch_prob, self.label_smoothing, self.num_classes = prob, switch_prob, label_smoothing, num_classes
        self.mode, self.correct_lam = mode, correct_lam
        self.mixup_enabled = True

    def draw_lambda(self):
        """_params_per_batch (reference :134-150) for mixup only: one uniform for the apply decision, then Beta(alpha, alpha)."""
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            return float(np.random.beta(self.mixup_alpha, self.mixup_alpha))
        return 1.

    # ------------------------------------------------------------------ parameter draws (reference :114-150)
    def _lam_mix(self, size=None):
        """(lam_mix, use_cutmix) of both _params_* functions; size None: scalars."""
        mix, cut = self.mixup_alpha > 0., self.cutmix_alpha > 0.
        assert mix or cut, "One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true."
        if mix and cut:
            if size is None:
                switched = np.random.rand() < self.switch_prob
                a = self.cutmix_alpha if switched else self.mixup_alpha
                return np.random.beta(a, a), switched
            use_cutmix = np.random.rand(size) < self.switch_prob
            lam_cut = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=size)
            return np.where(use_cutmix, lam_cut, np.random.beta(self.mixup_alpha, self.mixup_alpha, size=size)), use_cutmix
        a = self.mixup_alpha if mix else self.cutmix_alpha
        use_cutmix = cut if size is None else np.full(size, cut, dtype=bool)
        return np.random.beta(a, a, size=size), use_cutmix

    def _params_per_elem(self, batch_size):
        """(float32 lambdas, CutMix decisions) for `batch_size` rows: the mode draws for all of them, then one uniform per row
        decides which rows are mixed at all (lambda 1 otherwise)."""
        if not self.mixup_enabled:
            return np.ones(batch_size, dtype=np.float32), np.zeros(batch_size, dtype=bool)
        drawn, decisions = self._lam_mix(batch_size)
        mixed = np.random.rand(batch_size) < self.mix_prob
        return np.where(mixed, drawn.astype(np.float32), np.float32(1.)), decisions

    def _params_per_batch(self):
        """(lambda, CutMix decision) for the whole batch: the apply decision first, and only then the mode's draws."""
        if not (self.mixup_enabled and np.random.rand() < self.mix_prob):
            return 1., False
        drawn, decision = self._lam_mix()
        return float(drawn), decision

    def _box(self, shape, lam):
        return cutmix_bbox_and_lam(shape, lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)

    def _row_plan(self, batch_size, img_shape, pairs):
        """elem (pairs False) and pair (True) modes as a list of decisions: draws the per-row lambdas and CutMix decisions, then, row
        by row in order, the boxes of the mixed CutMix rows (the reference draws them inside its image loop, :161, :178; mixing itself
        consumes no random numbers, so drawing them up front is the same stream).  Returns ([(i, lam, box)] for every mixed leading
        row i -- box None: blend with lam; otherwise paste, lam being the corrected one -- and the final lambda vector, mirrored onto
        the partners in pair mode)."""
        lams, cuts = self._params_per_elem(batch_size // 2 if pairs else batch_size)
        steps = []
        for i, lam in enumerate(lams.copy()):
            if lam == 1.:
                continue
            box = None
            if cuts[i]:
                box, lam = self._box(img_shape, lam)
                lams[i] = lam
            steps.append((i, lam, box))
        return steps, (np.concatenate((lams, lams[::-1])) if pairs else lams)

    def draw_params(self, batch_size, img_shape):
        """One micro-step's mixing parameters, drawn exactly as __call__ draws them on a [batch_size, ..., H, W] batch (same
        np.random calls in the same order) but without an image:
            lam   float32 [B]    the row's lambda AFTER the CutMix box correction (1 = the row passes through)
            cut   bool    [B]    the row pastes its partner's box instead of blending
            box   int32   [B, 4] (top, bottom, left, right), zeros where cut is False
        The partner of row b is row B-1-b in every mode (reference :157, :174, :196).  In batch mode the float64 lambda the dense
        target is built from is kept in `self.last_lam`."""
        B, hw = batch_size, tuple(img_shape[-2:])
        assert B % 2 == 0, 'Batch size should be even when using this'
        lam_out, cut_out, box_out = np.ones(B, dtype=np.float32), np.zeros(B, dtype=bool), np.zeros((B, 4), dtype=np.int32)
        self.last_lam = None
        if self.mode in ('elem', 'pair'):
            pairs = self.mode == 'pair'
            steps, lam_out[:] = self._row_plan(B, hw, pairs)
            for i, _, box in steps:
                if box is not None:
                    rows = [i, B - 1 - i] if pairs else [i]
                    cut_out[rows], box_out[rows] = True, box
            return lam_out, cut_out, box_out
        lam, use_cutmix = self._params_per_batch()
        if lam != 1. and use_cutmix:
            box, lam = self._box(hw, lam)
            cut_out[:], box_out[:] = True, box
        lam_out[:] = lam
        self.last_lam = float(lam)
        return lam_out, cut_out, box_out

    # ------------------------------------------------------------------ mixing on a float batch (reference :152-200)
    def _mix_rows(self, x, pairs):
        """elem and pair modes on images: row i takes from row B-1-i of the UNMIXED batch; in pair mode the partner takes from row i
        with the same lambda and box."""
        B, source = len(x), x.clone()
        steps, lams = self._row_plan(B, tuple(x.shape[-2:]), pairs)
        for i, lam, box in steps:
            for dst, src in ((i, B - 1 - i), (B - 1 - i, i)) if pairs else ((i, B - 1 - i),):
                if box is not None:
                    _paste(x[dst], source[src], box)
                else:
                    x[dst] = source[dst] * lam + source[src] * (1 - lam)
        return torch.tensor(lams, device=x.device, dtype=x.dtype).unsqueeze(1)

    def _mix_elem(self, x):
        return self._mix_rows(x, False)

    def _mix_pair(self, x):
        return self._mix_rows(x, True)

    def _mix_batch(self, x):
        lam, use_cutmix = self._params_per_batch()
        if lam == 1.:
            return 1.
        if use_cutmix:
            box, lam = self._box(x.shape, lam)
            _paste(x, x.flip(0), box)
        else:
            xf = x.flip(0).mul_(1. - lam)
            x.mul_(lam).add_(xf)
        return lam

    def __call__(self, x, target, device='cuda'):
        assert len(x) % 2 == 0, 'Batch size should be even when using this'
        lam = {'elem': self._mix_elem, 'pair': self._mix_pair}.get(self.mode, self._mix_batch)(x)
        return x, mixup_target(target, self.num_classes, lam, self.label_smoothing, device=x.device)
