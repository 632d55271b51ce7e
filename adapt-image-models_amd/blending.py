"""Mini-batch blending of ``train_cfg.blending`` (mmaction/datasets/blending_utils.py:11-152), built through ``BLENDINGS``.

``Recognizer3D`` applies the configured blending to every training batch before ``forward_train``
(recognizers/base.py:104-107,254-255).  Each class splits the reference's ``do_blending`` in two:

* ``draw(imgs_shape)`` draws the random numbers in the reference's order -- Mixup: ``Beta.sample()`` then
  ``torch.randperm``; Cutmix: ``randperm``, ``Beta.sample()``, then the two ``randint`` calls of ``rand_bbox`` -- so a
  seeded run draws exactly what the reference draws.  It returns a ``BlendPlan`` (lam, permutation, box).
* ``apply(imgs, label, plan)`` materialises the blended clips and builds the soft labels with the reference's
  arithmetic.  ``__call__(imgs, label)`` is ``apply(imgs, label, draw(imgs.shape))``.

Unlike the reference's Cutmix, ``apply`` leaves the caller's ``imgs`` intact (it blends into a copy); the values are
the same.  On this package's backbones the recognizer does not call ``apply`` for the clips at all: ``fused(...)`` turns
the plan into a ``FusedBlend`` that the patch gather (``aim_patchify_blend``) applies while it reads the clips.
"""
from typing import NamedTuple, Optional, Tuple

import torch
from torch.distributions.beta import Beta

from .registry import BLENDINGS

__all__ = ["BaseMiniBatchBlending", "MixupBlending", "CutmixBlending", "LabelSmoothing", "BlendPlan", "FusedBlend"]

MIXUP, CUTMIX = 1, 2       # aim_patchify_blend modes


class BlendPlan(NamedTuple):
    """One batch's draws.  ``lam`` is the label weight (for Cutmix the one recomputed from the clamped box,
    blending_utils.py:141-142; ``lam_drawn`` is the Beta sample itself); ``box`` = (x1, y1, x2, y2)."""
    lam: torch.Tensor
    perm: torch.Tensor
    box: Optional[Tuple[int, int, int, int]] = None
    lam_drawn: Optional[torch.Tensor] = None


class FusedBlend(NamedTuple):
    """What the backbone's patch gather needs: per-clip partner index (int32, device), mode, lam, 1 - lam, box."""
    partner: torch.Tensor
    mode: int
    lam: float
    oml: float
    box: Tuple[int, int, int, int]


def one_hot(x, num_classes, on_value=1., off_value=0., device='cuda'):
    """blending_utils.py:11-13."""
    x = x.long().view(-1, 1)
    return torch.full((x.size()[0], num_classes), off_value, device=device).scatter_(1, x, on_value)


def _index_on(perm, device):
    """``perm`` where it is used.  A CUDA tensor indexed by a CPU index copies it up from pageable memory, which waits for
    the stream; from pinned memory the copy is asynchronous."""
    if torch.device(device).type != "cuda":
        return perm
    return perm.pin_memory().to(device, non_blocking=True)


class BaseMiniBatchBlending:
    """Hard labels -> (smoothed) one-hot rows; subclasses blend pairs of clips (blending_utils.py:16-58)."""

    mode = 0

    def __init__(self, num_classes, smoothing=0.):
        self.num_classes = num_classes
        self.off_value = smoothing / self.num_classes
        self.on_value = 1. - smoothing + self.off_value

    def draw(self, imgs_shape) -> Optional[BlendPlan]:
        return None

    def mix_imgs(self, imgs, plan):
        return imgs

    def mix_label(self, one_hot_label, plan):
        return one_hot_label

    def soft_label(self, label, plan):
        """Soft labels [B, num_classes] on ``label``'s device (torch ops; a few KB, not a hot path)."""
        oh = one_hot(label, num_classes=self.num_classes, on_value=self.on_value, off_value=self.off_value, device=label.device)
        return self.mix_label(oh, plan)

    def apply(self, imgs, label, plan):
        return self.mix_imgs(imgs, plan), self.soft_label(label, plan)

    def __call__(self, imgs, label, **kwargs):
        assert self.mode == 0 or len(kwargs) == 0, f'unexpected kwargs for {type(self).__name__} {kwargs}'
        return self.apply(imgs, label, self.draw(imgs.shape))

    def fused(self, plan, segments: int, device) -> Optional[FusedBlend]:
        """The plan as a ``FusedBlend`` for a batch reshaped to ``B * segments`` clips: clip ``b * S + s`` pairs with
        ``perm[b] * S + s``.  The index goes up from pinned memory without blocking the host."""
        if self.mode == 0:
            return None
        S = int(segments)
        idx = (plan.perm.view(-1, 1) * S + torch.arange(S).view(1, -1)).reshape(-1).to(torch.int32)
        partner = _index_on(idx, device)
        lam = plan.lam if self.mode == MIXUP else torch.ones((), dtype=torch.float32)
        return FusedBlend(partner, self.mode, float(lam), float(1 - lam), plan.box or (0, 0, 0, 0))


@BLENDINGS.register_module()
class MixupBlending(BaseMiniBatchBlending):
    """mixup (blending_utils.py:61-93): ``lam * a + (1 - lam) * a[perm]`` for clips and labels alike."""

    mode = MIXUP

    def __init__(self, num_classes, alpha=.2, smoothing=0.):
        super().__init__(num_classes=num_classes, smoothing=smoothing)
        self.beta = Beta(alpha, alpha)

    def draw(self, imgs_shape):
        lam = self.beta.sample()
        rand_index = torch.randperm(imgs_shape[0])
        return BlendPlan(lam, rand_index, None, lam)

    def mix_imgs(self, imgs, plan):
        lam = plan.lam
        return lam * imgs + (1 - lam) * imgs[_index_on(plan.perm, imgs.device), :]

    def mix_label(self, label, plan):
        lam = plan.lam
        return lam * label + (1 - lam) * label[_index_on(plan.perm, label.device), :]


@BLENDINGS.register_module()
class CutmixBlending(BaseMiniBatchBlending):
    """cutmix (blending_utils.py:96-145): the box of clip ``perm[b]`` pasted into clip b on every frame and channel."""

    mode = CUTMIX

    def __init__(self, num_classes, alpha=.2, smoothing=0.):
        super().__init__(num_classes=num_classes, smoothing=smoothing)
        self.beta = Beta(alpha, alpha)

    @staticmethod
    def rand_bbox(img_size, lam):
        """blending_utils.py:110-127, same torch ops (so the same draws and the same truncations)."""
        w = img_size[-1]
        h = img_size[-2]
        cut_rat = torch.sqrt(1. - lam)
        cut_w = torch.tensor(int(w * cut_rat))
        cut_h = torch.tensor(int(h * cut_rat))
        cx = torch.randint(w, (1, ))[0]
        cy = torch.randint(h, (1, ))[0]
        bbx1 = torch.clamp(cx - cut_w // 2, 0, w)
        bby1 = torch.clamp(cy - cut_h // 2, 0, h)
        bbx2 = torch.clamp(cx + cut_w // 2, 0, w)
        bby2 = torch.clamp(cy + cut_h // 2, 0, h)
        return bbx1, bby1, bbx2, bby2

    def draw(self, imgs_shape):
        rand_index = torch.randperm(imgs_shape[0])
        lam_drawn = self.beta.sample()
        bbx1, bby1, bbx2, bby2 = self.rand_bbox(imgs_shape, lam_drawn)
        lam = 1 - (1.0 * (bbx2 - bbx1) * (bby2 - bby1) / (imgs_shape[-1] * imgs_shape[-2]))
        return BlendPlan(lam, rand_index, (int(bbx1), int(bby1), int(bbx2), int(bby2)), lam_drawn)

    def mix_imgs(self, imgs, plan):
        x1, y1, x2, y2 = plan.box
        out = imgs.clone()
        out[:, ..., y1:y2, x1:x2] = imgs[_index_on(plan.perm, imgs.device), ..., y1:y2, x1:x2]
        return out

    def mix_label(self, label, plan):
        lam = plan.lam
        return lam * label + (1 - lam) * label[_index_on(plan.perm, label.device), :]


@BLENDINGS.register_module()
class LabelSmoothing(BaseMiniBatchBlending):
    """Smoothed one-hot labels only (blending_utils.py:148-152): ``on_value = 1 - s + s / C``, ``off_value = s / C``."""
