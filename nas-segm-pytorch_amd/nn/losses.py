"""Criteria of the heads the reference has no training loss for."""
from torch import nn

from .. import functional as F


class BerHuLoss(nn.Module):
    """Reverse-Huber criterion of a depth head: ``F.berhu_loss_masked`` (absent from the reference; Laina et al.
    2016, eq. 2).  forward(pred (B, 1, h, w), target (B, H, W) fp32 at any size, holes where the target is not
    finite or outside ``(valid_min, valid_max]``) -> 0-dim loss.  Handed to ``engine.trainer.train_segmenter`` as
    ``segm_crit`` it selects the depth step."""

    def __init__(self, valid_min=0.0, valid_max=float("inf")):
        super(BerHuLoss, self).__init__()
        self.valid_min = float(valid_min)
        self.valid_max = float(valid_max)

    def forward(self, pred, target):
        return F.berhu_loss_masked(pred, target, self.valid_min, self.valid_max)

    def extra_repr(self):
        return "valid_min={}, valid_max={}".format(self.valid_min, self.valid_max)
