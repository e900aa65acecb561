"""Training losses that need no particle correspondence — drop-in for src/dynamics/gnn/loss.py.

`ChamferLoss`, `EarthMoverLoss` and `HausdorffLoss` are called as the reference's: (pred (B,N,D), label (B,M,D)) -> scalar, D = 3.  The distances
run in the HIP kernels of `losses` (`ag_chamfer_*`, `ag_emd`, `ag_hausdorff`): no (B,N,M) tensor, no copy to the host, no scipy.  Each takes an
optional `mask=` ((B,N) bool, or a pair (pred_mask, label_mask)) the reference does not have: padded slots take no part.

`parse_loss_spec` / `build_loss_funcs` turn `train_config["loss_funcs"]` (a list of [name, weight]) into the `loss_funcs` list of
`train_model.unrolled_loss`.
"""
import math

import torch
from torch import nn

from . import losses

LOSS_NAMES = ("mse", "chamfer", "emd", "hausdorff")


def _masks(mask):
    if mask is None:
        return None, None
    if isinstance(mask, (tuple, list)):
        return mask[0], mask[1]
    return mask, mask


class ChamferLoss(nn.Module):
    """loss.py:4-22: mean_n min_m + mean_m min_n of the pair distances, averaged over the batch."""

    def forward(self, pred, label, mask=None):
        if mask is None:
            return losses.chamfer(pred, label).mean()
        xm, ym = _masks(mask)
        return losses.mean_chamfer_device(pred, label, xm, ym).mean()


class EarthMoverLoss(nn.Module):
    """loss.py:25-60: the mean distance of the optimally assigned pairs, averaged over the batch."""

    def forward(self, pred, label, mask=None):
        xm, ym = _masks(mask)
        return losses.emd(pred, label, xm, ym).mean()


class HausdorffLoss(nn.Module):
    """loss.py:63-82: max over the batch of max_n min_m d, plus max over the batch of max_m min_n d.  The kernel finds, per sample, the two
    directed maxima and their point pairs; the sample of the largest maximum is picked per direction and its pair's distance re-evaluated
    with tensor ops, which is what carries the gradient (to the two points of each selected pair, as autograd through max and min does)."""

    def forward(self, pred, label, mask=None):
        xm, ym = _masks(mask)
        val, arg = losses.hausdorff(pred, label, xm, ym)
        total = None
        for d in (0, 1):
            v = val[:, d]
            b = torch.argmax(torch.where(torch.isnan(v), torch.full_like(v, -1.0), v))      # (a sample with an empty side never wins)
            n, m = (arg[b, 0], arg[b, 1]) if d == 0 else (arg[b, 3], arg[b, 2])
            n, m = n.long().clamp_min(0), m.long().clamp_min(0)
            lb = b if label.shape[0] == pred.shape[0] else torch.zeros_like(b)
            diff = pred[b].index_select(0, n[None])[0].float() - label[lb].index_select(0, m[None])[0].float()
            dist = ((diff[0] * diff[0] + diff[1] * diff[1]) + diff[2] * diff[2]).sqrt() + v[b] * 0      # (NaN when no sample has two valid sides)
            total = dist if total is None else total + dist
        return total


def parse_loss_spec(spec):
    """[[name, weight], ...] -> [(name, float(weight)), ...]; ValueError for an unknown name, a malformed entry or a weight that is not a
    finite number.  Touches no GPU."""
    if not isinstance(spec, (list, tuple)) or len(spec) == 0:
        raise ValueError(f"loss_funcs: a non-empty list of [name, weight] pairs expected, got {spec!r}")
    out = []
    for entry in spec:
        if not isinstance(entry, (list, tuple)) or len(entry) != 2:
            raise ValueError(f"loss_funcs: [name, weight] expected, got {entry!r}")
        name, weight = entry
        if name not in LOSS_NAMES:
            raise ValueError(f"loss_funcs: unknown loss {name!r} (known: {', '.join(LOSS_NAMES)})")
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not math.isfinite(weight):
            raise ValueError(f"loss_funcs: the weight of {name!r} must be a finite number, got {weight!r}")
        out.append((name, float(weight)))
    return out


def build_loss_funcs(parsed, obj_mask=None):
    """The (function, weight) list `train_model.unrolled_loss` takes, for one batch: `mse` is its own mse_loss; the others get `obj_mask`
    ((B, n_obj), non-zero = a real particle) as the mask of both clouds, so padding never takes part in a matching."""
    modules = {"chamfer": ChamferLoss(), "emd": EarthMoverLoss(), "hausdorff": HausdorffLoss()}
    funcs = []
    for name, weight in parsed:
        if name == "mse":
            funcs.append((torch.nn.functional.mse_loss, weight))
        else:
            funcs.append((lambda pred, label, _m=modules[name]: _m(pred, label, mask=None if obj_mask is None else obj_mask[:, :pred.shape[1]]),
                          weight))
    return funcs
