"""Trajectory cost terms of the planner — drop-in for src/planning/losses.py.

`chamfer` runs the HIP kernel (`ag_chamfer`: no (B,M,N,3) temporaries).  The penalties and `box_loss` here are tensor ops over
(bsz, n_look_forward, n_obj) temporaries: the reference's arithmetic, the autograd path of `GradientPlanner`, and the form that runs on
CPU tensors.  A planner that only scores samples gets the same terms from one device call, `mpc.running_cost_fused` (`ag_plan_cost`).
"""
import torch

from . import _lib
from ._lib import _require_gpu, workspace


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def _y_batched(x, y):
    """1: one target cloud per sample; 0: one cloud for the whole batch (and a batch of one)."""
    return 1 if (y.shape[0] == x.shape[0] and x.shape[0] > 1) else 0


def _chamfer_tiled(x, xm, y, ym, y_batched, idx_x=None, idx_y=None):
    """`ag_chamfer_tiled`: clouds of any size, a sample split over many workgroups; the value (and the indices, when asked for) are the bits
    of the resident entry points wherever those apply.  Its scratch is the grow-only workspace of the current stream."""
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    nbytes = _lib.lib().ag_chamfer_tiled_workspace_bytes(B, N, M)
    ws = workspace(x.device, nbytes)
    _lib.call("ag_chamfer_tiled", x.device, x, xm, y, ym, B, N, M, y_batched, out, idx_x, idx_y, ws, nbytes)
    return out


def _cloud_backward(name, head, x, y, y_batched, grad_out, want_y):
    """The backward call of `_Chamfer` and `_Emd`: entry point `name`, `head` its arguments before grad_out -> gx, gy (None unless wanted).
    A broadcast y (B > 1, one cloud): the kernels write one row per sample and sum them into row 0, which is what comes back."""
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    g = grad_out.contiguous().float()
    gx = torch.empty_like(x)
    gy = torch.empty((B, M, 3), dtype=torch.float32, device=x.device) if want_y else None
    _lib.call(name, x.device, *head, g, B, N, M, y_batched, gx, gy)
    if want_y and y.shape[0] != B:
        gy = gy[:1]
    return gx, gy


class _Chamfer(torch.autograd.Function):
    """chamfer with a backward: `ag_chamfer_fwd_idx` (the same value bits as ag_chamfer / ag_chamfer_masked, plus the nearest-neighbour index
    of every point) and `ag_chamfer_backward` (gather form, no atomics: the gradient is the same bits on every call).  x (B,N,3) and y (B|1,M,3)
    fp32 contiguous on one GPU, xm / ym (B,N) / (B|1,M) u8 or both None.  A broadcast y (B > 1, one cloud) gets the sum of the per-sample
    gradients in ascending sample order.  tiled: `ag_chamfer_tiled` / `ag_chamfer_tiled_backward` instead (no size limit, the same bits)."""

    @staticmethod
    def forward(ctx, x, y, xm, ym, tiled=False):
        B, N, M = x.shape[0], x.shape[1], y.shape[1]
        y_batched = _y_batched(x, y)
        idx_x = torch.empty((B, N), dtype=torch.int32, device=x.device)
        idx_y = torch.empty((B, M), dtype=torch.int32, device=x.device)
        if tiled:
            out = _chamfer_tiled(x, xm, y, ym, y_batched, idx_x, idx_y)
        else:
            out = torch.empty(B, dtype=torch.float32, device=x.device)
            _lib.call("ag_chamfer_fwd_idx", x.device, x, xm, y, ym, B, N, M, y_batched, out, idx_x, idx_y)
        ctx.save_for_backward(x, y, idx_x, idx_y)
        ctx.masks, ctx.y_batched, ctx.tiled = (xm, ym), y_batched, tiled
        ctx.mark_non_differentiable(idx_x, idx_y)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, y, idx_x, idx_y = ctx.saved_tensors
        xm, ym = ctx.masks
        gx, gy = _cloud_backward("ag_chamfer_tiled_backward" if ctx.tiled else "ag_chamfer_backward", (x, xm, y, ym, idx_x, idx_y), x, y,
                                 ctx.y_batched, grad_out, ctx.needs_input_grad[1])
        return gx, gy, None, None, None


def chamfer(x, y, tiled=False):
    """x (B,N,3), y (B or 1,M,3) -> (B,)  mean_m min_n ||x-y|| + mean_n min_m ||x-y||   (losses.py:4-10).
    Differentiable in x and y when grad mode is on and either requires grad (same value bits either way).
    tiled: the form without the N + M <= 12 800 limit of the default (a goal cloud read from a .pcd file, plan.py:139-146), which also spreads
    a call of few samples over the whole device; the same bits as the default wherever that applies.  A cost function opts in with
    `partial(losses.chamfer, y=target, tiled=True)`."""
    _require_gpu(x, "x")
    assert x.dim() == 3 and y.dim() == 3 and x.shape[2] == 3 and y.shape[2] == 3
    assert y.shape[0] in (1, x.shape[0])
    if _needs_grad(x, y):
        return _Chamfer.apply(x.contiguous().float(), y.to(x.device).contiguous().float(), None, None, tiled)
    x = x.contiguous().float()
    y = y.to(x.device).contiguous().float()
    if tiled:
        return _chamfer_tiled(x, None, y, None, _y_batched(x, y))
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _lib.call("ag_chamfer", x.device, x, y, x.shape[0], x.shape[1], y.shape[1], _y_batched(x, y), out)
    return out


def mean_chamfer_device(state_pred, state_real, state_pred_mask, state_real_mask, tiled=False):
    """Per-sample chamfer over the masked-in points of two padded clouds, one launch for the whole batch -> (bsz,) tensor.
    tiled: as for `chamfer`."""
    _require_gpu(state_pred, "state_pred")
    dev = state_pred.device
    x = state_pred.contiguous().float()
    y = state_real.to(dev).contiguous().float()
    xm = state_pred_mask.to(dev).ne(0).to(torch.uint8).contiguous()
    ym = state_real_mask.to(dev).ne(0).to(torch.uint8).contiguous()
    assert x.dim() == 3 and y.dim() == 3 and y.shape[0] == x.shape[0] and xm.shape == x.shape[:2] and ym.shape == y.shape[:2]
    if _needs_grad(state_pred, state_real):      # (sys-id by gradient: differentiable in both clouds, same value bits)
        return _Chamfer.apply(x, y, xm, ym, tiled)
    if tiled:
        return _chamfer_tiled(x, xm, y, ym, 1)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=dev)
    _lib.call("ag_chamfer_masked", dev, x, xm, y, ym, x.shape[0], x.shape[1], y.shape[1], 1, out)
    return out


def mean_chamfer(state_pred, state_real, state_pred_mask, state_real_mask, tiled=False):
    """losses.py:12-24: numpy (bsz,) of chamfer(state_pred[i][mask_i], state_real[i][mask_i]); the reference loops over
    the batch with one `.item()` sync per sample, here it is one kernel and one copy."""
    return mean_chamfer_device(state_pred, state_real, state_pred_mask, state_real_mask, tiled).double().cpu().numpy()


def box_loss(state, target):
    """state (B,N,3), target [[xmin,xmax],[zmin,zmax]] -> (B,) mean distance to the box in the x-z plane (losses.py:26-35)."""
    x, z = state[:, :, 0], state[:, :, 2]
    dx = (target[0, 0] - x).clamp_min(0) + (x - target[0, 1]).clamp_min(0)
    dz = (target[1, 0] - z).clamp_min(0) + (z - target[1, 1]).clamp_min(0)
    return ((dx ** 2 + dz ** 2) ** 0.5).mean(dim=1)


def _states_before_push(state_pred, state_init):
    """x-z particle positions at the START of every look-ahead push: [state_init, state_pred[:, :-1]] (losses.py:42-43)."""
    bsz = state_pred.shape[0]
    first = state_init[:, [0, 2]][None, None].expand(bsz, 1, -1, -1)
    return torch.cat([first, state_pred[:, :-1, :, [0, 2]]], dim=1)


def rope_penalty(state_pred, action, state_init, sim_real_ratio=10.0):
    """exp(-100 max(d - 0.02 r, 0)) with d the pusher-start to nearest-particle distance (losses.py:37-48)."""
    pts = action[:, :, 0:2]                                            # (bsz, L, 2) = (x_start, z_start)
    d = (pts[:, :, None] - _states_before_push(state_pred, state_init)).norm(dim=-1).min(dim=-1).values
    return torch.exp(-(d - 0.02 * sim_real_ratio).clamp_min(0) * 100.0)


def cloth_penalty(state_pred, action, state_init, sim_real_ratio=10.0):
    """Grasp point must touch the cloth (min distance) and prefers far-from-edge picks (max distance) (losses.py:50-64)."""
    pts = action[:, :, 0:2]
    d = (pts[:, :, None] - state_init[:, [0, 2]][None, None]).norm(dim=-1)          # (bsz, L, n)
    dmin = (d.min(dim=-1).values - 0.005 * sim_real_ratio).clamp_min(0)
    dmax = d.max(dim=-1).values.clamp_max(0.4 * sim_real_ratio)
    dmax = dmax / dmax.max()
    return 1.0 - torch.exp(-dmin * 100.0) - dmax * 0.2


def granular_penalty(state_pred, action, state_init, sim_real_ratio=10.0):
    """Nine points along the flat pusher (half-width 0.05 r) must not start inside the pile (losses.py:66-92)."""
    x0, z0, theta = action[:, :, 0], action[:, :, 1], action[:, :, 2]
    rad = 0.05 * sim_real_ratio
    dx, dz = rad * torch.sin(theta), -rad * torch.cos(theta)
    offs = torch.tensor([-1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0], device=action.device)
    pts = torch.stack([x0[..., None] + offs * dx[..., None], z0[..., None] + offs * dz[..., None]], dim=-1)   # (bsz, L, 9, 2)
    s2d = _states_before_push(state_pred, state_init)                                                         # (bsz, L, n, 2)
    d = (pts[:, :, :, None] - s2d[:, :, None]).norm(dim=-1).min(dim=-1).values.min(dim=-1).values
    return torch.exp(-(d - 0.02 * sim_real_ratio).clamp_min(0) * 100.0)


# ---------------------------------------------------------------------------------------------------------------------
# Losses without particle correspondence (src/dynamics/gnn/loss.py): earth-mover and Hausdorff distance
# ---------------------------------------------------------------------------------------------------------------------
def _clouds_and_masks(x, y, x_mask, y_mask, who):
    """The contiguous fp32 clouds and u8 masks a matching kernel reads, and y_batched; shapes checked before anything is launched."""
    _require_gpu(x, "x")
    _require_gpu(y, "y")
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != 3 or y.shape[2] != 3:
        raise ValueError(f"{who}: x (B,N,3) and y (B or 1,M,3) expected, got {tuple(x.shape)} and {tuple(y.shape)}")
    if y.shape[0] not in (1, x.shape[0]):
        raise ValueError(f"{who}: y holds {y.shape[0]} clouds for {x.shape[0]} samples (1 or {x.shape[0]} expected)")
    if (x_mask is None) != (y_mask is None):
        raise ValueError(f"{who}: give both masks or neither")
    x = x.contiguous().float()
    y = y.to(x.device).contiguous().float()
    xm = ym = None
    if x_mask is not None:
        xm, ym = _lib._u8(x_mask.ne(0), x.device), _lib._u8(y_mask.ne(0), x.device)
        if xm.shape != x.shape[:2] or ym.shape != y.shape[:2]:
            raise ValueError(f"{who}: masks {tuple(xm.shape)} / {tuple(ym.shape)} do not match the clouds")
    return x, y, xm, ym, _y_batched(x, y)


def _emd_forward(x, y, xm, ym, y_batched):
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    col = torch.empty((B, N), dtype=torch.int32, device=x.device)
    row = torch.empty((B, M), dtype=torch.int32, device=x.device)
    _lib.call("ag_emd", x.device, x, xm, y, ym, B, N, M, y_batched, out, col, row)
    return out, col, row


class _Emd(torch.autograd.Function):
    """`ag_emd` with `ag_emd_backward`: the assignment is piecewise constant in the coordinates, so the gradient is that of the matched pairs'
    distances (what autograd gives the reference through its gather, loss.py:46-54).  Same value bits as the call without grad."""

    @staticmethod
    def forward(ctx, x, y, xm, ym, y_batched):
        out, col, row = _emd_forward(x, y, xm, ym, y_batched)
        ctx.save_for_backward(x, y, col, row)
        ctx.y_batched = y_batched
        ctx.mark_non_differentiable(col, row)
        return out, col, row

    @staticmethod
    def backward(ctx, grad_out, _gcol, _grow):
        x, y, col, row = ctx.saved_tensors
        gx, gy = _cloud_backward("ag_emd_backward", (x, y, col, row), x, y, ctx.y_batched, grad_out, ctx.needs_input_grad[1])
        return gx, gy, None, None, None


def emd(x, y, x_mask=None, y_mask=None, return_assignment=False):
    """x (B,N,3), y (B or 1,M,3) -> (B,): the mean distance of the pairs of the minimum-cost assignment of the smaller (valid) cloud into the
    larger, EarthMoverLoss.em_distance of dynamics/gnn/loss.py:29-55 per sample, on the device in one launch (`ag_emd`: exact, N, M <=
    AG_EMD_MAX_POINTS).  x_mask (B,N) / y_mask (B or 1,M): points that take part, both or neither.  A sample with an empty side or a non-finite
    valid coordinate is NaN.  Differentiable in x and y; the value bits are the same with and without grad.
    return_assignment: also col (B,N) and row (B,M) int32, the partner of every point or -1."""
    x, y, xm, ym, y_batched = _clouds_and_masks(x, y, x_mask, y_mask, "emd")
    if _needs_grad(x, y):
        out, col, row = _Emd.apply(x, y, xm, ym, y_batched)
    else:
        out, col, row = _emd_forward(x, y, xm, ym, y_batched)
    return (out, col, row) if return_assignment else out


def hausdorff(x, y, x_mask=None, y_mask=None):
    """x (B,N,3), y (B or 1,M,3) -> (values (B,2), arg (B,4) int32): per sample [max_n min_m ||x_n - y_m||, max_m min_n ||x_n - y_m||] over the
    valid points and the indices (n*, its nearest m, m*, its nearest n), ties to the lowest index; NaN / -1 for a sample with an empty side
    (`ag_hausdorff`, N + M <= 12 800).  The values carry no gradient: `gnn_loss.HausdorffLoss` re-evaluates the selected pairs with tensor ops."""
    x, y, xm, ym, y_batched = _clouds_and_masks(x, y, x_mask, y_mask, "hausdorff")
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    out = torch.empty((B, 2), dtype=torch.float32, device=x.device)
    arg = torch.empty((B, 4), dtype=torch.int32, device=x.device)
    _lib.call("ag_hausdorff", x.device, x.detach(), xm, y.detach(), ym, B, N, M, y_batched, out, arg)
    return out, arg
