"""Action codec and MPPI sampling/update — drop-in for src/planning/plan_utils.py:11-101."""
import ctypes
import math

import torch
import torch.nn.functional as F

from . import _lib


def decode_action(action, push_length=0.10):
    """(…, 4) [x, z, theta, length] -> ((…, 4) [x_s, z_s, x_e, z_e], (…) int32 repeat).

    The push end point is one `push_length` step along -(cos, sin)(theta); `length` is truncated toward zero
    to the number of model steps the push is repeated for (plan_utils.py:15-16)."""
    start = action[..., 0:2]
    theta = action[..., 2]
    repeat = action[..., 3].detach().to(torch.int32)
    direction = torch.stack([torch.cos(theta), torch.sin(theta)], dim=-1)
    end = start - push_length * direction
    return torch.cat([start, end], dim=-1), repeat


def angle_normalize(x):
    return ((x + math.pi) % (2 * math.pi)) - math.pi


def clip_actions(action, action_lower_lim, action_upper_lim):
    """Wrap theta into [-pi, pi) and clamp every field to its limits (plan_utils.py:31-39)."""
    out = action.clone()
    out[..., 2] = angle_normalize(action[..., 2])
    return torch.maximum(torch.minimum(out, action_upper_lim), action_lower_lim)


def _push_ends(act_seqs, push_length):
    xs, zs, th, ln = act_seqs.unbind(-1)
    return xs, zs, xs - ln * push_length * torch.cos(th), zs - ln * push_length * torch.sin(th)


def _from_ends(xs, zs, xe, ze, push_length):
    theta = torch.atan2(zs - ze, xs - xe)
    length = torch.stack([xe - xs, ze - zs], dim=-1).norm(dim=-1) / push_length
    return torch.stack([xs, zs, theta, length], dim=-1)


def sample_action_seq(act_seq, action_lower_lim, action_upper_lim, n_sample, device, iter_index=0, noise_level=0.3,
                      push_length=0.10):
    """(L,4) -> (n_sample, L, 4).  iter 0: uniform in the limits; later: Gaussian noise on both push end points, sigma
    growing 10x per look-ahead index, sample 0 kept as the unperturbed sequence (plan_utils.py:42-77).  Consumes the
    torch RNG exactly as the reference does (one rand / one normal(n_sample,4) per look-ahead step)."""
    L = act_seq.shape[0]
    if iter_index == 0:
        return torch.rand((n_sample, L, act_seq.shape[1]), device=device) * (action_upper_lim - action_lower_lim) + action_lower_lim
    assert act_seq.shape[-1] == 4
    out = act_seq.to(device)[None].repeat(n_sample, 1, 1)
    xs, zs, xe, ze = _push_ends(out, push_length)
    for i in range(L):
        res = 0.1 * (10 ** i) * torch.normal(0, noise_level, (n_sample, 4), device=device)
        cand = _from_ends(xs[:, i] + res[:, 0], zs[:, i] + res[:, 1], xe[:, i] + res[:, 2], ze[:, i] + res[:, 3], push_length)
        out[1:, i] = clip_actions(cand, action_lower_lim, action_upper_lim)[1:]
    return out


def optimize_action_mppi(act_seqs, reward_seqs, reward_weight=100.0, action_lower_lim=None, action_upper_lim=None,
                         push_length=0.10):
    """Softmax(reward * weight)-weighted mean of the push START and END points, re-encoded as (x, z, theta, length)
    and clipped (plan_utils.py:80-101)."""
    assert act_seqs.shape[-1] == 4
    w = F.softmax(reward_seqs * reward_weight, dim=0)[:, None]
    xs, zs, xe, ze = _push_ends(act_seqs, push_length)
    mean = [torch.sum(w * v, dim=0) for v in (xs, zs, xe, ze)]
    return clip_actions(_from_ends(*mean, push_length), action_lower_lim, action_upper_lim)


# ---------------------------------------------------------------------------------------------------------------------
# All chunks of a planning step at once (plan.py:241-247 runs one Planner.trajectory_optimization per chunk)
# ---------------------------------------------------------------------------------------------------------------------
def sample_action_seq_chunks(act_seq, action_lower_lim, action_upper_lim, n_sample, device, iter_index=0, noise_level=0.3, push_length=0.10,
                             noise=None):
    """(C, L, 4) -> (C, n_sample, L, 4): `sample_action_seq` for every chunk's own sequence.

    iter 0: C calls of `sample_action_seq` in chunk order, so under one torch seed the values are those of the per-chunk loop.
    Later: the same formula on all chunks at once with ONE normal draw of (C, n_sample, 4) per look-ahead index (sample 0 of every chunk stays the
    unperturbed sequence).  `noise`, a sequence of L such tensors of UNSCALED draws, replaces the draws (tests, replay).
    Draw ORDER: a loop that runs n_update_iter > 1 iterations per chunk consumes the generator chunk-major (all iterations of chunk 0, then chunk
    1, ...); a chunked step is iteration-major (iteration 0 of all chunks, then iteration 1), so under one seed only iteration 0 of chunk 0 sees
    the loop's numbers.  The distribution is the same."""
    C, L = act_seq.shape[0], act_seq.shape[1]
    if iter_index == 0:
        return torch.stack([sample_action_seq(act_seq[c], action_lower_lim, action_upper_lim, n_sample, device, 0, noise_level, push_length)
                            for c in range(C)])
    assert act_seq.shape[-1] == 4
    out = act_seq.to(device)[:, None].repeat(1, n_sample, 1, 1)
    xs, zs, xe, ze = _push_ends(out, push_length)
    for i in range(L):
        draw = torch.normal(0, noise_level, (C, n_sample, 4), device=device) if noise is None else noise[i].to(device)
        assert draw.shape == (C, n_sample, 4)
        res = 0.1 * (10 ** i) * draw
        cand = _from_ends(xs[:, :, i] + res[..., 0], zs[:, :, i] + res[..., 1], xe[:, :, i] + res[..., 2], ze[:, :, i] + res[..., 3], push_length)
        out[:, 1:, i] = clip_actions(cand, action_lower_lim, action_upper_lim)[:, 1:]
    return out


def optimize_action_mppi_chunks(act_seqs, reward_seqs, reward_weight=100.0, action_lower_lim=None, action_upper_lim=None, push_length=0.10):
    """act_seqs (C, S, L, 4), reward_seqs (C, S) -> new_seq (C, L, 4), best_idx (C) int32, best_seq (C, L, 4), best_reward (C): per chunk
    `optimize_action_mppi` of its S samples, and the sample of its largest reward (the lowest index on ties; a NaN reward is the largest).

    CUDA tensors: ONE device call for all chunks (`ag_mppi_update`, one workgroup per chunk; nothing read back, capturable in a HIP graph).
    CPU tensors: the per-chunk tensor ops below, which state the arithmetic; the device call follows them up to float32 summation order.
    The limits travel in the call's parameter block: pass them as host values (a CUDA tensor is read back here, one host synchronisation)."""
    assert act_seqs.dim() == 4 and act_seqs.shape[-1] == 4 and reward_seqs.shape == act_seqs.shape[:2]
    C, S, L = act_seqs.shape[:3]
    if not act_seqs.is_cuda:
        new_seq = torch.stack([optimize_action_mppi(act_seqs[c], reward_seqs[c], reward_weight, action_lower_lim, action_upper_lim, push_length)
                               for c in range(C)])
        k = torch.argmax(reward_seqs, dim=1)
        pick = torch.arange(C)
        return new_seq, k.to(torch.int32), act_seqs[pick, k], reward_seqs[pick, k]
    dev = act_seqs.device
    acts = act_seqs.detach().contiguous().float()
    reward = reward_seqs.detach().to(dev).contiguous().float()
    prm = _lib.MppiParams(C, S, L, float(reward_weight), float(push_length))
    prm.lo[:] = [float(v) for v in torch.as_tensor(action_lower_lim, dtype=torch.float32).reshape(4).tolist()]
    prm.hi[:] = [float(v) for v in torch.as_tensor(action_upper_lim, dtype=torch.float32).reshape(4).tolist()]
    new_seq, best_seq = torch.empty((2, C, L, 4), dtype=torch.float32, device=dev)
    best_idx = torch.empty(C, dtype=torch.int32, device=dev)
    best_reward = torch.empty(C, dtype=torch.float32, device=dev)
    _lib.call("ag_mppi_update", dev, ctypes.byref(prm), acts, reward, new_seq, best_idx, best_seq, best_reward)
    return new_seq, best_idx, best_seq, best_reward
