"""Batched multi-step rollout drivers on the HIP engine — drop-in for src/planning/forward_dynamics.py.

`dynamics(state, action, model, device, ppm_optimizer, physics_param=None)` (:11-205) and
`dynamics_masked(state_init, state_mask, action, model, device, ppm_optimizer, physics_param=None)` (:208-399)
keep the reference signatures and return dicts; `dynamics_differentiable` is `dynamics` under autograd (gradient planning) and
`dynamics_masked_differentiable` is `dynamics_masked` under autograd (sys-id by gradient).  The per-sample set-up (tool key-points from the decoded
action) is a handful of tiny device tensor ops; the inner loop — edges -> GNN forward -> record-on-repeat ->
tool advance -> history shift -> edge rebuild — is one `ag_rollout` call with no host synchronisation
(the reference syncs three times per step: truncate_graph, n_rels.max().item(), pad_torch).
"""
import collections
import ctypes
import os

import torch

from . import _lib
from ._lib import _u8, workspace
from .graph import threshold_sq
from .plan_utils import decode_action


def rollout_order(repeat):
    """The ordering of a ragged rollout for repeat (B,) int32 -> order (B,) int32, active (AG_RAGGED_MAX_STEPS + 1,) int32, on repeat's device
    (ag_rollout_order, include/adaptigraph_hip.h): order = the samples by repeat descending (negatives as 0), ties by ascending index;
    active[s] = #{b : repeat[b] >= s + 1}, the last word = #{b : repeat[b] > AG_RAGGED_MAX_STEPS}.  A GPU tensor takes the library's one launch
    (no host synchronisation); a CPU tensor the same arithmetic in torch, which is what the kernel is tested against."""
    S = _lib.AG_RAGGED_MAX_STEPS
    B = repeat.shape[0]
    if not repeat.is_cuda:
        r = repeat.to(torch.int64).clamp_min(0)
        order = torch.sort(r, descending=True, stable=True).indices.to(torch.int32)
        hist = torch.bincount(r.clamp_max(S + 1), minlength=S + 2)      # keys 0 .. S, and "above"
        active = hist.flip(0).cumsum(0).flip(0)[1:].to(torch.int32)     # active[s] = sum of hist[s + 1:]
        return order, active
    repeat = repeat.to(torch.int32).contiguous()
    order = torch.empty(B, dtype=torch.int32, device=repeat.device)
    active = torch.empty(S + 1, dtype=torch.int32, device=repeat.device)
    _lib.call("ag_rollout_order", repeat.device, repeat, B, order, active)
    return order, active


def rollout(model, state0, delta, attrs, p_instance, phys, mask, tool_mask, thr_sq, repeat, n_steps, topk,
            connect_tools_all, max_tools, height_mode=_lib.AG_HEIGHT_MIN, obj_mask=None, gripper_raise=0.0,
            return_state=False, out=None, order=None, active=None):
    """Native inner loop (forward_dynamics.py:156-197).  All tensors on the model's GPU.
    state0 (B,H,N,3), delta (B,N,3), attrs (B,N,2), p_instance (B,n_p,I), phys (B,P), mask/tool_mask (B,N) bool,
    thr_sq (B,), repeat (B,) int32 -> out_seq (B,n_p,3): prediction of step repeat[b] (zeros if never reached).
    `out`: an already ZEROED contiguous fp32 (B,n_p,3) tensor to write into instead of a fresh one.
    `active`: a HOST int32 tensor of at least n_steps words makes this the ragged rollout (ag_rollout_ragged): the inputs are in the order of
    rollout_order — repeat non-increasing — step s runs the first active[s - 1] samples only, and sample b's result goes to row order[b] (a GPU
    int32 tensor; None: row b) of the outputs; the returned state is then every sample's history after its OWN last step."""
    L = _lib.lib()
    dev = state0.device
    B, H, N, _ = state0.shape
    n_p, n_inst = p_instance.shape[1], p_instance.shape[2]
    prm = _lib.RolloutParams(B, N, n_p, n_inst, int(topk), 1 if connect_tools_all else 0, int(max_tools), int(n_steps),
                             int(height_mode), float(gripper_raise))
    if out is not None:
        assert out.shape == (B, n_p, 3) and out.dtype == torch.float32 and out.is_contiguous() and out.device == dev
    out_seq = out if out is not None else torch.zeros((B, n_p, 3), dtype=torch.float32, device=dev)
    state_final = torch.empty_like(state0, dtype=torch.float32) if return_state else None
    h = model.handle(dev)
    ws = workspace(dev, L.ag_rollout_workspace_bytes_for(h, ctypes.byref(prm)))      # exact for the model's current mode (q16 table: half the largest buffer)
    state0 = state0.contiguous().float()
    delta = delta.contiguous().float()
    attrs = attrs.contiguous().float()
    p_instance = p_instance.contiguous().float()
    phys = phys.to(dev, torch.float32).contiguous()
    mask_u8, tool_u8 = _u8(mask), _u8(tool_mask)
    obj_u8 = _u8(obj_mask) if obj_mask is not None else None
    repeat = repeat.to(dev, torch.int32).contiguous()
    thr_sq = thr_sq.contiguous()
    if active is not None:
        assert not active.is_cuda and active.dtype == torch.int32 and active.is_contiguous() and active.numel() >= int(n_steps)
        assert order is None or (order.device == dev and order.dtype == torch.int32 and order.is_contiguous() and order.numel() == B)
        _lib.call("ag_rollout_ragged", dev, h, ctypes.byref(prm), state0, delta, attrs, p_instance, phys, mask_u8, tool_u8, obj_u8, thr_sq, repeat,
                  ctypes.cast(active.data_ptr(), ctypes.POINTER(ctypes.c_int32)), order, out_seq, state_final, ws, ws.numel())
    else:
        _lib.call("ag_rollout", dev, h, ctypes.byref(prm), state0, delta, attrs, p_instance, phys, mask_u8, tool_u8, obj_u8, thr_sq, repeat,
                  out_seq, state_final, ws, ws.numel())
    return (out_seq, state_final) if return_state else out_seq


def _ragged_plan(rep_cols, device):
    """The device half of a ragged dynamics() call, enqueued BEFORE its one host read: ag_rollout_order per look-ahead column of rep_cols
    (n_look, B) int32, and the per-step counts on their way to pinned memory -> orders (n_look, B) on the GPU, the pinned (n_look,
    AG_RAGGED_MAX_STEPS + 1) counts (valid once the stream has been synchronised)."""
    n_look, bsz = rep_cols.shape
    S1 = _lib.AG_RAGGED_MAX_STEPS + 1
    orders = torch.empty((n_look, bsz), dtype=torch.int32, device=rep_cols.device)
    actives = torch.empty((n_look, S1), dtype=torch.int32, device=rep_cols.device)
    for li in range(n_look):
        _lib.call("ag_rollout_order", rep_cols.device, rep_cols[li], bsz, orders[li], actives[li])
    return orders, _to_pinned(actives, device)


def _ragged_steps(active):
    """Model steps of a column from its pinned counts, or None where a sample runs longer than AG_RAGGED_MAX_STEPS (the plain call's case)."""
    return None if int(active[-1]) != 0 else int(torch.count_nonzero(active[:-1]))


def _push_plan(order, active, rep):
    """What one push of a ragged call runs as -> (n_steps, order, active) for rollout(): the column's own steps, order and pinned counts, or — a
    push longer than the ragged call takes — the plain call on the batch as it is (no order, no counts; one more host read for its step count)."""
    n_steps = _ragged_steps(active)
    if n_steps is None:
        return int(rep.max()), None, None
    return n_steps, order, active


def rollout_scripted(model, state0, action0, tool_pos, tool_delta, attrs, p_instance, phys, mask, tool_mask, thr_sq, topk,
                     connect_tools_all, max_tools, variant="batch", gt=None, obj_mask=None, return_pred=True, return_state=False):
    """A cloud advanced under a RECORDED tool trajectory in one `ag_rollout_scripted` call (the step loop of src/dynamics/rollout/rollout.py:62-93):
    per step t the edges of state[:, -1] (builder `variant`), the forward on the current action, then the tool slots placed at tool_pos[:, t+1]
    and the next action set to tool_delta[:, t+1].  All tensors on the model's GPU; no host synchronisation.
    state0 (B,H,N,3), action0 (B,N,3) the action of step 0, tool_pos / tool_delta (B,T,N-n_p,3) indexed by step (entry 0 is never read; both may
    be None without tool slots, T then comes from gt), attrs (B,N,2), p_instance (B,n_p,I), phys (B,P), mask / tool_mask (B,N) bool, thr_sq (B,)
    rounded as `variant` rounds it (graph.threshold_sq), gt (B,T,n_p,3) ground truth, obj_mask (B,n_p) bool (None: every slot counts).
    -> dict: "pred_seq" (B,T,n_p,3) every step's prediction (return_pred), "err" (B,T) the masked mean distance to gt (gt given),
    "state_final" (B,H,N,3) the history the last step's forward read (return_state)."""
    dev = state0.device
    B, H, N, _ = state0.shape
    n_p, n_inst = p_instance.shape[1], p_instance.shape[2]
    script = tool_pos if tool_pos is not None else gt
    if script is None:
        raise ValueError("rollout_scripted: the number of steps comes from tool_pos or gt; both are None")
    T = script.shape[1]
    for name, t, shape in (("tool_pos", tool_pos, (B, T, N - n_p, 3)), ("tool_delta", tool_delta, (B, T, N - n_p, 3)), ("gt", gt, (B, T, n_p, 3)),
                           ("obj_mask", obj_mask, (B, n_p)), ("action0", action0, (B, N, 3))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"rollout_scripted: {name} is {tuple(t.shape)}, expected {shape}")
    var = _lib.AG_VARIANT_SINGLE if variant == "single" else _lib.AG_VARIANT_BATCH
    prm = _lib.ScriptedParams(B, N, n_p, n_inst, int(topk), 1 if connect_tools_all else 0, int(max_tools), var, T)
    f32 = lambda t: None if t is None else t.to(dev, torch.float32).contiguous()      # noqa: E731
    out = {}
    if return_pred:
        out["pred_seq"] = torch.empty((B, T, n_p, 3), dtype=torch.float32, device=dev)
    if gt is not None:
        out["err"] = torch.empty((B, T), dtype=torch.float32, device=dev)
    if return_state:
        out["state_final"] = torch.empty((B, H, N, 3), dtype=torch.float32, device=dev)
    h = model.handle(dev)
    ws = workspace(dev, _lib.lib().ag_rollout_scripted_workspace_bytes_for(h, ctypes.byref(prm)))
    _lib.call("ag_rollout_scripted", dev, h, ctypes.byref(prm), f32(state0), f32(action0), f32(tool_pos), f32(tool_delta), f32(attrs),
              f32(p_instance), f32(phys), _u8(mask), _u8(tool_mask), f32(thr_sq), f32(gt), None if obj_mask is None else _u8(obj_mask),
              out.get("pred_seq"), out.get("err"), out.get("state_final"), ws, ws.numel())
    return out


def _place_tool(task, decoded, theta, y, device):
    """Tool key-points and per-step delta from a decoded action (forward_dynamics.py:42-81 / :237-276).
    The reference-shaped form, for the two differentiable drivers; the no-grad drivers take _place_tool_lean, the same bits in fewer launches
    (tests/test_host_logic.py, with this form as the reference).  The two must not be merged: this one's backward accumulates the five key-points'
    gradients slice by slice, the lean form's would sum them in one broadcast reduction — another order, other gradient bits."""
    bsz = decoded.shape[0]
    pts = task["pusher_points"]
    ratio = task["sim_real_ratio"]
    n_t = len(pts)
    eef = torch.zeros((bsz, n_t, 3), device=device)
    dlt = torch.zeros((bsz, n_t, 3), device=device)
    dlt[:, :, 0] = (decoded[:, 2] - decoded[:, 0]).unsqueeze(1)
    dlt[:, :, 2] = (decoded[:, 3] - decoded[:, 1]).unsqueeze(1)
    eef[:, :, 1] = y[:, None]
    if n_t == 1:
        eef[:, 0, 0] = decoded[:, 0]
        eef[:, 0, 2] = decoded[:, 1]
    elif n_t == 5:
        eef[:, 0, 0] = decoded[:, 0]
        eef[:, 0, 2] = decoded[:, 1]
        for i in range(1, 5):
            off = float(pts[i][1]) * ratio
            eef[:, i, 0] = decoded[:, 0] + off * torch.sin(theta)
            eef[:, i, 2] = decoded[:, 1] - off * torch.cos(theta)
    else:
        raise NotImplementedError("pusher not implemented")
    raise_by = 0.01 * ratio if task["gripper_enable"] else 0.0
    if raise_by:
        eef[:, :, 1] += raise_by
    return eef, dlt, raise_by


def _place_tool_lean(task, decoded, theta, y, device, zero=None):
    """_place_tool with the same values in fewer launches (dynamics() issues this set-up once per look-ahead step in front of every rollout:
    a dozen 4-us fills and slice assignments are 0.4 % of a 256 x 10 pass and more of an MPPI chunk): the key-point table is assembled by ONE
    stack, the per-step motion by one subtraction + one stack; every element is produced by the same fp32 operation as in _place_tool
    (tests/test_host_logic.py compares the two bit for bit)."""
    pts = task["pusher_points"]
    ratio = task["sim_real_ratio"]
    n_t = len(pts)
    raise_by = 0.01 * ratio if task["gripper_enable"] else 0.0
    d = decoded[:, 2:4] - decoded[:, 0:2]
    dlt = torch.stack([d[:, 0], torch.zeros_like(d[:, 0]) if zero is None else zero, d[:, 1]], dim=-1)[:, None].expand(-1, n_t, -1)      # (`zero`: a cached (bsz,) zero column)
    yy = y + raise_by if raise_by else y
    if n_t == 1:
        eef = torch.stack([decoded[:, 0], yy, decoded[:, 1]], dim=-1)[:, None]
    elif n_t == 5:
        key = ("pusher_off", tuple(float(pts[i][1]) * ratio for i in range(1, 5)), str(device))      # (a host list -> device tensor is a synchronising copy: once per pusher)
        off = _memo(_OFFSETS, key, lambda: torch.tensor([0.0] + list(key[1]), device=device))      # (key-point 0: x + 0 * sin is x + 0)
        sn, cs = torch.sin(theta), torch.cos(theta)
        ex = decoded[:, 0:1] + off[None] * sn[:, None]
        ez = decoded[:, 1:2] - off[None] * cs[:, None]
        ex[:, 0] = decoded[:, 0]         # key-point 0 is the decoded start itself (x + 0 * sin(theta) would turn a -0.0 into +0.0 and an inf * 0 into NaN)
        ez[:, 0] = decoded[:, 1]
        eef = torch.stack([ex, yy[:, None].expand(-1, 5), ez], dim=-1)
    else:
        raise NotImplementedError("pusher not implemented")
    return eef, dlt, raise_by


def _physics(ppm_optimizer, physics_param, bsz, device):
    physics_param = ppm_optimizer.physics_param if physics_param is None else physics_param
    material = ppm_optimizer.material
    dims = ppm_optimizer.material_dims
    assert len(dims) == 1 and material in dims, "Only support single material."
    p = physics_param[material].to(device, torch.float32)
    if p.dim() == 2:      # extension over the reference: one parameter vector PER SAMPLE (batched sys-id sweeps)
        assert p.shape[0] == bsz, f"per-sample physics_param needs {bsz} rows, got {p.shape[0]}"
        return p.contiguous()
    return p[None].repeat(bsz, 1)


_CONST = collections.OrderedDict()      # per (batch, particles, tools, instances, device): the call-invariant inputs of dynamics(), LRU of _CONST_MAX
_CONST_MAX = 4                          # entries (an MPPI loop alternates between its chunk size and the bsz = 1 best-sample rollout: 2 live keys)
_CONST_MAX_BYTES = 256 << 20            # and device bytes (20 000 samples x 200 particles: 66 MB per entry)
_PINNED = {}                            # per (length, dtype, device): pinned staging buffers of _to_pinned
_OFFSETS = {}                           # per (pusher geometry, device): key-point offsets of _place_tool_lean
_LANES = {}                             # per device: the lane indices 0 .. 63 of block_sum


def _memo(cache, key, make):
    """cache[key], made by make() on first use: the small per-device tables above, whose first construction is an allocation or a synchronising copy."""
    value = cache.get(key)
    if value is None:
        value = cache[key] = make()
    return value


def _to_pinned(t, device):
    """t on its way to pinned host memory -> the host tensor of t's shape, valid once the stream has been synchronised (_host_read).  One buffer per
    (length, dtype, device): streams of different devices never share a staging buffer."""
    host = _memo(_PINNED, (t.numel(), t.dtype, str(device)), lambda: torch.empty(t.numel(), dtype=t.dtype, pin_memory=True)).view(t.shape)
    host.copy_(t, non_blocking=True)
    return host


def _host_read(model, device):
    """The ONE host round trip of a no-grad driver call (reference: one per look-ahead + 3 per step; ~75 us each on these boxes): the read of the
    model's deferred numeric status synchronises the stream, which also completes whatever _to_pinned sent in front of it — so everything the
    first push needs is enqueued BEFORE this, and after it only the rollout's own launches stand between the host and a busy GPU."""
    copied = torch.cuda.Event()
    copied.record(torch.cuda.current_stream(torch.device(device)))
    model.take_status(device)
    copied.synchronize()      # normally already complete (take_status synchronises the same stream); never rely on a subclass / stub doing so


def _strict_status(model, device):
    """AG_STRICT_STATUS=1: read the model's numeric status at the END of the call that may have raised it (one more host round trip per call)
    and raise instead of warning; by default the status of call k is seen by call k + 1's read (sync-free), or by an explicit
    model.take_status()."""
    if os.environ.get("AG_STRICT_STATUS", "0") == "1":
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            flags = model.take_status(device)
        if flags:
            raise FloatingPointError(f"adaptigraph_amd: this rollout left the range of its arithmetic (ag_model_status = {flags}): non-finite "
                                     "inputs, or an fp16 activation of the 'fast' edge stack beyond 65504 — use model.set_option('precision', 1)")


def _constants(bsz, n_obj, n_t, max_n, device):
    """attrs / p_instance / mask / tool_mask of forward_dynamics.py:83-123 depend only on the shapes: built once per shape (a dozen tiny
    launches per call otherwise, issued while the GPU idles behind the call's one host sync).  A small LRU bounded by entries AND bytes, so
    varying MPPI chunk sizes (20 000 samples, chunks, the bsz = 1 best-sample rollout) cannot pile up device memory.
    READ-ONLY: the tensors are shared by every later call with the same shapes — callers must not write into them."""
    key = (bsz, n_obj, n_t, max_n, str(device))
    c = _CONST.get(key)
    if c is not None:
        _CONST.move_to_end(key)
        return c
    N = n_obj + n_t
    attrs = torch.zeros((bsz, N, 2), device=device)
    attrs[:, :n_obj, 0] = 1.0
    attrs[:, n_obj:, 1] = 1.0
    p_instance = torch.zeros((bsz, n_obj, max_n), device=device)
    p_instance[:, :, 0] = 1.0
    mask = torch.ones((bsz, N), dtype=torch.bool, device=device)
    tool_mask = torch.zeros((bsz, N), dtype=torch.bool, device=device)
    tool_mask[:, n_obj:] = True
    zeros = torch.zeros((1, n_obj, 3), device=device)        # expanded per call: the object particles' per-step motion (forward_dynamics.py:116-123) and a zero per sample
    c = (attrs, p_instance, mask, tool_mask, zeros)
    nbytes = lambda e: sum(t.numel() * t.element_size() for t in e)      # noqa: E731
    while _CONST and (len(_CONST) >= _CONST_MAX or sum(map(nbytes, _CONST.values())) + nbytes(c) > _CONST_MAX_BYTES):
        _CONST.popitem(last=False)
    _CONST[key] = c
    return c


def _frames(obj, eef, dlt, n_his, obj_still):
    """The inputs of a push's first model step: the cloud obj (B,n_obj,3) and the tool key-points eef (B,n_t,3) in each of the n_his history frames
    -> state0 (B,n_his,N,3); no motion (obj_still, (B,n_obj,3) zeros) for the object rows and dlt (B,n_t,3) per step for the tool's -> delta (B,N,3).
    One cat of expanded views each, for every driver: the differentiable ones record exactly this graph."""
    bsz, n_obj, n_t = obj.shape[0], obj.shape[1], eef.shape[1]
    state0 = torch.cat([obj[:, None].expand(bsz, n_his, n_obj, 3), eef[:, None].expand(bsz, n_his, n_t, 3)], dim=2)
    return state0, torch.cat([obj_still, dlt], dim=1)


def _push_inputs(task, obj, dec, theta, obj_still, order=None, shared=False):
    """state0, delta and the gripper raise of one look-ahead push of dynamics(): the tool placed at the height of the cloud obj (B,n_obj,3) for the
    decoded action rows dec (B,4) and angles theta (B,).
    `shared`: every sample starts from the same cloud — its height is one reduction over n_obj values, not bsz of them (28 -> 5 us at 256 x 1 000).
    `order`: the ragged rollout's — row r of everything per sample is sample order[r].  The action rows, theta and (unless shared: all rows are
    one cloud) the previous frame are gathered HERE, in front of the tool placement: B n_obj 3 floats, where gathering the assembled state0 / delta
    would move B H N 3."""
    bsz = obj.shape[0]
    if order is not None:
        dec, theta = dec.index_select(0, order), theta.index_select(0, order)
        obj = obj if shared else obj.index_select(0, order)
    y = obj[0, :, 1].min().expand(bsz) if shared else obj[:, :, 1].min(dim=1).values
    eef, dlt, raise_by = _place_tool_lean(task, dec, theta, y, obj.device, zero=obj_still[:, 0, 0])
    return _frames(obj, eef, dlt, task["n_his"], obj_still) + (raise_by,)


@torch.no_grad()
def dynamics(state, action, model, device, ppm_optimizer, physics_param=None):
    task = ppm_optimizer.task_config
    state = state.to(device, torch.float32)
    action = action.to(device, torch.float32)
    bsz, n_look = action.shape[0], action.shape[1]
    decoded, repeat = decode_action(action, push_length=task["push_length"])
    n_obj, n_t = state.shape[0], ppm_optimizer.eef_num

    attrs, p_instance, mask, tool_mask, obj_still = _constants(bsz, n_obj, n_t, task["max_n"], device)
    obj_still = obj_still.expand(bsz, n_obj, 3)
    phys = _physics(ppm_optimizer, physics_param, bsz, device)
    src = ppm_optimizer.physics_param if physics_param is None else physics_param
    same_phys = src[ppm_optimizer.material].dim() != 2      # one physics row for all samples: nothing to gather
    thr = threshold_sq(ppm_optimizer.adj_thresh, bsz, torch.device(device), _lib.AG_VARIANT_BATCH)
    rep_cols = repeat.to(torch.int32).t().contiguous()      # (n_look, B): each look-ahead step's column contiguous, made before the sync
    seq = torch.zeros((bsz, n_look, n_obj, 3), device=device)
    first = state[None].expand(bsz, n_obj, 3)
    # model.ragged_rollout only changes a column's plan — (n_steps, order, active) of rollout().  Off: (the column's step maximum, None, None).
    # On: every push is ONE ag_rollout_ragged call that computes a sample for exactly its own number of steps — the samples are ordered on the
    # device (ag_rollout_order), what differs between samples is gathered into that order (attrs, p_instance and the masks are the same for every
    # sample), and the library scatters each result back to its sample's row.  The per-step counts replace the step maximum in the one host read.
    ragged = bool(getattr(model, "ragged_rollout", False))
    if ragged:
        orders, counts = _ragged_plan(rep_cols, device)
    ready = _push_inputs(task, first, decoded[:, 0], action[:, 0, 2], obj_still, orders[0] if ragged else None, shared=True)
    if not ragged:      # the step maxima travel to pinned memory behind the first push's set-up, the last thing in front of the read
        counts = _to_pinned(repeat.max(dim=0).values, device)
    _host_read(model, device)
    max_steps = None if ragged else counts.tolist()
    for li in range(n_look):
        rep = rep_cols[li]
        n_steps, order, active = _push_plan(orders[li], counts[li], rep) if ragged else (max_steps[li], None, None)
        if li > 0 or (ragged and order is None):      # (the first push's inputs stand ready, unless its plan fell back to the plain call's)
            ready = _push_inputs(task, first if li == 0 else seq[:, li - 1], decoded[:, li], action[:, li, 2], obj_still, order, shared=li == 0)
        state0, delta, raise_by = ready
        direct = seq[:, 0] if n_look == 1 else None     # a single look-ahead step: the library writes the result tensor itself
        res = rollout(model, state0, delta, attrs, p_instance, phys if order is None or same_phys else phys.index_select(0, order), mask, tool_mask,
                      thr, rep if order is None else rep.index_select(0, order), n_steps, task["topk"], task["connect_tools_all"], n_t,
                      _lib.AG_HEIGHT_MIN, None, raise_by, out=direct, order=order, active=active)
        if direct is None:
            seq[:, li] = res
    _strict_status(model, device)
    return {"state_seqs": seq, "action_seqs": decoded}


def _frozen_view(model):
    """The parameters of a DynamicsPredictor (or TrainableDynamicsPredictor) DETACHED, in the attribute layout
    TrainableDynamicsPredictor.forward reads: the differentiable rollout optimises actions / physics, never the weights, so no weight
    gradient is ever formed (the chain / linear backward passes skip it when no parameter asks for one)."""
    from types import SimpleNamespace as NS
    lin = lambda m: NS(weight=m.weight.detach(), bias=m.bias.detach())      # noqa: E731
    mlp = lambda blk: NS(model={i: lin(blk.model[i]) for i in (0, 2, 4)})   # noqa: E731
    d = model.non_rigid_predictor
    return NS(nf_effect=model.nf_effect, model_config=model.model_config, motion_clamp=model.motion_clamp, fused_dense=True,
              particle_encoder=mlp(model.particle_encoder), relation_encoder=mlp(model.relation_encoder),
              relation_propagator=NS(linear=lin(model.relation_propagator.linear)), particle_propagator=NS(linear=lin(model.particle_propagator.linear)),
              non_rigid_predictor=NS(linear_0=lin(d.linear_0), linear_1=lin(d.linear_1), linear_2=lin(d.linear_2)))


def block_sum(x):
    """x (B, n) -> (B,): the sum over n in the ORDER of the rollout kernels' workgroup reduction (rollout_step_kernel, ag_step_update): 256
    strided per-thread partials, the xor butterfly 32, 16, .. 1 inside each of the four waves, then (w0 + w1) + (w2 + w3) — as tensor ops, so that
    the masked mean of the tensor-op step update has the kernels' bits.  Differentiable."""
    B, n = x.shape
    k = max(1, -(-n // 256))
    x = torch.nn.functional.pad(x, (0, k * 256 - n)).view(B, k, 256)
    acc = torch.zeros((B, 256), dtype=x.dtype, device=x.device)
    for j in range(k):
        acc = acc + x[:, j]
    v = acc.view(B, 4, 64)
    lanes = _memo(_LANES, str(x.device), lambda: torch.arange(64, device=x.device))
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    w = v[..., 0]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def step_update_ops(pred, states, delta, rec, repeat, ai, height_mode=_lib.AG_HEIGHT_MIN, obj_mask=None, raise_by=0.0):
    """The tail of a model step as tensor ops (forward_dynamics.py:160-176 / :356-372): record where repeat == ai, the tool rows advanced by
    delta at the height of the prediction (min y, or the masked mean of y in the kernels' summation order) plus the raise, the history shifted
    -> (states, rec).  `dynamics_differentiable` runs this form; `step_update` is the same function in one launch each way."""
    bsz, n_obj = pred.shape[0], pred.shape[1]
    n_t = states.shape[2] - n_obj
    rec = torch.where((repeat == ai)[:, None, None], pred, rec)
    tool = states[:, -1, n_obj:] + delta[:, n_obj:]
    if height_mode == _lib.AG_HEIGHT_MIN:
        y = pred[:, :, 1].min(dim=1).values
    else:
        w = obj_mask.to(pred.dtype)
        y = block_sum(pred[:, :, 1] * w) / block_sum(w)
    y_cur = y + raise_by
    tool = torch.stack([tool[..., 0], y_cur[:, None].expand(bsz, n_t), tool[..., 2]], dim=-1)
    states = torch.cat([states[:, 1:], torch.cat([pred, tool], dim=1)[:, None]], dim=1)
    return states, rec


class _StepUpdate(torch.autograd.Function):
    """step_update_ops in one launch (ag_step_update_forward) with its adjoint in one (ag_step_update_backward): the prediction has ONE consumer,
    and the three contributions to its gradient (newest frame, record, tool height) meet in the kernel's fixed order."""

    @staticmethod
    def forward(ctx, pred, states, delta, rec, repeat, ai, height_mode, obj_u8, raise_by):
        _lib._require_gpu(pred, "pred")
        pred, states, delta, rec = (t.contiguous().float() for t in (pred, states, delta, rec))
        B, H, N, _ = states.shape
        n_p = pred.shape[1]
        assert pred.shape == (B, n_p, 3) and delta.shape == (B, N, 3) and rec.shape == pred.shape and repeat.dtype == torch.int32
        states_out, rec_out = torch.empty_like(states), torch.empty_like(pred)
        _lib.call("ag_step_update_forward", pred.device, pred, states, delta, rec, repeat, obj_u8, B, H, N, n_p, int(ai), int(height_mode),
                  float(raise_by), states_out, rec_out)
        ctx.save_for_backward(pred, repeat, obj_u8)
        ctx.meta = (B, H, N, n_p, int(ai), int(height_mode))
        return states_out, rec_out

    @staticmethod
    def backward(ctx, g_states, g_rec):
        pred, repeat, obj_u8 = ctx.saved_tensors
        B, H, N, n_p, ai, mode = ctx.meta
        g_states, g_rec = g_states.contiguous().float(), g_rec.contiguous().float()
        g_pred, g_rec_in = torch.empty_like(pred), torch.empty_like(pred)
        g_in = torch.empty_like(g_states)
        g_delta = torch.empty((B, N, 3), dtype=torch.float32, device=pred.device)
        _lib.call("ag_step_update_backward", pred.device, pred, repeat, obj_u8, B, H, N, n_p, ai, mode, g_states, g_rec, g_pred, g_in, g_delta, g_rec_in)
        return g_pred, g_in, g_delta, g_rec_in, None, None, None, None, None


def step_update(pred, states, delta, rec, repeat, ai, height_mode=_lib.AG_HEIGHT_MIN, obj_mask=None, raise_by=0.0):
    """step_update_ops on the device kernels, under autograd: pred (B,n_p,3), states (B,H,N,3), delta (B,N,3), rec (B,n_p,3), repeat (B,) int32,
    obj_mask (B,n_p) bool for AG_HEIGHT_MASKED_MEAN -> (states, rec)."""
    obj_u8 = _u8(obj_mask, pred.device) if obj_mask is not None else None
    return _StepUpdate.apply(pred, states, delta, rec, repeat, ai, height_mode, obj_u8, raise_by)


def _model_step(view, phys_key, attrs, p_instance, csr, views, repeat, ai, height_mode, obj_mask, raise_by, kernel, states, delta, phys, rec):
    """One model step of the differentiable rollouts: the training forward on the step's edge lists (csr and its EdgeViews), then the state update
    — `kernel`: step_update's one launch each way, else the tensor ops of step_update_ops.
    A function of the four trailing tensors alone: under checkpoint_steps only they are kept, and this runs again in the backward pass."""
    from .train_model import TrainableDynamicsPredictor
    pred, _ = TrainableDynamicsPredictor.forward(view, states, attrs, csr, None, p_instance, action=delta, edge_views=views, **{phys_key: phys})
    return (step_update if kernel else step_update_ops)(pred, states, delta, rec, repeat, ai, height_mode, obj_mask, raise_by)


def _push_differentiable(view, ppm_optimizer, states, delta, attrs, p_instance, mask, tool_mask, phys, repeat, n_steps, checkpoint_steps=False,
                         height_mode=_lib.AG_HEIGHT_MIN, obj_mask=None, raise_by=0.0, device_views=False, kernel=False):
    """One push of the differentiable drivers, n_steps model steps on the detached weights `view` (_frozen_view) from states (B,H,N,3) -> the
    record (B,n_obj,3) of every sample's step repeat[b].
    Per step: the HIP edge builder under no_grad, `train_ops.EdgeViews` over its edges (device_views: both views in one launch), then _model_step.
    checkpoint_steps: the same autograd graph, whose saved activations are dropped and recomputed from the step's four input tensors when the
    backward pass first asks for one; every kernel is deterministic, so gradients keep their bits."""
    from functools import partial
    from torch.utils.checkpoint import checkpoint
    from . import graph, train_ops      # build_edges and EdgeViews are looked up at every call
    task = ppm_optimizer.task_config
    rec = torch.zeros((states.shape[0], p_instance.shape[1], 3), device=states.device)
    for ai in range(1, 1 + n_steps):
        with torch.no_grad():
            csr = graph.build_edges(states[:, -1].detach(), ppm_optimizer.adj_thresh, mask, tool_mask, task["topk"], task["connect_tools_all"],
                                    "batch", max_tools=ppm_optimizer.eef_num)
        step = partial(_model_step, view, ppm_optimizer.material + "_physics_param", attrs, p_instance, csr,
                       train_ops.EdgeViews(csr, device_views=device_views), repeat, ai, height_mode, obj_mask, raise_by, kernel)
        if checkpoint_steps:
            states, rec = checkpoint(step, states, delta, phys, rec, use_reentrant=False, preserve_rng_state=False)
        else:
            states, rec = step(states, delta, phys, rec)
    return rec


def dynamics_differentiable(state, action, model, device, ppm_optimizer, physics_param=None, checkpoint_steps=False):
    """`dynamics` under autograd: the same signature, output dict and semantics (forward_dynamics.py:12-205 without @torch.no_grad,
    including the .detach() of the object state between look-ahead pushes, the tool height from min y, the per-sample action_repeat
    record and gripper_enable), with gradients to `action` (x, z, theta; the push length only counts steps) and to physics_param
    tensors that require grad.  Model weights are used detached.

    Per model step: the HIP radius / top-k edge builder under no_grad, `train_ops.EdgeViews` over its edges, then
    TrainableDynamicsPredictor.forward (HIP gather / segment-sum kernels and fused MFMA chains, forward and backward).
    Cost: one host read per model step (the edge count of EdgeViews) plus one per look-ahead push (its step count), and memory of
    O(steps x saved activations): meant for planning batches of tens to a few hundred samples, not the 20 000 of an MPPI sweep,
    which `dynamics` serves without autograd.

    checkpoint_steps: each model step keeps only its inputs (history frames, tool delta, physics, the step's edge lists) and is recomputed
    in the backward pass: memory O(steps x inputs) + one step's activations, the same outputs and gradients bit for bit.  The state update is
    then ag_step_update's one launch each way instead of the tensor ops (step_update_ops), whose values and gradients it reproduces bit for
    bit (tests/test_sysid_grad.py) — except where two particles share the minimum height exactly: the kernel sends the height's gradient to
    the first of them, torch.min to the one it returned."""
    task = ppm_optimizer.task_config
    state = state.to(device, torch.float32)
    action = action.to(device, torch.float32)
    bsz, n_look = action.shape[0], action.shape[1]
    decoded, repeat = decode_action(action, push_length=task["push_length"])
    n_obj, n_t = state.shape[0], ppm_optimizer.eef_num
    attrs, p_instance, mask, tool_mask, _ = _constants(bsz, n_obj, n_t, task["max_n"], device)
    phys = _physics(ppm_optimizer, physics_param, bsz, device)
    view = _frozen_view(model)
    obj_still = torch.zeros((bsz, n_obj, 3), device=device)
    max_steps = repeat.max(dim=0).values.tolist()
    rep_cols = repeat.t().contiguous()      # (n_look, B) int32: a look-ahead step's column contiguous, as ag_step_update reads it
    seqs = []
    obj = state[None].expand(bsz, n_obj, 3)
    for li in range(n_look):
        if li > 0:
            obj = seqs[li - 1].detach()                                               # forward_dynamics.py:38
        y = obj[:, :, 1].min(dim=1).values
        eef, dlt, raise_by = _place_tool(task, decoded[:, li], action[:, li, 2], y, device)
        states, delta = _frames(obj, eef, dlt, task["n_his"], obj_still)
        seqs.append(_push_differentiable(view, ppm_optimizer, states, delta, attrs, p_instance, mask, tool_mask, phys, rep_cols[li],
                                         int(max_steps[li]), checkpoint_steps, raise_by=raise_by, kernel=bool(checkpoint_steps)))
    return {"state_seqs": torch.stack(seqs, dim=1), "action_seqs": decoded}


def _masked_inputs(state_mask, n_t, max_n):
    """What the masked drivers derive from state_mask (B,n_obj) — bool or 0/1, on its device — for n_t tool slots behind the n_obj object slots and
    max_n instances -> attrs (B,N,2), p_instance (B,n_obj,max_n) in its "first `count` slots" form (forward_dynamics.py:292-300), mask and
    tool_mask (B,N) bool, obj_mask (B,n_obj) bool, cnt (B,) the valid slots per sample.  ONE statement of it: the gradient sys-id is tested
    against the no-grad one, so both must see the same bits."""
    bsz, n_obj = state_mask.shape
    device, N = state_mask.device, n_obj + n_t
    obj_mask = state_mask.bool()
    cnt = state_mask.sum(dim=1)
    attrs = torch.zeros((bsz, N, 2), device=device)
    attrs[:, :n_obj, 0] = state_mask.float()
    attrs[:, n_obj:, 1] = 1.0
    p_instance = torch.zeros((bsz, n_obj, max_n), device=device)
    p_instance[:, :, 0] = (torch.arange(n_obj, device=device)[None] < cnt[:, None]).float()
    mask = torch.ones((bsz, N), dtype=torch.bool, device=device)
    mask[:, :n_obj] = obj_mask
    tool_mask = torch.zeros((bsz, N), dtype=torch.bool, device=device)
    tool_mask[:, n_obj:] = True
    return attrs, p_instance, mask, tool_mask, obj_mask, cnt


def _masked_height(state, state_mask, cnt):
    """The masked mean of y over a sample's valid slots (forward_dynamics.py:235): where the masked drivers put the tool at the start."""
    return (state[:, :, 1] * state_mask).sum(dim=1) / cnt


def dynamics_masked_differentiable(state_init, state_mask, action, model, device, ppm_optimizer, physics_param=None, checkpoint_steps=False):
    """`dynamics_masked` under autograd — the objective of sys-id by gradient: the same signature, output dict and semantics
    (forward_dynamics.py:208-399 without @torch.no_grad: per-sample start clouds with masks, one push, the tool height from the masked mean
    of y at the start and at every step, the per-sample action_repeat record, gripper_enable, a per-sample physics_param of shape (bsz, d)),
    with gradients to physics_param tensors that require grad, to the masked-in rows of state_init and to x, z, theta of `action`.  Model
    weights are used detached.

    Per model step: the HIP edge builder under no_grad, both views of its edge list on the device (EdgeViews(device_views=True): one launch
    of ag_edge_views), TrainableDynamicsPredictor.forward, and the state update in one launch each way (ag_step_update_forward / _backward).
    One host read per model step (the edge count) plus one for the step count.  checkpoint_steps: as in `dynamics_differentiable`."""
    task = ppm_optimizer.task_config
    state_mask = state_mask.to(device)
    n_t = ppm_optimizer.eef_num
    attrs, p_instance, mask, tool_mask, obj_mask, cnt = _masked_inputs(state_mask, n_t, task["max_n"])
    state = state_init.to(device, torch.float32)
    state = torch.where(obj_mask[:, :, None], state, state.detach())      # masked-out rows carry their values along, never a gradient
    action = action.to(device, torch.float32)
    bsz, n_obj = state.shape[0], state.shape[1]
    decoded, repeat = decode_action(action[:, None], push_length=task["push_length"])
    decoded, repeat = decoded[:, 0], repeat[:, 0].contiguous()
    eef, dlt, raise_by = _place_tool(task, decoded, action[:, 2], _masked_height(state, state_mask, cnt), device)
    states, delta = _frames(state, eef, dlt, task["n_his"], torch.zeros((bsz, n_obj, 3), device=device))
    phys = _physics(ppm_optimizer, physics_param, bsz, device)
    rec = _push_differentiable(_frozen_view(model), ppm_optimizer, states, delta, attrs, p_instance, mask, tool_mask, phys, repeat, int(repeat.max().item()),
                               checkpoint_steps, height_mode=_lib.AG_HEIGHT_MASKED_MEAN, obj_mask=obj_mask, raise_by=raise_by, device_views=True,
                               kernel=True)
    return {"state_seqs": rec, "action_seqs": decoded}


@torch.no_grad()
def dynamics_masked(state_init, state_mask, action, model, device, ppm_optimizer, physics_param=None):
    task = ppm_optimizer.task_config
    state = state_init.to(device, torch.float32)
    state_mask = state_mask.to(device)
    action = action.to(device, torch.float32)
    bsz, n_obj = state.shape[0], state.shape[1]
    decoded, repeat = decode_action(action[:, None], push_length=task["push_length"])
    decoded, repeat = decoded[:, 0], repeat[:, 0]
    n_t = ppm_optimizer.eef_num

    attrs, p_instance, mask, tool_mask, obj_mask, cnt = _masked_inputs(state_mask, n_t, task["max_n"])
    obj_still = torch.zeros((bsz, n_obj, 3), device=device)
    eef, dlt, raise_by = _place_tool_lean(task, decoded, action[:, 2], _masked_height(state, state_mask, cnt), device, zero=obj_still[:, 0, 0])
    state0, delta = _frames(state, eef, dlt, task["n_his"], obj_still)
    phys = _physics(ppm_optimizer, physics_param, bsz, device)
    thr = threshold_sq(ppm_optimizer.adj_thresh, bsz, torch.device(device), _lib.AG_VARIANT_BATCH)
    ragged = bool(getattr(model, "ragged_rollout", False))      # the per-step counts instead of the step maximum, in the same one host read
    if ragged:
        orders, counts = _ragged_plan(repeat.to(torch.int32)[None].contiguous(), device)
    else:
        counts = _to_pinned(repeat.max(), device)
    _host_read(model, device)
    n_steps, order, active = _push_plan(orders[0], counts[0], repeat) if ragged else (int(counts.tolist()), None, None)
    if order is not None:      # every per-sample input, built already, in the order of the call; the library scatters the result back
        state0, delta, attrs, p_instance, mask, tool_mask, phys, repeat, obj_mask = (
            t.index_select(0, order) for t in (state0, delta, attrs, p_instance, mask, tool_mask, phys, repeat, obj_mask))
    seq = rollout(model, state0, delta, attrs, p_instance, phys, mask, tool_mask, thr, repeat, n_steps, task["topk"],
                  task["connect_tools_all"], n_t, _lib.AG_HEIGHT_MASKED_MEAN, obj_mask, raise_by, order=order, active=active)
    _strict_status(model, device)
    return {"state_seqs": seq, "action_seqs": decoded}
