"""MPPI planning iteration on the engine (BASELINE configs[4]).

`running_cost` is a drop-in for src/planning/plan.py:27-59; `MPPIPlanner.trajectory_optimization_mppi` follows
src/planning/real_world/planner.py:234-277 (sample -> rollout -> evaluate -> softmax update -> keep the best sample),
with the rollout sharded over the ranks of the process group when one is initialised.  Everything stays on the GPU: `running_cost`
and `Planner`'s iteration read nothing back (the reference's `error.max().item()` normaliser is a 0-d tensor here and the best
sample is picked with a device-side `index_select`, not with a 0-d tensor index, which PyTorch resolves through `.item()`).
"""
import ctypes
import functools

import torch

from . import _lib, losses
from .dist import dynamics_sharded, replicate
from .forward_dynamics import dynamics
from .plan_utils import (clip_actions, optimize_action_mppi, optimize_action_mppi_chunks, sample_action_seq,
                         sample_action_seq_chunks)


def running_cost(state, action, state_cur, error_func, penalty_func, bbox, **kwargs):
    """state (bsz, L, n, 3), action (bsz, L, 4), state_cur (n, 3), bbox [[xmin,xmax],[zmin,zmax]] -> {"reward_seqs": (bsz,)}."""
    bsz, L = state.shape[0], state.shape[1]
    error = error_func(state.reshape(bsz * L, state.shape[2], state.shape[3])).reshape(bsz, L)
    error_weight = 2.0 / (error.max() + 1e-6)                # a 0-d tensor: the reference reads it back to the host (plan.py:38), the engine need not
    collision = penalty_func(state, action, state_cur)
    lo, hi = state.min(dim=2).values, state.max(dim=2).values                     # (bsz, L, 3)
    bbox = torch.as_tensor(bbox, dtype=state.dtype, device=state.device)
    margins = torch.stack([lo[..., 0] - bbox[0, 0], bbox[0, 1] - hi[..., 0], lo[..., 2] - bbox[1, 0], bbox[1, 1] - hi[..., 2]], dim=-1)
    box = torch.exp(-margins.clamp_min(0) * 100.0).max(dim=-1).values             # 1 when a particle sits on the workspace edge
    reward = -error_weight * error[:, -1] - 5.0 * collision.mean(dim=1) - 5.0 * box.mean(dim=1)
    return {"reward_seqs": reward}


_PENALTY_FUNCS = {"rope": losses.rope_penalty, "cloth": losses.cloth_penalty, "granular": losses.granular_penalty}


def _no_penalty(state, action, state_cur):
    return torch.zeros(state.shape[:2], dtype=state.dtype, device=state.device)


def running_cost_fused(state, action, state_cur, bbox, penalty, sim_real_ratio=10.0, error_func=None, box_target=None, return_terms=False,
                       **kwargs):
    """`running_cost` as ONE device call (`ag_plan_cost`: two launches that read every predicted cloud once, no (bsz, L, n) temporaries, no host
    read): state (bsz, L, n, 3), action (bsz, L, 4), state_cur (n, 3), bbox [[xmin,xmax],[zmin,zmax]] -> {"reward_seqs": (bsz,)} and, with
    return_terms, "terms" (bsz, L, 9): error, collision, box, nearest, farthest pusher distance, xlo, xhi, zlo, zhi per cloud.

    penalty: "rope", "cloth", "granular" (the `losses.*_penalty` of that name at `sim_real_ratio`) or None (no collision term).
    Exactly one of error_func (a callable on (bsz * L, n, 3) as for `running_cost`, e.g. partial(losses.chamfer, y=target): its result goes
    in as the error term) and box_target ((2, 2): the `losses.box_loss` criterion, computed in the same pass).

    No backward: with grad mode on and `state` or `action` requiring grad, and for CPU tensors, this IS `running_cost` with the tensor-op
    penalty and criterion (the same values as before)."""
    return _fused_cost("running_cost_fused", state, action, state_cur, None, bbox, penalty, sim_real_ratio, error_func, box_target, return_terms)


def _fused_cost(who, state, action, state_cur, n_chunk, bbox, penalty, sim_real_ratio, error_func, box_target, return_terms):
    """`running_cost_fused` (n_chunk None) and `running_cost_chunked`: the checks, the tensor-op route, the device call."""
    if (error_func is None) == (box_target is None):
        raise ValueError(f"{who}: give exactly one of error_func and box_target")
    if penalty not in _lib.AG_PENALTIES:
        raise ValueError(f"{who}: penalty {penalty!r} is not one of 'rope', 'cloth', 'granular', None")
    if not state.is_cuda or (torch.is_grad_enabled() and (state.requires_grad or action.requires_grad)):
        if error_func is None:
            error_func = functools.partial(losses.box_loss, target=torch.as_tensor(box_target, dtype=state.dtype, device=state.device))
        penalty_func = functools.partial(_PENALTY_FUNCS[penalty], sim_real_ratio=sim_real_ratio) if penalty else _no_penalty
        if return_terms:
            raise NotImplementedError(f"{who}: the per-cloud terms come from the device call (no autograd, no CPU tensors)")
        if n_chunk is None:
            return running_cost(state, action, state_cur, error_func, penalty_func, bbox)
        if n_chunk < 1 or state.shape[0] % n_chunk:
            raise ValueError(f"{who}: {state.shape[0]} samples are not {n_chunk} chunks of equal size")
        parts = [running_cost(s, a, state_cur, error_func, penalty_func, bbox)["reward_seqs"]
                 for s, a in zip(state.chunk(n_chunk), action.chunk(n_chunk))]
        return {"reward_seqs": torch.cat(parts)}
    dev = state.device
    bsz, L, n = state.shape[0], state.shape[1], state.shape[2]
    assert state.dim() == 4 and state.shape[3] == 3 and action.shape[:2] == (bsz, L) and action.shape[2] >= (3 if penalty == "granular" else 2)
    state = state.detach().contiguous().float()
    act = action.detach().to(dev).float()
    if act.shape[2] != 4:                        # the kernel reads (x_start, z_start, theta, length) rows
        act = torch.nn.functional.pad(act[:, :, :4], (0, max(0, 4 - act.shape[2])))
    act = act.contiguous()
    init = state_cur.detach().to(dev).contiguous().float()
    assert init.shape == (n, 3)
    error = None
    if error_func is not None:
        error = error_func(state.reshape(bsz * L, n, 3)).detach().reshape(bsz * L).contiguous().float()
    prm = _lib.PlanCostParams(bsz, L, n, _lib.AG_PENALTIES[penalty], _lib.AG_ERROR_GIVEN if box_target is None else _lib.AG_ERROR_BOX,
                              float(sim_real_ratio))
    prm.bbox[:] = [float(v) for v in torch.as_tensor(bbox, dtype=torch.float32).reshape(4).tolist()]
    if box_target is not None:
        prm.box[:] = [float(v) for v in torch.as_tensor(box_target, dtype=torch.float32).reshape(4).tolist()]
    reward = torch.empty(bsz, dtype=torch.float32, device=dev)
    terms = torch.empty((bsz, L, _lib.AG_PLAN_TERMS), dtype=torch.float32, device=dev) if return_terms else None
    nbytes = _lib.lib().ag_plan_cost_workspace_bytes(ctypes.byref(prm))
    ws = _lib.workspace(dev, nbytes)
    if n_chunk is None:
        _lib.call("ag_plan_cost", dev, ctypes.byref(prm), state, act, init, error, reward, terms, ws, nbytes)
    else:
        _lib.call("ag_plan_cost_chunked", dev, ctypes.byref(prm), int(n_chunk), state, act, init, error, reward, terms, ws, nbytes)
    res = {"reward_seqs": reward}
    if return_terms:
        res["terms"] = terms
    return res


def running_cost_chunked(state, action, state_cur, n_chunk, bbox, penalty, sim_real_ratio=10.0, error_func=None, box_target=None,
                         return_terms=False, **kwargs):
    """The cost of ALL chunks of a planning step (plan.py:241-247 scores each chunk in a `running_cost` call of its own) as one device call,
    `ag_plan_cost_chunked`: the arguments of `running_cost_fused` plus n_chunk, state (n_chunk * S, L, n, 3) holding chunk c in rows
    [c S, (c + 1) S).  The error normaliser `2 / (error.max() + 1e-6)` and cloth's largest capped distance are taken over each chunk alone, so
    reward[c S:(c + 1) S] is bit for bit `running_cost_fused` on that slice (n_chunk = the batch size: every sample its own normaliser, the
    reference's call on the one best sequence).  `error_func` sees all clouds at once and must score each cloud on its own, as the chamfer and
    box criteria do.  On CPU tensors and under autograd: the concatenation of `running_cost` over the chunk slices."""
    return _fused_cost("running_cost_chunked", state, action, state_cur, n_chunk, bbox, penalty, sim_real_ratio, error_func, box_target, return_terms)


class Planner:
    """Drop-in for the MPPI branch of the reference's `Planner(config)` (src/planning/real_world/planner.py:38-326): the same
    config keys, `trajectory_optimization(state_cur, act_seq)` result dict and `merge_res`, so plan.py:190-247 can construct it
    unchanged with `model_rollout_fn = partial(adaptigraph_amd.forward_dynamics.dynamics, model=..., ...)`.

    Required keys: action_dim, model_rollout_fn, evaluate_traj_fn, n_sample, n_look_ahead, n_update_iter, reward_weight,
    action_lower_lim, action_upper_lim (tensors of shape (action_dim,)), planner_type ('MPPI'; 'GD' differentiates through the
    rollout, which the inference engine does not provide, and 'MPPI_GD' is unimplemented in the reference too).
    Optional keys (reference defaults): device 'cuda', verbose False, sampling_action_seq_fn, clip_action_seq_fn,
    optimize_action_mppi_fn, noise_type 'normal', noise_level 0.1, n_his 1, rollout_best True.
    The per-iteration progress print of the reference is dropped; nothing here reads a value back to the host."""

    def __init__(self, config):
        self.config = config
        self.action_dim = config["action_dim"]
        self.model_rollout, self.evaluate_traj = config["model_rollout_fn"], config["evaluate_traj_fn"]
        self.n_sample, self.n_look_ahead, self.n_update_iter = config["n_sample"], config["n_look_ahead"], config["n_update_iter"]
        self.reward_weight = config["reward_weight"]
        self.action_lower_lim, self.action_upper_lim = config["action_lower_lim"], config["action_upper_lim"]
        self.planner_type = config["planner_type"]
        assert self.planner_type in ("GD", "MPPI", "MPPI_GD")
        assert isinstance(self.action_lower_lim, torch.Tensor) and isinstance(self.action_upper_lim, torch.Tensor)
        assert self.action_lower_lim.shape == (self.action_dim,) and self.action_upper_lim.shape == (self.action_dim,)
        self.device = config.get("device", "cuda")
        self.verbose = config.get("verbose", False)
        self.sample_action_sequences = config.get("sampling_action_seq_fn", self.sample_action_sequences_default)
        self.clip_action_sequences = config.get("clip_action_seq_fn", self.clip_actions_default)
        self.optimize_action_mppi = config.get("optimize_action_mppi_fn", self.optimize_action_mppi_default)
        self.noise_type = config.get("noise_type", "normal")
        assert self.noise_type == "normal", ("only the 'normal' sampler is provided: the 'fps' grid sampler runs farthest-point sampling on a float64 np.arange grid "
                                             "(~1e10 points at the shipped action limits), whose ties the fp32 kernel ag_fps cannot reproduce")
        self.noise_level = config.get("noise_level", 0.1)
        self.n_his = config.get("n_his", 1)
        self.rollout_best = config.get("rollout_best", True)
        self.chunk_id, self.total_chunks = 0, 1

    def sample_action_sequences_default(self, act_seq, iter_index=0):
        """Low-pass filtered Gaussian perturbations of `act_seq` (planner.py:119-160: beta = 0.7), clipped per step."""
        assert act_seq.shape == (self.n_look_ahead, self.action_dim)
        acts = act_seq[None].repeat(self.n_sample, 1, 1)
        resid = torch.zeros((self.n_sample, self.action_dim), dtype=acts.dtype, device=self.device)
        for i in range(self.n_look_ahead):
            noise = torch.normal(0, self.noise_level, (self.n_sample, self.action_dim), device=self.device)
            resid = 0.7 * noise + resid * (1.0 - 0.7)
            acts[:, i] = torch.clamp(acts[:, i] + resid, self.action_lower_lim, self.action_upper_lim)
        return acts

    def clip_actions_default(self, act_seqs):
        act_seqs.data.clamp_(self.action_lower_lim, self.action_upper_lim)
        return act_seqs

    def optimize_action_mppi_default(self, act_seqs, reward_seqs):
        w = torch.softmax(reward_seqs * self.reward_weight, dim=0)
        return self.clip_action_sequences((act_seqs * w[:, None, None]).sum(dim=0))

    def optimize_action(self, act_seqs, reward_seqs, optimizer=None):
        assert act_seqs.shape == (self.n_sample, self.n_look_ahead, self.action_dim) and reward_seqs.shape == (self.n_sample,)
        if self.planner_type != "MPPI":
            raise NotImplementedError(f"planner_type {self.planner_type}: only the MPPI update is provided")
        return self.optimize_action_mppi(act_seqs, reward_seqs)

    def trajectory_optimization(self, state_cur, act_seq):
        assert isinstance(state_cur, torch.Tensor) and isinstance(act_seq, torch.Tensor)
        assert act_seq.shape == (self.n_look_ahead, self.action_dim)
        if self.planner_type != "MPPI":
            raise NotImplementedError(f"planner_type {self.planner_type}: the engine rolls out without autograd; use 'MPPI'")
        return self.trajectory_optimization_mppi(state_cur, act_seq)

    @torch.no_grad()
    def trajectory_optimization_mppi(self, state_cur, act_seq):
        model_outputs, eval_outputs = [], []
        best_seq = best_reward = None
        for i in range(self.n_update_iter):
            act_seqs = self.sample_action_sequences(act_seq, iter_index=i)
            assert act_seqs.shape == (self.n_sample, self.n_look_ahead, self.action_dim)
            model_out = self.model_rollout(state_cur, act_seqs)
            eval_out = self.evaluate_traj(model_out["state_seqs"], act_seqs, state_cur=state_cur, weights=model_out.get("weights"))
            reward = eval_out["reward_seqs"]
            act_seq = self.optimize_action(act_seqs, reward)
            k = torch.argmax(reward).reshape(1)    # stays on the device: indexing with a 0-d tensor would go through .item() (a host sync)
            seq_k, reward_k = act_seqs.index_select(0, k)[0], reward.index_select(0, k)[0]
            if i == 0:
                best_seq, best_reward = seq_k, reward_k
            else:                                   # keep the better of the two without reading the comparison back
                better = reward_k > best_reward
                best_seq, best_reward = torch.where(better, seq_k, best_seq), torch.where(better, reward_k, best_reward)
            if self.verbose:
                model_outputs.append(model_out)
                eval_outputs.append(eval_out)
        best_model_out = best_eval_out = None
        if self.rollout_best:
            best_model_out = self.model_rollout(state_cur, best_seq[None])
            best_eval_out = self.evaluate_traj(best_model_out["state_seqs"], best_seq[None], state_cur=state_cur)
        return {"act_seq": best_seq, "model_outputs": model_outputs if self.verbose else None,
                "eval_outputs": eval_outputs if self.verbose else None, "best_model_output": best_model_out,
                "best_eval_output": best_eval_out}

    def merge_res(self, res_list):
        """Best chunk by the reward of its best sample (planner.py:312-323); ONE host read for all chunks instead of one each."""
        assert not self.verbose and self.rollout_best
        rewards = torch.stack([r["best_eval_output"]["reward_seqs"].mean() for r in res_list])
        best = res_list[int(torch.argmax(rewards).item())]
        return {"act_seq": best["act_seq"], "model_outputs": None, "eval_outputs": None,
                "best_model_output": best["best_model_output"], "best_eval_output": best["best_eval_output"]}


class ChunkedPlanner(Planner):
    """The chunk loop of plan.py:241-247 — one `Planner.trajectory_optimization` per chunk of n_sample samples, then `merge_res` — as ONE pass
    over all chunks: per iteration one rollout of n_chunk * n_sample samples, one `running_cost_chunked`, one `optimize_action_mppi_chunks`;
    afterwards one rollout of the n_chunk best sequences, scored with chunk size 1 (each its own normaliser, the loop's bsz = 1 call), and a
    device arg-max.  Every chunk keeps its own normalisers, softmax update and best sample, so the results are the loop's; nothing is read back
    to the host beyond what `model_rollout_fn` reads.

    config: `Planner`'s keys (n_sample is the size of ONE chunk, as plan.py:197 sets it) plus
      n_chunk      number of chunks
      cost         dict of `running_cost_chunked`'s keywords: bbox, penalty, and sim_real_ratio, error_func or box_target as needed
      push_length  of the task (plan_utils.py's codec)
    Not read, so that the dict of plan.py:188-208 can be passed as it is: evaluate_traj_fn, optimize_action_mppi_fn, clip_action_seq_fn and the
    per-chunk sampling_action_seq_fn.  The cost and the update are the two device calls with the config's reward_weight and limits; the sampler is
    `plan_utils.sample_action_seq_chunks` with the config's limits and noise_level (see there for the draw order with n_update_iter > 1).

    `trajectory_optimization(state_cur, act_seq, samples=None)`: act_seq (L, 4), every chunk starts from it.  Returns `merge_res`'s dict plus
    "chunks": {"act_seq" (C, L, 4), "reward" (C,): every chunk's best sample and its reward in its sampled batch; "new_seqs": the
    (C, L, 4) MPPI mean of every iteration; "best_reward_seqs" (C,): the rewards of the best sequences rolled out again}.  `samples`, a list
    of one (C * S, L, 4) tensor per iteration, replaces the sampler (tests, replay)."""

    def __init__(self, config):
        cost = dict(config["cost"])
        super().__init__(dict(config, evaluate_traj_fn=functools.partial(running_cost_chunked, **cost)))
        self.n_chunk, self.push_length = int(config["n_chunk"]), float(config["push_length"])
        assert self.planner_type == "MPPI" and self.action_dim == 4 and self.rollout_best and self.n_chunk >= 1
        # the update's limits travel in its parameter block: host copies, made once
        self.lim_lo, self.lim_hi = self.action_lower_lim.detach().cpu(), self.action_upper_lim.detach().cpu()

    def sample_chunks(self, act_seq, iter_index=0):
        return sample_action_seq_chunks(act_seq, self.action_lower_lim, self.action_upper_lim, self.n_sample, self.device,
                                        iter_index=iter_index, noise_level=self.noise_level, push_length=self.push_length)

    @torch.no_grad()
    def trajectory_optimization(self, state_cur, act_seq, samples=None):
        C, S, L = self.n_chunk, self.n_sample, self.n_look_ahead
        assert isinstance(state_cur, torch.Tensor) and isinstance(act_seq, torch.Tensor) and act_seq.shape == (L, 4)
        assert samples is None or len(samples) == self.n_update_iter
        act_seq = act_seq[None].repeat(C, 1, 1)
        model_outputs, eval_outputs, new_seqs = [], [], []
        best_seq = best_reward = None
        for i in range(self.n_update_iter):
            act_seqs = (self.sample_chunks(act_seq, iter_index=i) if samples is None else samples[i]).reshape(C * S, L, 4)
            model_out = self.model_rollout(state_cur, act_seqs)
            eval_out = self.evaluate_traj(model_out["state_seqs"], act_seqs, state_cur=state_cur, n_chunk=C)
            act_seq, _, seq_k, reward_k = optimize_action_mppi_chunks(
                act_seqs.reshape(C, S, L, 4), eval_out["reward_seqs"].reshape(C, S), reward_weight=self.reward_weight,
                action_lower_lim=self.lim_lo, action_upper_lim=self.lim_hi, push_length=self.push_length)
            new_seqs.append(act_seq)
            if i == 0:
                best_seq, best_reward = seq_k, reward_k
            else:                                   # per chunk, the better of the two without reading the comparison back
                better = reward_k > best_reward
                best_seq, best_reward = torch.where(better[:, None, None], seq_k, best_seq), torch.where(better, reward_k, best_reward)
            if self.verbose:
                model_outputs.append(model_out)
                eval_outputs.append(eval_out)
        best_model_out = self.model_rollout(state_cur, best_seq)
        again = self.evaluate_traj(best_model_out["state_seqs"], best_seq, state_cur=state_cur, n_chunk=C)["reward_seqs"]
        k = torch.argmax(again).reshape(1)          # merge_res: the chunk whose best sequence scores highest, picked on the device
        pick = lambda v: v.index_select(0, k) if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == C else v
        return {"act_seq": best_seq.index_select(0, k)[0], "model_outputs": model_outputs if self.verbose else None,
                "eval_outputs": eval_outputs if self.verbose else None,
                "best_model_output": {key: pick(v) for key, v in best_model_out.items()},
                "best_eval_output": {"reward_seqs": again.index_select(0, k)},
                "chunks": {"act_seq": best_seq, "reward": best_reward, "new_seqs": new_seqs, "best_reward_seqs": again}}


class GradientPlanner(Planner):
    """The reference Planner's 'GD' branch (src/planning/real_world/planner.py:212-223, 279-310): Adam on the sampled action sequences
    themselves, `-mean(reward)` differentiated through the rollout and the cost.  The same config keys as `Planner` (planner_type is not
    read) plus `lr` (default 1e-3, planner.py:114); `trajectory_optimization(state_cur, act_seq)` returns the same result dict.

    `model_rollout_fn` must be differentiable in the actions for the model to steer the plan:
    `partial(adaptigraph_amd.forward_dynamics.dynamics_differentiable, model=..., device=..., ppm_optimizer=...)`.  With the no-grad
    `dynamics` only the cost terms that read the actions directly (the penalties) carry a gradient, exactly as in the reference.  A NaN
    gradient raises FloatingPointError (the reference prints and exits)."""

    def __init__(self, config):
        super().__init__(dict(config, planner_type="GD"))
        self.lr = config.get("lr", 1e-3)

    def trajectory_optimization(self, state_cur, act_seq):
        assert isinstance(state_cur, torch.Tensor) and isinstance(act_seq, torch.Tensor)
        assert act_seq.shape == (self.n_look_ahead, self.action_dim)
        with torch.no_grad():
            act_seqs = self.sample_action_sequences(act_seq)
        act_seqs = act_seqs.detach().clone().requires_grad_()
        optimizer = torch.optim.Adam([act_seqs], lr=self.lr, betas=(0.9, 0.999))
        model_outputs, eval_outputs = [], []
        reward = None
        for _ in range(self.n_update_iter):
            assert act_seqs.shape == (self.n_sample, self.n_look_ahead, self.action_dim)
            model_out = self.model_rollout(state_cur, act_seqs)
            eval_out = self.evaluate_traj(model_out["state_seqs"], act_seqs, state_cur=state_cur)
            reward = eval_out["reward_seqs"]
            optimizer.zero_grad()
            (-torch.mean(reward)).backward()
            if act_seqs.grad is not None and bool(torch.isnan(act_seqs.grad).any()):
                raise FloatingPointError("GradientPlanner: NaN in the gradient of the reward w.r.t. the action sequences")
            optimizer.step()
            self.clip_action_sequences(act_seqs)
            if self.verbose:
                model_outputs.append(model_out)
                eval_outputs.append(eval_out)
        best_seq = act_seqs[torch.argmax(reward)]         # the last iteration's rewards, the sequences after its step (planner.py:302)
        best_model_out = best_eval_out = None
        if self.rollout_best:
            best_model_out = self.model_rollout(state_cur, best_seq[None])
            best_eval_out = self.evaluate_traj(best_model_out["state_seqs"], best_seq[None], state_cur=state_cur)
        return {"act_seq": best_seq, "model_outputs": model_outputs if self.verbose else None,
                "eval_outputs": eval_outputs if self.verbose else None, "best_model_output": best_model_out,
                "best_eval_output": best_eval_out}


class MPPIPlanner:
    """Minimal planner with the reference Planner's MPPI branch (planner.py:38-326 keeps many unrelated modes)."""

    def __init__(self, model, device, ppm_optimizer, error_func, penalty_func, bbox, action_lower_lim, action_upper_lim,
                 n_sample, n_look_ahead=1, n_update_iter=1, reward_weight=500.0, noise_level=1.0, rollout_best=True, n_sample_chunk=None,
                 shared_state=True, penalty=None, box_target=None, sim_real_ratio=None):
        task = ppm_optimizer.task_config
        # Every rollout of this planner is ONE cloud under many sampled pushes (planner.py:246): let the engine roll the tool-less base trajectory out
        # once and compute per sample only what can differ from it (ag_set_option "shared_state"; same bits, 8x fewer ms at 1 024 x 15 on rope-1k).
        # None leaves the model's option as it is.
        if shared_state is not None and hasattr(model, "set_option"):
            model.set_option("shared_state", 1 if shared_state else 0)
        self.device = device
        self.lo = torch.as_tensor(action_lower_lim, dtype=torch.float32, device=device)
        self.hi = torch.as_tensor(action_upper_lim, dtype=torch.float32, device=device)
        self.n_sample, self.n_look_ahead, self.n_update_iter = n_sample, n_look_ahead, n_update_iter
        self.reward_weight, self.noise_level, self.push_length = reward_weight, noise_level, task["push_length"]
        self.rollout_best = rollout_best
        self.model = model
        self.n_sample_chunk = n_sample_chunk      # None: all samples in ONE rollout (the engine has no memory reason to chunk).  An int only
                                                   # chunks the ROLLOUT's memory: cost normaliser and softmax update still see all samples at once.
                                                   # The reference's chunked planner (rope.yaml:41-42: 20 000 in chunks of 500) is different: an
                                                   # independent Planner per chunk + merge_res — mpc.ChunkedPlanner has those semantics.
        # copy=False (multi-GPU): a gathered result is a view of the cached receive buffer, valid until the next gather of the same shape —
        # fine for one rollout scored right away, not for chunked rollouts that are concatenated afterwards
        self.model_rollout = lambda state, acts, copy=True: dynamics_sharded(dynamics, state, acts, model, device, ppm_optimizer, copy=copy)
        self.evaluate_traj = functools.partial(running_cost, error_func=error_func, penalty_func=penalty_func, bbox=bbox)
        # Opt-in: score with ONE device call (running_cost_fused) instead of the tensor ops.  penalty ("rope" / "cloth" / "granular") replaces
        # penalty_func, box_target (a (2, 2) box) replaces error_func; sim_real_ratio defaults to the task's.  With neither given nothing changes.
        if penalty is not None or box_target is not None:
            ratio = task.get("sim_real_ratio", 10.0) if sim_real_ratio is None else sim_real_ratio
            self.evaluate_traj = functools.partial(running_cost_fused, bbox=bbox, penalty=penalty, sim_real_ratio=ratio,
                                                   error_func=None if box_target is not None else error_func, box_target=box_target)

    def sample(self, act_seq, iter_index, device=None):
        """Sampled action sequences, REPLICATED across the process group: every rank scores the gathered rollouts of all
        samples against this tensor, so rank 0's draw is broadcast (ranks need not share an RNG state)."""
        dev = self.device if device is None else device
        acts = sample_action_seq(act_seq.to(dev), self.lo.to(dev), self.hi.to(dev), self.n_sample, dev, iter_index=iter_index,
                                 noise_level=self.noise_level, push_length=self.push_length).to(self.device)
        return replicate(acts)

    @torch.no_grad()
    def step(self, state_cur, act_seqs):
        """One MPPI update from GIVEN samples: rollout, rewards, softmax-weighted new sequence.
        The returned `out` may be a VIEW of the cached all-gather buffer (multi-GPU): valid until the next rollout of the same shape — clone what
        has to outlive it."""
        if self.n_sample_chunk and self.n_sample_chunk < act_seqs.shape[0]:
            parts = [self.model_rollout(state_cur, a) for a in act_seqs.split(self.n_sample_chunk)]
            out = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
        else:
            try:
                out = self.model_rollout(state_cur, act_seqs, copy=False)
            except TypeError:      # an externally assigned two-argument model_rollout (the reference's calling convention)
                out = self.model_rollout(state_cur, act_seqs)
        reward = self.evaluate_traj(out["state_seqs"], act_seqs, state_cur=state_cur)["reward_seqs"]
        new_seq = optimize_action_mppi(act_seqs, reward, reward_weight=self.reward_weight, action_lower_lim=self.lo,
                                       action_upper_lim=self.hi, push_length=self.push_length)
        return new_seq, reward, out

    @torch.no_grad()
    def trajectory_optimization_mppi(self, state_cur, act_seq, sample_device=None):
        best_seq, best_reward = None, None
        for i in range(self.n_update_iter):
            act_seqs = self.sample(act_seq, i, sample_device)
            act_seq, reward, _ = self.step(state_cur, act_seqs)
            k = torch.argmax(reward).reshape(1)
            seq_k, reward_k = act_seqs.index_select(0, k)[0], reward.index_select(0, k)[0]
            if best_reward is None:
                best_seq, best_reward = seq_k, reward_k
            else:
                better = reward_k > best_reward
                best_seq, best_reward = torch.where(better, seq_k, best_seq), torch.where(better, reward_k, best_reward)
        res = {"act_seq": best_seq, "best_reward": best_reward}
        if self.rollout_best:
            out = self.model_rollout(state_cur, best_seq[None])
            res["best_model_output"] = out
            res["best_eval_output"] = self.evaluate_traj(out["state_seqs"], best_seq[None], state_cur=state_cur)
        if hasattr(self.model, "take_status"):       # the caller is about to act on the result: surface THIS call's numeric status now
            self.model.take_status(self.device)       # (dynamics() itself only reports the previous call's, to stay sync-free)
        return res
