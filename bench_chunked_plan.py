#!/usr/bin/env python3
"""The reference's shipped planning step — n_sample 20 000 in chunks of 500 (40 chunks), one look-ahead push, 200 particles — in its two forms,
measured in ONE run on one machine: the chunk loop of plan.py:241-247 (one `mpc.Planner.trajectory_optimization` per chunk, scored by
`running_cost_fused`, then `merge_res`) against `mpc.ChunkedPlanner` (one rollout of all samples, `ag_plan_cost_chunked`, `ag_mppi_update`, one
rollout of the 40 best sequences).  Both sample with the reference's sampler, roll out on the same model (random weights, the engine's default
precision, shared-state rollout) under the task's action limits, and start every repetition from the same torch seed, so they plan the same step.

Per case (granular with the box criterion, rope with the chamfer criterion) it reports
  loop_ms / chunked_ms   wall clock of one planning step (host clock around the call, device synchronised before and after), median over the
                         repetitions after the warm-ups, the two forms alternating inside every repetition
  graph_ms               `ag_plan_cost_chunked` + `ag_mppi_update` on the step's 20 000 samples captured in one HIP graph, per replay (HIP events):
                         the device time of the two new calls without the host's share
  same_act_seq           whether the two forms returned the same action sequence, bit for bit
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time
from functools import partial

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CASES = [("granular", "box"), ("rope", "chamfer")]


def build_case(mat, criterion, dev, n_chunk, n_sample, particles):
    import torch
    from adaptigraph_amd import configs, losses, mpc, synth
    from adaptigraph_amd.forward_dynamics import dynamics
    from adaptigraph_amd.model import DynamicsPredictor
    from adaptigraph_amd.plan_utils import optimize_action_mppi, sample_action_seq
    task = configs.task_config(mat)
    lo, hi = (torch.tensor(task[k], dtype=torch.float32, device=dev) for k in ("action_lower_lim", "action_upper_lim"))
    state, act = synth.make_mpc_inputs(mat, particles, 1, seed=0, len_lo=float(lo[3]), len_hi=float(hi[3]) - 0.1, spacing=0.02)
    centre = (task["action_lower_lim"][0] + task["action_upper_lim"][0]) / 2, (task["action_lower_lim"][1] + task["action_upper_lim"][1]) / 2
    state[:, 0] += np.float32(centre[0] - state[:, 0].mean())      # the object in the middle of the sampled push starts
    state[:, 2] += np.float32(centre[1] - state[:, 2].mean())
    bbox = np.array([[state[:, 0].min() - 5, state[:, 0].max() + 5], [state[:, 2].min() - 5, state[:, 2].max() + 5]])
    state_t = torch.from_numpy(state).to(dev)
    ppm = configs.ppm_optimizer_stub(mat)
    ppm.physics_param = {mat: torch.tensor([0.5], device=dev)}
    model = DynamicsPredictor(configs.model_config(), configs.material_config(mat), configs.dataset_config(mat), dev)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.empty_like(p).uniform_(-1, 1, generator=g) / np.sqrt(p.shape[-1]))
    model = model.to(dev).eval().set_option("precision", 2).set_option("shared_state", 1)
    cost = dict(bbox=bbox, penalty=mat, sim_real_ratio=task["sim_real_ratio"])
    if criterion == "box":
        cx, cz = float(state[:, 0].mean()) + 0.4, float(state[:, 2].mean()) + 0.3
        cost["box_target"] = np.array([[cx - 0.5, cx + 0.5], [cz - 0.5, cz + 0.5]], np.float32)
    else:
        target = torch.from_numpy((state + np.array([0.4, 0.0, 0.3], np.float32)).astype(np.float32)).to(dev)
        cost["error_func"] = partial(losses.chamfer, y=target[None])
    push, weight, noise = task["push_length"], task["reward_weight"], task["noise_level"]
    cfg = dict(action_dim=4, model_rollout_fn=partial(dynamics, model=model, device=dev, ppm_optimizer=ppm), n_sample=n_sample,
               n_look_ahead=task["n_look_ahead"], n_update_iter=1, reward_weight=weight, action_lower_lim=lo, action_upper_lim=hi,
               planner_type="MPPI", device=dev, noise_level=noise, rollout_best=True)
    loop = mpc.Planner(dict(cfg, evaluate_traj_fn=partial(mpc.running_cost_fused, **cost),                   # plan.py:188-209
                            sampling_action_seq_fn=partial(sample_action_seq, action_lower_lim=lo, action_upper_lim=hi, n_sample=n_sample, device=dev,
                                                           noise_level=noise, push_length=push),
                            optimize_action_mppi_fn=partial(optimize_action_mppi, reward_weight=weight, action_lower_lim=lo, action_upper_lim=hi,
                                                            push_length=push)))
    chunked = mpc.ChunkedPlanner(dict(cfg, n_chunk=n_chunk, cost=cost, push_length=push))
    act_seq = torch.from_numpy(act[0]).to(dev)

    def loop_step():
        torch.manual_seed(1234)
        res_all = []
        for ci in range(n_chunk):                                                                           # plan.py:241-247
            loop.chunk_id = ci
            res = loop.trajectory_optimization(state_t, act_seq)
            res_all.append({k: ({kk: vv.detach().clone() for kk, vv in v.items()} if isinstance(v, dict) else
                                v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in res.items()})
        return loop.merge_res(res_all)

    def chunked_step():
        torch.manual_seed(1234)
        return chunked.trajectory_optimization(state_t, act_seq)

    return loop_step, chunked_step, chunked, state_t, cost, task


def graph_of_the_two_calls(chunked, state_t, cost, dev, n_chunk, n_sample):
    """The step's cost and update calls on its 20 000 samples, captured in one HIP graph (the chamfer term computed beforehand and given)."""
    import torch
    from adaptigraph_amd import mpc
    from adaptigraph_amd.plan_utils import optimize_action_mppi_chunks
    torch.manual_seed(1234)
    L = chunked.n_look_ahead
    acts = chunked.sample_chunks(torch.zeros((n_chunk, L, 4), device=dev), iter_index=0).reshape(n_chunk * n_sample, L, 4)
    states = chunked.model_rollout(state_t, acts)["state_seqs"].clone()
    kw = dict(cost)
    if "error_func" in kw:
        kw["error_func"] = lambda s, e=kw["error_func"](states.reshape(-1, states.shape[2], 3)).clone(): e

    def run():
        reward = mpc.running_cost_chunked(states, acts, state_t, n_chunk, **kw)["reward_seqs"]
        return optimize_action_mppi_chunks(acts.reshape(n_chunk, n_sample, L, 4), reward.reshape(n_chunk, n_sample), chunked.reward_weight,
                                           chunked.lim_lo, chunked.lim_hi, chunked.push_length)
    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, eager)), "the replayed calls differ from the eager ones"
    return graph


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7, help="timed planning steps per case and form")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--graph-reps", type=int, default=30)
    ap.add_argument("--chunks", type=int, default=40)
    ap.add_argument("--chunk-samples", type=int, default=500)
    ap.add_argument("--particles", type=int, default=200)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunked_plan_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import _lib
    assert torch.cuda.is_available(), "bench_chunked_plan.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = torch.device(args.device)
    _lib.lib()
    rows = []
    with torch.cuda.device(dev):
        for mat, criterion in CASES:
            loop_step, chunked_step, chunked, state_t, cost, task = build_case(mat, criterion, dev, args.chunks, args.chunk_samples, args.particles)
            forms = {"loop": loop_step, "chunked": chunked_step}
            ms = {k: [] for k in forms}
            last = {}
            for r in range(args.warmup + args.reps):
                for k, fn in forms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[k] = fn()
                    torch.cuda.synchronize()
                    if r >= args.warmup:
                        ms[k].append((time.perf_counter() - t0) * 1e3)
            graph = graph_of_the_two_calls(chunked, state_t, cost, dev, args.chunks, args.chunk_samples)
            g_ms = []
            for r in range(5 + args.graph_reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph.replay()
                e1.record()
                e1.synchronize()
                if r >= 5:
                    g_ms.append(e0.elapsed_time(e1))
            rows.append(dict(material=mat, criterion=criterion, n_chunk=args.chunks, chunk_samples=args.chunk_samples, particles=args.particles,
                             n_look_ahead=task["n_look_ahead"], push_steps=[task["action_lower_lim"][3], task["action_upper_lim"][3]],
                             loop_ms=round(statistics.median(ms["loop"]), 2), chunked_ms=round(statistics.median(ms["chunked"]), 2),
                             loop_min_max_ms=[round(min(ms["loop"]), 2), round(max(ms["loop"]), 2)],
                             chunked_min_max_ms=[round(min(ms["chunked"]), 2), round(max(ms["chunked"]), 2)],
                             graph_ms=round(statistics.median(g_ms), 4),
                             same_act_seq=bool(torch.equal(last["loop"]["act_seq"], last["chunked"]["act_seq"])),
                             same_best_reward=bool(torch.equal(last["loop"]["best_eval_output"]["reward_seqs"],
                                                               last["chunked"]["best_eval_output"]["reward_seqs"]))))
            del loop_step, chunked_step, chunked, graph, last
    line = json.dumps(dict(bench="chunked_plan", device=torch.cuda.get_device_name(dev), reps=args.reps, warmup=args.warmup,
                           timing="median wall clock of one planning step, forms alternating; graph_ms: median HIP-event time of one replay",
                           cases=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
