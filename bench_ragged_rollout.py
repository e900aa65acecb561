#!/usr/bin/env python3
"""Ragged rollouts measured: `dynamics()` and a `ChunkedPlanner` step with `DynamicsPredictor.ragged_rollout` off and on, in ONE run on one
machine, the two forms alternating inside every repetition.  With the attribute on a sample is rolled out for exactly its own number of model
steps (`ag_rollout_order` + `ag_rollout_ragged`) instead of the batch's maximum; the results are the same bits, which every case checks.

Cases: `dynamics()` on 1 024 sampled pushes of a 1 000-particle rope, and on 20 000 pushes of a 200-particle cloud under the granular and the rope
push-length limits, each with the shared-state rollout off and on; and the planning step of bench_chunked_plan.py (40 chunks of 500 samples).
Per case:
  plain_ms / ragged_ms     wall clock of one call (host clock, device synchronised before and after), median over the repetitions after the warm-ups
  *_min_max_ms             the run's own spread
  executed_fraction        sum(repeat) / (B max(repeat)): the share of the plain call's sample-steps the ragged call executes
  same_bits                whether both forms returned the same tensors, bit for bit
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DYNAMICS_CASES = [("rope", 1024, 1000), ("granular", 20000, 200), ("rope", 20000, 200)]      # material (its push-length limits), samples, particles


def random_model(mat, dev, shared_state):
    import torch
    from adaptigraph_amd import configs
    from adaptigraph_amd.model import DynamicsPredictor
    model = DynamicsPredictor(configs.model_config(), configs.material_config(mat), configs.dataset_config(mat), dev)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.empty_like(p).uniform_(-1, 1, generator=g) / np.sqrt(p.shape[-1]))
    return model.to(dev).eval().set_option("precision", 2).set_option("shared_state", shared_state)


def executed_fraction(action, push_length):
    from adaptigraph_amd.plan_utils import decode_action
    rep = decode_action(action, push_length=push_length)[1].clamp_min(0).long()      # (B, n_look)
    return float(rep.sum()) / float((rep.max(dim=0).values * rep.shape[0]).sum())


def alternate(forms, reps, warmup):
    """forms: name -> callable; every repetition runs each once -> (ms lists, last results)"""
    import torch
    ms, last = {k: [] for k in forms}, {}
    for r in range(warmup + reps):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = fn()
            torch.cuda.synchronize()
            if r >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms, last


def timing_fields(ms):
    out = {}
    for k, v in ms.items():
        out[f"{k}_ms"] = round(statistics.median(v), 3)
        out[f"{k}_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
    out["ragged_over_plain"] = round(out["ragged_ms"] / out["plain_ms"], 4)
    return out


def dynamics_case(mat, bsz, particles, shared_state, dev, reps, warmup):
    import torch
    from adaptigraph_amd import configs, synth
    from adaptigraph_amd.forward_dynamics import dynamics
    task = configs.task_config(mat)
    lo, hi = task["action_lower_lim"][3], task["action_upper_lim"][3]
    state, act = synth.make_mpc_inputs(mat, particles, bsz, seed=0, len_lo=float(lo), len_hi=float(hi) - 1e-3, spacing=0.02 if particles < 500 else 0.1)
    state_t, act_t = torch.from_numpy(state).to(dev), torch.from_numpy(act).to(dev)
    ppm = configs.ppm_optimizer_stub(mat)
    ppm.physics_param = {mat: torch.tensor([0.5], device=dev)}
    model = random_model(mat, dev, shared_state)

    def form(on):
        def run():
            model.ragged_rollout = on
            return dynamics(state_t, act_t, model, dev, ppm)["state_seqs"]
        return run
    ms, last = alternate({"plain": form(False), "ragged": form(True)}, reps, warmup)
    return dict(call="dynamics", material=mat, samples=bsz, particles=particles, shared_state=shared_state, push_steps=[lo, hi],
                executed_fraction=round(executed_fraction(act_t, task["push_length"]), 4), same_bits=bool(torch.equal(last["plain"], last["ragged"])),
                **timing_fields(ms))


def planner_case(mat, criterion, dev, n_chunk, n_sample, particles, reps, warmup):
    import torch
    from bench_chunked_plan import build_case
    _, chunked_step, chunked, _, _, task = build_case(mat, criterion, dev, n_chunk, n_sample, particles)
    model = chunked.model_rollout.keywords["model"]

    def form(on):
        def run():
            model.ragged_rollout = on
            return chunked_step()
        return run
    ms, last = alternate({"plain": form(False), "ragged": form(True)}, reps, warmup)
    torch.manual_seed(1234)
    L = chunked.n_look_ahead
    acts = chunked.sample_chunks(torch.zeros((n_chunk, L, 4), device=dev), iter_index=0).reshape(n_chunk * n_sample, L, 4)
    a, b = last["plain"], last["ragged"]
    same = (torch.equal(a["act_seq"], b["act_seq"]) and torch.equal(a["best_model_output"]["state_seqs"], b["best_model_output"]["state_seqs"])
            and torch.equal(a["best_eval_output"]["reward_seqs"], b["best_eval_output"]["reward_seqs"]))
    return dict(call="ChunkedPlanner", material=mat, criterion=criterion, n_chunk=n_chunk, chunk_samples=n_sample, particles=particles, shared_state=1,
                push_steps=[task["action_lower_lim"][3], task["action_upper_lim"][3]],
                executed_fraction=round(executed_fraction(acts, task["push_length"]), 4), same_bits=bool(same), **timing_fields(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunks", type=int, default=40)
    ap.add_argument("--chunk-samples", type=int, default=500)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--only", choices=["dynamics", "planner"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_rollout_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import _lib
    assert torch.cuda.is_available(), "bench_ragged_rollout.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = torch.device(args.device)
    _lib.lib()
    rows = []
    with torch.cuda.device(dev):
        if args.only in (None, "dynamics"):
            for mat, bsz, particles in DYNAMICS_CASES:
                for shared_state in (0, 1):
                    rows.append(dynamics_case(mat, bsz, particles, shared_state, dev, args.reps, args.warmup))
                    print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
                    _lib._WS.clear()
                    torch.cuda.empty_cache()
        if args.only in (None, "planner"):
            for mat, criterion in (("granular", "box"), ("rope", "chamfer")):
                rows.append(planner_case(mat, criterion, dev, args.chunks, args.chunk_samples, 200, args.reps, args.warmup))
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps(dict(bench="ragged_rollout", device=torch.cuda.get_device_name(dev), reps=args.reps, warmup=args.warmup,
                           timing="median wall clock of one call, attribute off / on alternating inside every repetition", cases=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
