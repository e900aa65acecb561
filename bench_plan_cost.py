"""The planner's trajectory cost in its two forms, measured in ONE run on one machine: `mpc.running_cost` with the tensor-op penalties of
`losses` (a few dozen launches over (bsz, L, n) temporaries) against `mpc.running_cost_fused` (`ag_plan_cost`: two launches that read every
predicted cloud once), on the same tensors.

Per case (penalty, bsz x L x n, criterion; clouds uniform in a square, every push starting near a particle, seeded) it reports
  tensor_ops_ms / fused_ms   the median over repetitions of the device time between two HIP events around one call, after warm-up, the two
                             forms alternating inside every repetition
  fused_graph_ms             the two `ag_plan_cost` launches captured in a HIP graph (the error term given), per replay: their device time
                             without the host's share of a call (the event pair around an eager call also holds the Python and ctypes
                             work in front of the first launch)
  chamfer_ms                 (chamfer criterion) the `ag_chamfer` call that both forms pay, alone
  copy_ms                    a plain device copy of bsz * L * n * 12 bytes in the same run: the lower bound of one pass over the clouds
  *_peak_mb                  torch.cuda.max_memory_allocated over one call, above what was allocated before it
  max_abs_diff               the largest difference of the two reward vectors
and one `MPPIPlanner.step` (1 024 samples x a 15-step push on rope-1k) scored either way.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
from functools import partial

import numpy as np

#        penalty     bsz    L  n     criterion
CASES = [("granular", 20000, 1, 200, "box"),          # config/planning/granular.yaml: no other cost kernel runs
         ("rope", 1024, 1, 1000, "chamfer"),
         ("rope", 1024, 3, 1000, "chamfer"),
         ("cloth", 512, 1, 4096, "chamfer")]
BBOX = np.array([[-1.0, 5.0], [-1.0, 5.0]])
BOX = np.array([[1.0, 2.5], [1.5, 3.0]], np.float32)


def make_inputs(penalty, B, L, n, rng):
    """Clouds uniform in [0, 4]^2 (a third of them with a particle near or beyond an edge of BBOX), pushes that start within 0.06 of a particle
    of the cloud they are measured against; sim_real_ratio 1."""
    state = rng.uniform(0, 4, (B, L, n, 3)).astype(np.float32)
    state[..., 1] *= 0.025
    init = state[0, 0].copy()
    edge = rng.uniform(-1.03, -0.97, (B, L)).astype(np.float32)
    state[::3, :, 0, 0] = edge[::3]
    prev = np.concatenate([np.broadcast_to(init[None, None], (B, 1, n, 3)), state[:, :-1]], 1)
    if penalty == "cloth":
        prev = np.broadcast_to(init[None, None], (B, L, n, 3))
    j = rng.integers(n, size=(B, L))
    at = np.take_along_axis(prev, j[:, :, None, None], 2)[:, :, 0]
    phi, d = rng.uniform(0, 2 * np.pi, (B, L)), rng.uniform(0.005, 0.06, (B, L))
    action = np.zeros((B, L, 4), np.float32)
    action[..., 0] = at[..., 0] + d * np.cos(phi)
    action[..., 1] = at[..., 2] + d * np.sin(phi)
    action[..., 2] = rng.uniform(-3.14, 3.14, (B, L))
    action[..., 3] = rng.uniform(5, 15, (B, L))
    return state, action, init


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternate(forms, reps, warmup):
    """forms: name -> callable.  Median ms per form, the forms taking turns inside every repetition."""
    ms = {k: [] for k in forms}
    for r in range(warmup + reps):
        for k, fn in forms.items():
            t, _ = timed(fn)
            if r >= warmup:
                ms[k].append(t)
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def peak_mb(fn):
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def planner_step(dev, reps, warmup):
    """bench_mpc.py's iteration (rope-1k, 1 024 samples, 15-step pushes, the engine's fast mode, shared-state rollout), scored either way."""
    import torch
    from adaptigraph_amd import configs, losses, mpc, synth
    from adaptigraph_amd.model import DynamicsPredictor
    mat, particles, samples, push_steps = "rope", 1000, 1024, 15
    task = configs.task_config(mat)
    lo, hi = np.array(task["action_lower_lim"], np.float32), np.array(task["action_upper_lim"], np.float32)
    lo[3], hi[3] = push_steps, push_steps + 0.5
    state, act = synth.make_mpc_inputs(mat, particles, 1, seed=0, len_lo=push_steps, len_hi=push_steps + 0.4, spacing=0.1)
    target = (state + np.array([0.4, 0.0, 0.3], np.float32)).astype(np.float32)
    bbox = np.array([[state[:, 0].min() - 5, state[:, 0].max() + 5], [state[:, 2].min() - 5, state[:, 2].max() + 5]])
    g = torch.Generator().manual_seed(0)
    ppm = configs.ppm_optimizer_stub(mat)
    ppm.physics_param = {mat: torch.tensor([0.5], device=dev)}
    state_t, target_t = torch.from_numpy(state).to(dev), torch.from_numpy(target).to(dev)
    model = DynamicsPredictor(configs.model_config(), configs.material_config(mat), configs.dataset_config(mat), dev)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.empty_like(p).uniform_(-1, 1, generator=g) / np.sqrt(p.shape[-1]))
    model = model.to(dev).eval().set_option("precision", 2)
    error, pen = partial(losses.chamfer, y=target_t[None]), partial(losses.rope_penalty, sim_real_ratio=task["sim_real_ratio"])
    kw = dict(n_sample=samples, n_update_iter=1, rollout_best=False, shared_state=True)
    planners = {"tensor_ops": mpc.MPPIPlanner(model, dev, ppm, error, pen, bbox, lo, hi, **kw),
                "fused": mpc.MPPIPlanner(model, dev, ppm, error, pen, bbox, lo, hi, penalty="rope", **kw)}
    torch.manual_seed(1234)
    smp = planners["fused"].sample(torch.from_numpy(act[0]).to(dev), 1)
    rewards = {k: p.step(state_t, smp)[1].clone() for k, p in planners.items()}
    ms = alternate({k: (lambda p=p: p.step(state_t, smp)) for k, p in planners.items()}, reps, warmup)
    return dict(workload=f"MPPIPlanner.step rope-{particles}, {samples} samples x {push_steps}-step push", tensor_ops_ms=ms["tensor_ops"],
                fused_ms=ms["fused"], max_abs_diff=float((rewards["fused"] - rewards["tensor_ops"]).abs().max()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30, help="timed repetitions per case and form")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--planner-reps", type=int, default=8)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "plan_cost_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import _lib, losses, mpc
    assert torch.cuda.is_available(), "bench_plan_cost.py measures the GPU kernels: it needs an MI355X (no fallback)"
    dev = torch.device(args.device)
    _lib.lib()
    penalties = {"rope": losses.rope_penalty, "cloth": losses.cloth_penalty, "granular": losses.granular_penalty}
    rng = np.random.default_rng(0)
    rows = []
    with torch.cuda.device(dev), torch.no_grad():
        for penalty, B, L, n, criterion in CASES:
            st, ac, si = (torch.from_numpy(a).to(dev) for a in make_inputs(penalty, B, L, n, rng))
            pen = partial(penalties[penalty], sim_real_ratio=1.0)
            if criterion == "box":
                ef, kw = partial(losses.box_loss, target=torch.from_numpy(BOX).to(dev)), dict(box_target=BOX)
            else:
                target = torch.from_numpy(rng.uniform(1, 3, (1, min(n, 1000), 3)).astype(np.float32)).to(dev)
                ef = partial(losses.chamfer, y=target)
                kw = dict(error_func=ef)
            forms = {"tensor_ops": lambda: mpc.running_cost(st, ac, si, ef, pen, BBOX)["reward_seqs"],
                     "fused": lambda: mpc.running_cost_fused(st, ac, si, BBOX, penalty, sim_real_ratio=1.0, **kw)["reward_seqs"]}
            got = {k: fn().clone() for k, fn in forms.items()}
            row = dict(penalty=penalty, B=B, L=L, n=n, criterion=criterion,
                       max_abs_diff=float((got["fused"] - got["tensor_ops"]).abs().max()))
            for k, fn in forms.items():
                row[k + "_peak_mb"] = peak_mb(fn)
            dst = torch.empty_like(st)
            extra = {"copy": lambda: dst.copy_(st)}
            if criterion == "chamfer":
                flat = st.reshape(B * L, n, 3)
                extra["chamfer"] = lambda: ef(flat)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            kwg = kw if criterion == "box" else dict(error_func=lambda s, e=ef(st.reshape(B * L, n, 3)).clone(): e)      # (the chamfer call stays outside)
            with torch.cuda.graph(graph):
                captured = mpc.running_cost_fused(st, ac, si, BBOX, penalty, sim_real_ratio=1.0, **kwg)["reward_seqs"]
            extra["fused_graph"] = graph.replay
            ms = alternate({**forms, **extra}, args.reps, args.warmup)
            assert torch.equal(captured, got["fused"]), "the replayed call differs from the eager one"
            row.update({k + "_ms": v for k, v in ms.items()})
            row["state_mb"] = round(B * L * n * 12 / 2 ** 20, 2)
            rows.append(row)
            del st, ac, si, dst
        step = planner_step(dev, args.planner_reps, 2)
    line = json.dumps(dict(bench="plan_cost", device=torch.cuda.get_device_name(dev), reps=args.reps, warmup=args.warmup,
                           timing="median of HIP-event times around one call, forms alternating", cases=rows, planner_step=step))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
