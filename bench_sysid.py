"""Physics-parameter identification by sweep and by gradient, measured in ONE run on one machine: `physics_param_optimizer.optimize` with
method="sweep" (the derivative-free batched search) and method="gd" (Adam through `dynamics_masked_differentiable` and the differentiable
masked chamfer), on a 1-parameter and a 2-parameter synthetic rope task whose observations come from `dynamics_masked` at planted parameters.

Per task and method: wall time of the whole `optimize` call (median of --reps, after one warm-up call), the graph-steps it rolled out (samples
of a rollout call x its model steps, summed over the calls; for "gd" the differentiable ones — each also run backwards — counted apart), the
final objective (`dynamics_error` at the returned point) and the returned point.  Then, for one forward + backward of the gd batch at
--mem-steps model steps, the peak device memory with and without checkpoint_steps.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import time

import numpy as np

PLANTED = {1: [0.3], 2: [0.3, 0.7]}
W0 = "particle_encoder.model.0.weight"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iterations", type=int, default=60, help="`iterations` of optimize, for both methods")
    ap.add_argument("--interactions", type=int, default=4)
    ap.add_argument("--particles", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mem-steps", type=int, default=6)
    ap.add_argument("--mem-batch", type=int, default=16)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "sysid_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import configs, forward_dynamics as fd, physics_param_optimizer as ppo, synth
    from adaptigraph_amd.model import DynamicsPredictor
    assert torch.cuda.is_available(), "bench_sysid.py measures the GPU paths: it needs an MI355X (no fallback)"
    dev = args.device
    tg = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    weights = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "weights_seed0.npz")))

    def make(dims):
        """A rope task with `dims` used physics parameters (the second: a seeded permutation of the first's input column) on seed-0 weights."""
        w = {k: v.copy() for k, v in weights.items()}
        if dims == 2:
            w[W0] = np.insert(w[W0], 3, w[W0][np.random.default_rng(2).permutation(w[W0].shape[0]), 2], axis=1)
        params = [{"name": "particle_radius", "use": False, "min": 0.0, "max": 1.0}]
        params += [{"name": f"param{i}", "use": True, "min": 0.0, "max": 1.0} for i in range(dims)]
        model = DynamicsPredictor(configs.model_config(), {"material_index": {"rope": 0}, "rope": {"physics_params": params}},
                                  configs.dataset_config("rope"), dev)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        model = model.to(dev).eval()
        task = dict(configs.task_config("rope"), max_nobj=args.particles, material_dims={"rope": dims})
        return ppo.PhysicsParamOnlineOptimizer(task, model, "rope", dev, ".")

    def interactions(ppm, dims, n_int, lo, hi, seed=51):
        n = args.particles
        obj, act = synth.make_mpc_inputs("rope", n, n_int, n_look=1, seed=seed, len_lo=lo, len_hi=hi, spacing=0.1)
        rng = np.random.default_rng(seed + 100)
        state, mask = np.zeros((n_int, n, 3), np.float32), np.zeros((n_int, n), bool)
        for b in range(n_int):
            c = n - (0, 3, 7, 2, 5, 1, 6, 4)[b % 8]
            state[b, :c] = obj[:c] + rng.normal(0, 0.003, (c, 3)).astype(np.float32)
            mask[b, :c] = True
        real = fd.dynamics_masked(tg(state), tg(mask), tg(act[:, 0]), ppm.model, dev, ppm,
                                  physics_param={"rope": torch.tensor(PLANTED[dims], device=dev)})["state_seqs"].cpu().numpy()
        cnt = mask.sum(1)
        return ([act[i, 0] for i in range(n_int)], [state[i, :cnt[i]] for i in range(n_int)], [real[i, :cnt[i]] for i in range(n_int)],
                (state, mask, act[:, 0]))

    # graph-steps: every rollout call of the optimizer, counted where it enters forward_dynamics
    steps = {"plain": 0, "differentiable": 0}

    def counted(fn, key):
        def run(state_init, state_mask, action, *a, **kw):
            steps[key] += int(action.shape[0]) * int(action[:, 3].max().item())
            return fn(state_init, state_mask, action, *a, **kw)
        return run
    ppo.dynamics_masked = counted(fd.dynamics_masked, "plain")
    ppo.dynamics_masked_differentiable = counted(fd.dynamics_masked_differentiable, "differentiable")

    rows = []
    for dims in (1, 2):
        ppm = make(dims)
        acts, inits, reals, _ = interactions(ppm, dims, args.interactions, 2.0, 4.9)
        for method in ("sweep", "gd"):
            times = []
            for rep in range(args.reps + 1):
                steps["plain"] = steps["differentiable"] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                p, err, err0 = ppo.optimize(ppm, acts, inits, reals, reals, iterations=args.iterations, method=method)
                torch.cuda.synchronize()
                if rep:
                    times.append(time.perf_counter() - t0)
            rows.append(dict(task=f"rope-{args.particles} x {args.interactions} interactions, {dims} parameter(s)", planted=PLANTED[dims],
                             method=method, iterations=args.iterations, wall_s=round(statistics.median(times), 4),
                             graph_steps_forward_only=steps["plain"], graph_steps_forward_backward=steps["differentiable"],
                             objective=err, objective_at_start=err0, recovered=[round(float(v), 5) for v in p]))
    # peak memory of one gd iteration's forward + backward, with and without checkpoint_steps
    ppm = make(1)
    _, _, _, (state, mask, act) = interactions(ppm, 1, args.mem_batch, args.mem_steps, args.mem_steps + 0.9)
    peak = {}
    for ck in (False, True, False, True):      # (the first pair warms caches and workspaces up)
        P = torch.full((args.mem_batch, 1), 0.5, device=dev, requires_grad=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fd.dynamics_masked_differentiable(tg(state), tg(mask), tg(act), ppm.model, dev, ppm, physics_param={"rope": P}, checkpoint_steps=ck)
        out["state_seqs"].square().sum().backward()
        torch.cuda.synchronize()
        peak[ck] = torch.cuda.max_memory_allocated() - base
        del out, P
    res = dict(bench="sysid", device=torch.cuda.get_device_name(0), rows=rows,
               memory=dict(shape=f"{args.mem_batch} samples x {args.particles + 1} nodes x {args.mem_steps} model steps, forward + backward",
                           peak_bytes_plain=peak[False], peak_bytes_checkpoint_steps=peak[True]))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
