"""The evaluation rollout's step loop against the scripted call (`ag_rollout_scripted`), measured in ONE run.

Two shapes:
  valid    the validation driver: 128 start graphs x (max_nobj 100 + 1 tool) slots x 100 model steps (eval_rollout.ROLLOUT_STEPS), variant "single"
  rope1k   16 graphs x (1 000 + 1) slots x 20 steps
Per shape, in ms for a whole rollout, the median (and min / max) over `--reps` passes after `--warmup` warm ones, host clock around a pass that
ends in a device synchronise, the three forms alternating pass by pass:
  loop      the step loop of eval_rollout.rollout_batch as the parent commit runs it: per step build_edges + model(...) + the error on the
            device + cat / shift / action in torch
  scripted  forward_dynamics.rollout_scripted, errors included
  graph     the same call captured once with torch.cuda.graph and replayed
Before anything is timed the scripted call's predictions are compared with the loop's bit for bit and its errors within (n_p + 8) 2^-24.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import time

import numpy as np

SHAPES = {"valid": dict(n_obj=100, batch=128, steps=100, spacing=0.2), "rope1k": dict(n_obj=1000, batch=16, steps=20, spacing=0.1)}
RADIUS, TOPK = 0.5, 10


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--shapes", default="valid,rope1k")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "eval_rollout_bench.txt"))
    args = ap.parse_args()
    assert args.reps >= 5 and args.warmup >= 1
    import torch
    from adaptigraph_amd import _lib, configs, graph, synth
    from adaptigraph_amd.forward_dynamics import rollout_scripted
    from adaptigraph_amd.model import DynamicsPredictor
    assert torch.cuda.is_available(), "bench_eval_rollout.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = torch.device(args.device)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    w = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "weights_seed0.npz")))
    model = DynamicsPredictor(configs.model_config(), configs.material_config("rope"), configs.dataset_config("rope"), dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    model = model.to(dev).eval()

    def measure(name, n_obj, batch, steps, spacing):
        g = synth.make_graph_inputs("rope", n_obj, batch, seed=2, spacing=spacing)
        n_p, B, T = g["n_p"], batch, steps
        rng = np.random.default_rng(3)
        tool0 = g["state"][:, -1, n_p:]
        # a recorded push: the tool moves along the rope by 0.02 per step; ground truth = the start cloud + noise
        eef_start = np.stack([tool0 + np.array([0.02 * k, 0.0, 0.0], np.float32) for k in range(T)], 1).astype(np.float32)
        eef_delta = np.broadcast_to(np.array([0.02, 0.0, 0.0], np.float32), eef_start.shape).copy()
        gt = (g["state"][:, -1:, :n_p] + rng.normal(0, 0.02, (B, T, n_p, 3))).astype(np.float32)
        state0, action0, attrs, p_instance, phys = t(g["state"]), t(g["action"]), t(g["attrs"]), t(g["p_instance"]), t(g["phys"])
        mask, tool_mask, obj_mask = t(g["mask"]), t(g["tool_mask"]), t(g["mask"][:, :n_p].copy())
        eef_start, eef_delta, gt = t(eef_start), t(eef_delta), t(gt)
        thr = graph.threshold_sq(RADIUS, B, dev, _lib.AG_VARIANT_SINGLE)
        n_valid = obj_mask.sum(1).clamp_min(1).float()

        def loop(keep=False):
            state, action = state0, action0
            errors = torch.zeros((B, T), device=dev)
            preds = []
            for k in range(T):
                edges = graph.build_edges(state[:, -1], RADIUS, mask, tool_mask, TOPK, False, "single", max_tools=1)
                pred, _ = model(state, attrs, edges, None, p_instance, action=action, rope_physics_param=phys)
                errors[:, k] = ((pred - gt[:, k]).norm(dim=-1) * obj_mask).sum(1) / n_valid
                if keep:
                    preds.append(pred)
                if k + 1 < T:
                    nxt = torch.cat([pred, eef_start[:, k + 1]], 1)
                    state = torch.cat([state[:, 1:], nxt[:, None]], 1)
                    action = torch.zeros_like(action)
                    action[:, n_p:] = eef_delta[:, k + 1]
            return errors, preds

        def scripted(return_pred=False):
            return rollout_scripted(model, state0, action0, eef_start, eef_delta, attrs, p_instance, phys, mask, tool_mask, thr, TOPK, False, 1,
                                    variant="single", gt=gt, obj_mask=obj_mask, return_pred=return_pred)

        errors, preds = loop(keep=True)
        out = scripted(return_pred=True)
        assert torch.equal(out["pred_seq"], torch.stack(preds, 1)), f"{name}: the scripted call's predictions differ from the loop's"
        rel = float(((out["err"] - errors).abs() / errors).max())
        assert rel <= (n_p + 8) * 2.0 ** -24, f"{name}: errors differ by {rel:.3e}"
        del preds, out
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            scripted()
        torch.cuda.current_stream().wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            captured = scripted()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured["err"], scripted()["err"]), f"{name}: the replayed graph differs from the call"
        forms = {"loop": loop, "scripted": scripted, "graph": gr.replay}
        times = {k: [] for k in forms}
        for r in range(args.warmup + args.reps):
            for k, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        row = dict(shape=name, B=B, N=n_p + 1, steps=T, err_rel_dev=rel)
        for k, v in times.items():
            row[k + "_ms"] = round(statistics.median(v), 3)
            row[k + "_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
        row["loop_over_scripted"] = round(row["loop_ms"] / row["scripted_ms"], 3)
        row["loop_over_graph"] = round(row["loop_ms"] / row["graph_ms"], 3)
        return row

    rows = [measure(name, **SHAPES[name]) for name in args.shapes.split(",")]
    line = json.dumps(dict(bench="eval_rollout", device=torch.cuda.get_device_name(0), precision=model.get_option("precision"), reps=args.reps,
                           warmup=args.warmup, shapes=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
