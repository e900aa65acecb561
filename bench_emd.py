"""The earth-mover loss on the device (`losses.emd`: ag_emd, one wave per sample) against the host procedure of dynamics/gnn/loss.py:29-55,
measured in ONE run on one machine.

  device   median over repetitions of the HIP-event time around one `ag_emd` call (forward with the assignment), and around one
           `ag_emd_backward` call, after warm-up
  host     median wall time of: the (B,N,M) distance tensor on the GPU, its copy to the host, scipy.optimize.linear_sum_assignment per sample,
           the gather of the pairs and the mean on the GPU.  Printed only when scipy imports (the package does not need it); otherwise the
           script says so and reports the device times alone.

Shapes: 128 x 100 x 100 (the training batch), 128 x 200 x 200 and 16 x 1000 x 1000 Gaussian clouds, and the chain (x_n = (n,0,0), y_m = (m+0.4,0,0),
the rows in descending order: every augmentation walks the chain it has built) at 256 x L x L for L = AG_EMD_MAX_POINTS and the powers of two
below it: the case that sets the size limit (one launch of 256 samples under 1 s).  Then one training step (forward, backward,
Adam) on the synthetic rope batch of bench_train.py with the `mse` objective and with `emd`.

The first launch at a new shape is ONE sample in a child process under its own time limit; the batch is run only if that sample came back
under --single-limit-ms, and nothing more is started after a child that failed or ran out of time.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
GAUSS = [(128, 100, 100), (128, 200, 200), (16, 1000, 1000)]


def clouds(kind, B, N, M, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal((B, N, 3)).astype(np.float32), rng.standard_normal((B, M, 3)).astype(np.float32)
    x, y = np.zeros((B, N, 3), np.float32), np.zeros((B, M, 3), np.float32)
    x[:, :, 0] = np.arange(N, dtype=np.float32)[::-1]
    y[:, :, 0] = np.arange(M, dtype=np.float32) + np.float32(0.4)
    return x, y


def device_ms(torch, fn, reps, warmup):
    ms = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 4)


def emd_calls(torch, _lib, kind, B, N, M, dev):
    """-> (forward, backward, out): closures over one `ag_emd` / `ag_emd_backward` call on fixed buffers."""
    x, y = (torch.from_numpy(a).to(dev) for a in clouds(kind, B, N, M))
    out = torch.empty(B, device=dev)
    col, row = torch.empty((B, N), dtype=torch.int32, device=dev), torch.empty((B, M), dtype=torch.int32, device=dev)
    g, gx, gy = torch.ones(B, device=dev), torch.empty_like(x), torch.empty_like(y)
    yb = 1 if B > 1 else 0
    fwd = lambda: _lib.call("ag_emd", dev, x, None, y, None, B, N, M, yb, out, col, row)
    bwd = lambda: _lib.call("ag_emd_backward", dev, x, y, col, row, g, B, N, M, yb, gx, gy)
    return fwd, bwd, (x, y, out, col)


def probe(kind, N, M):
    """Child process: one sample, one launch, its device time."""
    import torch
    from adaptigraph_amd import _lib
    dev = torch.device("cuda:0")
    fwd, _, _ = emd_calls(torch, _lib, kind, 1, N, M, dev)
    print(json.dumps(dict(single_ms=device_ms(torch, fwd, 1, 0))))


def host_procedure(torch, scipy_optimize, x, y):
    """dynamics/gnn/loss.py:32-54 as written there: distance tensor, copy, scipy per sample, gather, mean."""
    dis = torch.norm(x[:, :, None, :] - y[:, None, :, :], 2, dim=3)
    xs, ys = [], []
    for i in range(dis.shape[0]):
        i1, i2 = scipy_optimize.linear_sum_assignment(dis[i].detach().cpu().numpy())
        xs.append(x[i, i1])
        ys.append(y[i, i2])
    return torch.mean(torch.norm(torch.stack(xs) - torch.stack(ys), 2, dim=2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--single-limit-ms", type=float, default=1000.0, help="a shape whose single sample takes longer is not run as a batch")
    ap.add_argument("--probe-timeout", type=int, default=120, help="seconds a single-sample child process may take, start-up included")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emd_bench.txt"))
    ap.add_argument("--probe", nargs=3, metavar=("KIND", "N", "M"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.probe:
        return probe(args.probe[0], int(args.probe[1]), int(args.probe[2]))
    try:
        import scipy.optimize as scipy_optimize
    except ImportError:
        scipy_optimize = None
        print("scipy does not import here: the host column is left out, the device times stand alone", flush=True)
    import torch
    from adaptigraph_amd import _lib, gnn_loss
    assert torch.cuda.is_available(), "bench_emd.py measures the GPU kernels: it needs an MI355X (no fallback)"
    dev = torch.device("cuda:0")
    limit = _lib.AG_EMD_MAX_POINTS
    chain = []
    L = limit
    while L >= 128:
        chain.append((256, L, L))
        L //= 2
    rows, stopped = [], None
    for kind, shapes in (("chain", chain), ("gauss", GAUSS)):
        for B, N, M in shapes:
            row = dict(kind=kind, B=B, N=N, M=M)
            rows.append(row)
            try:
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--probe", kind, str(N), str(M)], capture_output=True, text=True,
                                       timeout=args.probe_timeout, cwd=ROOT)
            except subprocess.TimeoutExpired:
                stopped = f"the single sample of {kind} {N} x {M} did not finish in {args.probe_timeout} s"
                break
            if child.returncode != 0:
                stopped = f"the single sample of {kind} {N} x {M} failed ({child.returncode}): {child.stderr[-300:]}"
                break
            row["single_ms"] = json.loads(child.stdout.strip().splitlines()[-1])["single_ms"]
            if row["single_ms"] > args.single_limit_ms:
                row["batch"] = "not run: the single sample is over the limit"
                continue
            fwd, bwd, (x, y, out, col) = emd_calls(torch, _lib, kind, B, N, M, dev)
            fwd()
            torch.cuda.synchronize()
            row["value"] = float(out.double().mean())
            row["emd_ms"] = device_ms(torch, fwd, args.reps, args.warmup)
            row["emd_backward_ms"] = device_ms(torch, bwd, args.reps, args.warmup)
            if scipy_optimize is not None and kind == "gauss":
                ms = []
                for _ in range(args.host_reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ref = host_procedure(torch, scipy_optimize, x, y)
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
                row["host_ms"] = round(statistics.median(ms), 3)
                row["host_value"] = float(ref)
                row["speedup"] = round(row["host_ms"] / row["emd_ms"], 1)
        if stopped:
            break
    result = dict(bench="emd", device=torch.cuda.get_device_name(dev), limit=limit, reps=args.reps, warmup=args.warmup,
                  timing="device: median of HIP-event times around one call; host: median wall time with synchronisation",
                  host="scipy " + __import__("scipy").__version__ if scipy_optimize is not None else "not measured: scipy does not import",
                  shapes=rows)
    if stopped:
        result["stopped"] = stopped
    else:
        ok = [r["N"] for r in rows if r["kind"] == "chain" and r.get("emd_ms", float("inf")) < 1000.0]
        result["chain_limit"] = max(ok) if ok else None
        result["train_step_ms"] = train_steps(torch, gnn_loss, dev, args.train_steps)
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


def train_steps(torch, gnn_loss, dev, steps):
    """One optimisation step (forward over 3 future frames, backward, Adam) on the synthetic rope batch, per objective."""
    from adaptigraph_amd import configs, train_ops
    from adaptigraph_amd.train_model import TrainableDynamicsPredictor, unrolled_loss
    from adaptigraph_amd.train_ops import EdgeViews
    from bench_train import synthetic_batch, timed
    out = {}
    for name, spec in (("mse", [["mse", 1]]), ("emd", [["emd", 1]]), ("mse+emd", [["mse", 1], ["emd", 1]])):
        torch.manual_seed(0)
        model = TrainableDynamicsPredictor(configs.model_config(), configs.material_config("rope"), configs.dataset_config("rope"), dev).to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        data, csr = synthetic_batch(128, 100, dev)
        data.update(Rr=csr, Rs=None, edge_views=EdgeViews(csr))
        funcs = gnn_loss.build_loss_funcs(gnn_loss.parse_loss_spec(spec), data["p_instance"][..., 0] != 0)

        def step():
            opt.zero_grad(set_to_none=False)
            with train_ops.direct_grads(model.fused_dense):
                loss = unrolled_loss(model, data, 3, funcs)
                loss.backward()
            opt.step()
            return loss

        ms, loss = timed(step, steps, 3)
        out[name] = dict(ms=round(ms, 3), loss=float(loss.detach()))
    return out


if __name__ == "__main__":
    main()
