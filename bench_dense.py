"""Dense one-hot Rr / Rs <-> CSR: the host functions against the HIP kernels (`ag_edges_from_dense`, `ag_edges_to_dense`), measured in ONE run.

Two shapes:
  train    the reference training batch: 128 rope key-point graphs, max_nobj 100 + max_neef 1 slots, relation rows padded to max_nR 1000
           (src/config/dynamics/rope.yaml:19-26; `configs.dataset_config` carries only the keys the model reads, not these, so the shipped
           values are restated in TRAIN below)
  planner  a planner chunk: 500 samples x 201 slots (config/planning/rope.yaml: max_nobj 200 + 1 tool), edges of `build_edges` on a synthetic
           rope, E = the batch maximum
Per shape, medians over warmed repetitions, in ms:
  from_host / from_device        `graph.csr_from_dense` against `graph.csr_from_dense_device`, host clock around a call followed by a device
                                 synchronise; from_device_events: the device work alone between two HIP events, and the rate at which it reads
                                 the 2 B E N 4 bytes it must read (all five launches, so a lower bound for the row scan itself)
  to_dense_torch / to_dense / to_dense_e_max
                                 the torch construction `CSREdges.to_dense` used before the kernel (kept here as the yardstick), `to_dense()` (one
                                 host read for the shape, then the kernel) and `to_dense(e_max=E)` (no host read); to_dense_events and the rate
                                 at which it writes its 2 B E N 4 bytes
  forward                        one `model(**graph)` on the CSR adjacency of `build_edges`, same run: what the conversion is added to;
                                 forward_dense_inputs: the same call on the dense pair (conversion included); forward_e_cap_BE: on the CSR the
                                 device conversion returns, whose capacity is the bound B E (the edge count stays on the device)
Every device result is checked against the host result before anything is timed.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import time

import numpy as np

TRAIN = dict(batch=128, max_nobj=100, max_neef=1, max_nR=1000, spacing=0.2)
PLANNER = dict(batch=500, n_obj=200, spacing=0.1)


def to_dense_torch(torch, csr):
    n = csr.n_rel()
    e_max = int(n.max().item())
    total = int(csr.row_ptr[-1].item())
    dev = csr.row_ptr.device
    Rr = torch.zeros((csr.B, e_max, csr.N), device=dev)
    Rs = torch.zeros((csr.B, e_max, csr.N), device=dev)
    r, s = csr.edge_recv[:total].long(), csr.edge_send[:total].long()
    b = r // csr.N
    idx = torch.arange(total, device=dev) - csr.row_ptr.long()[b * csr.N]
    Rr[b, idx, r - b * csr.N] = 1
    Rs[b, idx, s - b * csr.N] = 1
    return Rr, Rs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "dense_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import configs, graph, synth
    from adaptigraph_amd.model import DynamicsPredictor
    assert torch.cuda.is_available(), "bench_dense.py measures the GPU path: it needs an MI355X (no fallback)"
    dev = args.device
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def wall_ms(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    def event_ms(fn):
        ts = []
        for r in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    w = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "weights_seed0.npz")))
    model = DynamicsPredictor(configs.model_config(), configs.material_config("rope"), configs.dataset_config("rope"), dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    model = model.to(dev).eval()

    def measure(name, g, e_rows):
        csr = graph.build_edges(t(g["state"][:, -1]), 0.5, t(g["mask"]), t(g["tool_mask"]), 10, False, "batch", max_tools=1)
        e_max = int(csr.n_rel().max())
        E = e_max if e_rows is None else e_rows
        assert E >= e_max, f"{name}: {e_max} edges in a sample, {E} rows"
        Rr, Rs = csr.to_dense(e_max=E)
        B, _, N = Rr.shape
        host, devc = graph.csr_from_dense(Rr, Rs), graph.csr_from_dense_device(Rr, Rs)
        total = int(host.row_ptr[-1])
        assert torch.equal(host.row_ptr, devc.row_ptr) and torch.equal(host.edge_recv[:total], devc.edge_recv[:total]) and \
            torch.equal(host.edge_send[:total], devc.edge_send[:total]), name
        old = to_dense_torch(torch, csr)
        new = csr.to_dense()
        assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1]) and torch.equal(Rr[:, :e_max], old[0]), name
        del old, new, host, devc
        nbytes = 2 * B * E * N * 4
        row = dict(shape=name, B=B, E=E, N=N, edges=total, dense_bytes=nbytes)
        row["from_host_ms"] = round(wall_ms(lambda: graph.csr_from_dense(Rr, Rs)), 4)
        row["from_device_ms"] = round(wall_ms(lambda: graph.csr_from_dense_device(Rr, Rs)), 4)
        ev = event_ms(lambda: graph.csr_from_dense_device(Rr, Rs))
        row["from_device_events_ms"] = round(ev, 4)
        row["from_device_read_GBps"] = round(nbytes / ev / 1e6, 1)
        row["from_ratio_host_over_device"] = round(row["from_host_ms"] / row["from_device_ms"], 2)
        row["to_dense_torch_ms"] = round(wall_ms(lambda: to_dense_torch(torch, csr)), 4)
        row["to_dense_ms"] = round(wall_ms(lambda: csr.to_dense()), 4)
        row["to_dense_e_max_ms"] = round(wall_ms(lambda: csr.to_dense(e_max=e_max)), 4)
        ev = event_ms(lambda: csr.to_dense(e_max=e_max))
        row["to_dense_events_ms"] = round(ev, 4)
        row["to_dense_write_GBps"] = round(2 * B * e_max * N * 4 / ev / 1e6, 1)
        row["to_ratio_torch_over_e_max"] = round(row["to_dense_torch_ms"] / row["to_dense_e_max_ms"], 2)
        kw = dict(state=t(g["state"]), attrs=t(g["attrs"]), p_instance=t(g["p_instance"]), action=t(g["action"]), rope_physics_param=t(g["phys"]))
        row["forward_ms"] = round(wall_ms(lambda: model(Rr=csr, Rs=None, **kw)), 4)
        row["forward_dense_inputs_ms"] = round(wall_ms(lambda: model(Rr=Rr, Rs=Rs, **kw)), 4)
        wide = graph.csr_from_dense_device(Rr, Rs)          # the same edges with e_cap = B E instead of the builder's bound: what the capacity alone costs
        row["forward_e_cap_BE_ms"] = round(wall_ms(lambda: model(Rr=wide, Rs=None, **kw)), 4)
        row["e_cap_builder"], row["e_cap_BE"] = int(csr.e_cap), int(wide.e_cap)
        return row

    c = TRAIN
    g = synth.make_graph_inputs("rope", c["max_nobj"], c["batch"], seed=0, spacing=c["spacing"])
    assert g["attrs"].shape[1] == c["max_nobj"] + c["max_neef"]
    rows = [measure("train", g, c["max_nR"])]
    c = PLANNER
    rows.append(measure("planner", synth.make_graph_inputs("rope", c["n_obj"], c["batch"], seed=1, spacing=c["spacing"]), None))
    line = json.dumps(dict(bench="dense", device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, shapes=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
