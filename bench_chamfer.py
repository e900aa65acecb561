"""The chamfer cost in its two forms, measured in ONE run on one machine: the LDS-resident kernels (`ag_chamfer`, `ag_chamfer_fwd_idx`,
`ag_chamfer_backward`: one workgroup per sample, N + M <= 12 800) against the tiled ones (`ag_chamfer_tiled`, `ag_chamfer_tiled_backward`:
query tiles over many workgroups, any size).

Per shape (B x N x M, normal clouds, seeded) and per operation
  fwd       the value alone
  fwd_idx   the value and the nearest-neighbour indices (the forward under autograd)
  bwd_gx    the backward into the particles
  bwd_gxgy  the backward into particles and target (a broadcast target: with the sum over the samples' rows)
it reports the median over repetitions of the device time between two HIP events around one call, after warm-up, the two forms alternating
inside every repetition.  Where both forms apply their outputs are compared bit for bit before anything is timed.  Prints one JSON line and
writes it to --out.
"""
import argparse
import ctypes
import json
import os
import statistics

import numpy as np

#          B     N      M      target        forms
SHAPES = [(1024, 1000, 1000, "broadcast", ("resident", "tiled")),      # the planner's call
          (64, 1000, 11800, "broadcast", ("resident", "tiled")),       # at the resident limit
          (1, 6400, 6400, "per-sample", ("resident", "tiled")),
          (64, 1000, 50000, "broadcast", ("tiled",)),
          (1, 50000, 50000, "per-sample", ("tiled",))]
OPS = ("fwd", "fwd_idx", "bwd_gx", "bwd_gxgy")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20, help="timed repetitions per shape, operation and form")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "chamfer_tiled_bench.txt"))
    args = ap.parse_args()
    import torch
    from adaptigraph_amd import _lib
    assert torch.cuda.is_available(), "bench_chamfer.py measures the GPU kernels: it needs an MI355X (no fallback)"
    dev = torch.device(args.device)
    L = _lib.lib()
    tq, to = ctypes.c_int(0), ctypes.c_int(0)
    L.ag_chamfer_tile_sizes(ctypes.byref(tq), ctypes.byref(to))
    rng = np.random.default_rng(0)
    rows = []
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for B, N, M, target, forms in SHAPES:
            yb = 1 if (target == "per-sample" and B > 1) else 0
            By = B if yb else 1
            x = torch.from_numpy(rng.normal(0, 2, (B, N, 3)).astype(np.float32)).to(dev)
            y = torch.from_numpy(rng.normal(0.3, 2, (By, M, 3)).astype(np.float32)).to(dev)
            g = torch.from_numpy(rng.uniform(0.5, 2.0, B).astype(np.float32)).to(dev)
            nbytes = L.ag_chamfer_tiled_workspace_bytes(B, N, M)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            buf = {f: dict(out=torch.empty(B, device=dev), ix=torch.empty((B, N), dtype=torch.int32, device=dev),
                           iy=torch.empty((B, M), dtype=torch.int32, device=dev), gx=torch.empty((B, N, 3), device=dev),
                           gy=torch.empty((B, M, 3), device=dev)) for f in forms}

            def call(form, op):
                b = buf[form]
                p = {k: v.data_ptr() for k, v in b.items()}
                if op in ("fwd", "fwd_idx"):
                    ix, iy = (p["ix"], p["iy"]) if op == "fwd_idx" else (None, None)
                    if form == "tiled":
                        rc = L.ag_chamfer_tiled(x.data_ptr(), None, y.data_ptr(), None, B, N, M, yb, p["out"], ix, iy, ws.data_ptr(), nbytes, stream)
                    elif op == "fwd":
                        rc = L.ag_chamfer(x.data_ptr(), y.data_ptr(), B, N, M, yb, p["out"], stream)
                    else:
                        rc = L.ag_chamfer_fwd_idx(x.data_ptr(), None, y.data_ptr(), None, B, N, M, yb, p["out"], ix, iy, stream)
                else:
                    fn = L.ag_chamfer_tiled_backward if form == "tiled" else L.ag_chamfer_backward
                    rc = fn(x.data_ptr(), None, y.data_ptr(), None, p["ix"], p["iy"], g.data_ptr(), B, N, M, yb, p["gx"],
                            p["gy"] if op == "bwd_gxgy" else None, stream)
                assert rc == 0, L.ag_last_error()

            for f in forms:                                  # results first: the value, then with indices, then both backwards
                for op in OPS:
                    call(f, op)
                    if op == "fwd":
                        buf[f]["value"] = buf[f]["out"].clone()
            torch.cuda.synchronize()
            same = None
            if len(forms) == 2:
                a, b = buf["resident"], buf["tiled"]
                same = bool(all(torch.equal(a[k], b[k]) for k in ("value", "out", "ix", "iy", "gx")) and torch.equal(a["gy"][:By], b["gy"][:By]))
                assert same, f"the two forms differ at {(B, N, M)}"
            ms = {f: {op: [] for op in OPS} for f in forms}
            for op in OPS:
                for r in range(args.warmup + args.reps):
                    for f in forms:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        call(f, op)
                        e1.record()
                        e1.synchronize()
                        if r >= args.warmup:
                            ms[f][op].append(e0.elapsed_time(e1))
            row = dict(B=B, N=N, M=M, target=target, bit_equal=same)
            for f in forms:
                row[f + "_ms"] = {op: round(statistics.median(ms[f][op]), 4) for op in OPS}
            rows.append(row)
    line = json.dumps(dict(bench="chamfer", device=torch.cuda.get_device_name(dev), query_tile=tq.value, other_chunk=to.value, reps=args.reps,
                           warmup=args.warmup, timing="median of HIP-event times around one call", shapes=rows))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
