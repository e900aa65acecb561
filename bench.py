#!/usr/bin/env python3
"""Headline benchmark: rollout graph-steps/s (batch x steps / wall) on N MI355X — BASELINE.json `metric`.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch: `dynamics()` on `--batch` action samples per GPU
(default 256) of the rope-1k cloud with a `--rollout-steps`-step (default 10) push, i.e. BASELINE configs[1]
"rope, ~1k particles, batch 256, 10-step rollout": per model step a radius-graph rebuild, the GNN forward and
the state/tool update for every graph.  Multi-GPU: the batch shards across ranks with no data-path collective
(weak scaling: per-GPU batch fixed), then ONE RCCL all-gather of the predicted states (north_star).

A plain run sets up, warms up, times `--steps` passes and prints one JSON line on rank 0 (`metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step` = milliseconds of one timed pass, `config`, and `ranks` for N > 1).
`--dump-outputs DIR` writes what the last timed pass returned (`state_seqs`, `action_seqs`; float32) as DIR/<name>.npy, rows of a
fixed seeded sample of the batch if the whole would exceed 64 MB; the inputs are seeded, so two builds can be compared output for output.
`--full` adds everything below (each of `--no-profile`, `--no-extra`, `--no-cpu-baseline` drops its part of it):
  roofline      the edge encoder (MFMA-bound): achieved = F_min FLOP (140 100 per edge) x edges per
                launch / average launch time, measured live with HIP events on the launch stream in a single-stream
                pass, against the dense bf16/f16 MFMA peak (split modes) or the fp32 MFMA peak (f32 mode);
                `mfma_issue_util` = the same with the 2 (mode "fast": f16 x split-f16) or 3 (split-bf16) MFMAs the edge stack
                issues per fp32 product; `issue_frac_of_sustained` = issued FLOP/s against what pure MFMA chains sustain on random
                operands under the chip's power limit (`sustained_peak_measured`, profiles/r02_power_probe.txt);
                `traffic` = HBM bytes per launch from the PMC passes recorded in profiles/pmc_traffic.json, used only
                if that file was collected from the kernel sources being run (sha256 of adaptigraph_amd/csrc), else null
  roofline_hbm  the segment-reduce kernel (HBM-bound), same accounting against 8 TB/s
  cpu_baseline  the CPU oracle ("port") on a bounded sample of the same workload on this box's cores (N = 1 only);
                cpu_baseline_dense_bmm = the reference's dense one-hot-bmm formulation in PyTorch-CPU on a smaller sample
  extra         (N = 1 only) the exact-fp32 engine mode on the same workload, BASELINE configs[2] / [3] per-GPU shapes
                (granular-2k batch 128, cloth-4k batch 64 x 20 steps) and configs[4] (one MPPI iteration, 1024 x 15 on
                rope-1k), each a short timed run of its own
  ranks         (N > 1) per-rank rollout / all-gather milliseconds per step (min / max over ranks; in a plain run too)
"""
import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import sys
import time

_T_START = time.perf_counter()       # wall-clock legs of this process (`legs_s` in the JSON line): everything below is attributed to a named leg
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on these hosts (RCCL across processes needs it)

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from adaptigraph_amd import _lib, configs, synth                       # noqa: E402
from adaptigraph_amd import dist as agdist                             # noqa: E402
from adaptigraph_amd.forward_dynamics import dynamics                  # noqa: E402
from adaptigraph_amd.model import DynamicsPredictor                    # noqa: E402

LEGS = {"import": time.perf_counter() - _T_START}      # (a fresh box pages torch + ROCm in from the image: minutes, not this program's doing)


@contextlib.contextmanager
def leg(name):
    """Attribute the wall-clock of a block to `legs_s[name]` (accumulating; nested legs are the caller's business: none are nested here)."""
    t0 = time.perf_counter()
    try:
        yield
    finally:
        LEGS[name] = LEGS.get(name, 0.0) + time.perf_counter() - t0


PEAK_FP32_MFMA_TFLOPS = 157.3        # MI355X_MICROARCH.md "Peak FP32 (matrix)"
PEAK_BF16_MFMA_TFLOPS = 2500.0       # MI355X_MICROARCH.md "Peak BF16/FP16 MFMA" (dense)
# what pure MFMA chains sustain on RANDOM operands under the ~1 300 W the chip regulates to (tools/power_probe.sh,
# profiles/r02_power_probe.txt): the practical ceiling of an MFMA-bound kernel on real data; the f32 MFMA runs at full clock
SUSTAINED_MFMA_TFLOPS = {"f32": 157.3, "bf16x3": 1777.0, "fast": 1630.0}
PEAK_HBM_GBS = 8000.0                # HBM3E spec; 6290 GB/s is the measured float4-copy ceiling (same file)
FLOP_PER_EDGE = 2 * (17 * 150 + 3 * 150 * 150)   # F_min edge work: encoder 17->150->150->150 + W_rp[:, :150] block
PRECISIONS = {"f32": 0, "bf16x3": 1, "fast": 2}
DTYPE = {"f32": "f32 (exact fp32 MFMA)",
         "bf16x3": "f32 operands split hi+lo bf16, 3 bf16 MFMAs per product, f32 accumulate",
         "fast": "node stacks: f32 operands split hi+lo bf16, 3 bf16 MFMAs per product; edge stack: f16(W) x f16(x) on the f16 MFMA + "
                 "[e4m3(W_lo) | e4m3(W_hi)] x [e5m2(x) | e5m2(x - f16(x))] on the block-scaled fp8 MFMA (W and x to ~2^-15); f32 accumulate; "
                 "per-edge table, the senders' node terms and the per-node message sums 16-bit block-scaled fixed point (q16)"}
# fp16-MFMA-times issued per fp32 product in the edge stack: split-bf16 3; "fast": ten f16 MFMAs + five scaled fp8 MFMAs (K = 64, 1.25 f16-MFMA-times
# each under the power limit, tools/ubench/mx_mfma.hip) per 160 x 32 out-tile = 16.25 / 10
EDGE_PRODUCTS = {"f32": 1, "bf16x3": 3, "fast": 1.625}
DTYPE_TOKEN = {"f32": "f32", "bf16x3": "bf16x3", "fast": "f16+fp8corr+bf16x3"}
# <= 100 characters: the driver's record truncates longer config strings (the full description is the line's top-level "arithmetic")
ARITH_SHORT = {"f32": "exact fp32 MFMA", "bf16x3": "fp32 as hi+lo bf16, 3 MFMAs per product, f32 accumulate",
               "fast": "edge: f16 MFMA + scaled-fp8 corrections; node: bf16x3; Eterm/Hs/agg q16; f32 accumulate"}
assert all(len(v) <= 100 for v in ARITH_SHORT.values())
WORKLOADS = {"rope": dict(n_obj=1000, kw=dict(spacing=0.1)), "granular": dict(n_obj=2000, kw={}),
             "cloth": dict(n_obj=4096, kw={})}
PMC_FILE = os.path.join(ROOT, "profiles", "pmc_traffic.json")
MEASURED_STREAM_GBS = 5800.0      # 7:1 read:write streaming ubench on an MI355X box (profiles/r03_hbm_bw_ubench.txt), for context next to the 8 TB/s spec peak
DUMP_LIMIT_BYTES = 64 << 20       # --dump-outputs: at most this much in all


def host_threads():
    """CPU threads this process may use: its affinity mask, capped by OMP_NUM_THREADS when that is set (the oracle's OpenMP loop
    runs that many).  os.cpu_count() counts the whole host, which on a shared box can be many times what a job is given."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    try:
        omp = int(os.environ.get("OMP_NUM_THREADS", "0"))
    except ValueError:
        omp = 0
    return max(1, min(n, omp) if omp > 0 else n)


def capture_outputs(out):
    """Host copies (float32, or float64 where the engine returned float64) of what one pass returned, for --dump-outputs."""
    return {k: v.detach().cpu().numpy().astype(np.float64 if v.dtype == torch.float64 else np.float32) for k, v in out.items()}


def dump_outputs(outputs, d):
    """Write `outputs` as d/<name>.npy.  Over DUMP_LIMIT_BYTES in all, every array keeps the same rows of its batch axis: a sorted
    sample drawn with a fixed seed, so two runs with the same arguments write the same rows."""
    B = next(iter(outputs.values())).shape[0]
    per_row = sum(a.nbytes // max(a.shape[0], 1) for a in outputs.values())
    keep = max(1, min(B, DUMP_LIMIT_BYTES // max(per_row, 1)))
    rows = None if keep == B else np.sort(np.random.default_rng(0).choice(B, keep, replace=False))
    os.makedirs(d, exist_ok=True)
    for k, a in outputs.items():
        np.save(os.path.join(d, f"{k}.npy"), a if rows is None else a[rows])
    what = f"rows {keep} of {B} (seeded sample)" if rows is not None else f"all {B} rows"
    print(f"bench.py: wrote {', '.join(sorted(outputs))} to {d} ({what})", file=sys.stderr)


def csrc_sha():
    """sha256 over the kernel sources (the GPU box has no .git: hash the files themselves)."""
    d = os.path.join(ROOT, "adaptigraph_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()


def pmc_traffic(material, batch, precision, kernel):
    """HBM bytes per launch (FETCH_SIZE x2 per the gfx950 correction + WRITE_SIZE, tools/pmc_traffic.py) or None when the
    recorded passes were not collected from the sources being run."""
    try:
        rec = json.load(open(PMC_FILE))
    except (OSError, ValueError):
        return None, "profiles/pmc_traffic.json absent"
    if rec.get("csrc_sha256") != csrc_sha():
        return None, "profiles/pmc_traffic.json is stale (collected from other kernel sources)"
    v = rec.get("entries", {}).get(f"{material}/{batch}/{precision}/{kernel}")
    return (v, rec.get("source", "profiles/pmc_traffic.json")) if v is not None else (None, "workload not in profiles/pmc_traffic.json")


def cpu_baseline(weights, material, n_obj, kw, T=10, gpu_out=None):
    """Oracle ("port" of the reference algorithm: dense-formulation forward, O(N^2) edge build, per-step rebuild) on the SAME inputs as the timed
    GPU workload — the first `bsz` action samples of it, ONE graph per host thread (the oracle's OpenMP loop runs over graphs), all T rollout
    steps, once: ~3.3 s per model step on the 256-thread GPU-box host.  Because it is the same workload, its result is also the reference
    trajectory the engine's result is held against: `drift` = max |engine - oracle| over those samples after the T steps, per arithmetic mode
    (`gpu_out`: mode -> engine state_seqs as numpy) — per STEP on identical graphs the deviation is <= 1e-5 (tests); over a rollout a top-k
    near-tie can pick another neighbour and the trajectories part (profiles/r05_rollout_drift.txt), which is what this number shows.
    A host with few threads runs fewer samples and, below 16 threads, fewer steps (then no drift is reported); the threads counted are the ones
    this process may use (host_threads()), so the leg takes about T x 3.3 s wherever it runs."""
    from oracle import ag_oracle as ago
    os.environ.setdefault("OMP_WAIT_POLICY", "passive")      # idle OpenMP threads sleep instead of spinning beside torch's own pool
    cores = host_threads()
    B = 256
    bsz = max(1, min(cores, B))
    steps = T if cores >= 16 else 2
    state, act = synth.make_mpc_inputs(material, n_obj, B, seed=0, len_lo=steps, len_hi=steps + 0.9, **kw)
    act = act[:bsz]
    task = configs.task_config(material)
    ago.lib()
    t0 = time.perf_counter()
    seq, _ = ago.dynamics(weights, task, state, act)
    dt = time.perf_counter() - t0
    res = {"value": bsz * steps / dt, "unit": "graph-steps/s", "cores": min(cores, bsz), "host_threads": cores, "kind": "port",
           "sample": f"{material} n_obj={n_obj}: the first {bsz} of the timed workload's 256 action samples (one graph per host thread), the full "
                     f"{steps}-step rollout, once ({dt:.1f} s), OpenMP over graphs: {min(cores, bsz)} of {cores} host threads busy"}
    if gpu_out and steps == T:
        dev = {k: np.abs(v[:bsz] - seq[:, 0]) for k, v in gpu_out.items() if v is not None and v.shape[0] >= bsz}
        res["drift"] = {k: float(d.max()) for k, d in dev.items()}
        # the maximum is ONE coordinate: a near-tie that parts two trajectories moves a few particles by 1e-3 .. 1e-2 whatever the arithmetic (the exact-fp32
        # mode shows the same); the median and the share of coordinates beyond the one-step gate say how the rest of the rollout compares
        res["drift_median"] = {k: float(np.median(d)) for k, d in dev.items()}
        res["drift_frac_over_1e-4"] = {k: float((d > 1e-4).mean()) for k, d in dev.items()}
        # engine against engine: where the default mode and the exact-fp32 mode take the same side of every near-tie, their trajectories stay together
        if "f32" in dev and all(gpu_out.get(k) is not None for k in ("fast", "f32")):
            res["drift_fast_vs_f32_engine"] = float(np.abs(gpu_out["fast"][:bsz] - gpu_out["f32"][:bsz]).max())
        res["drift_note"] = (f"max |engine - oracle| of the predicted positions after the {T}-step rollout over those {bsz} samples; one-step deviation on "
                             "identical graphs is <= 1e-5 (gate 1e-4, tests/test_gpu_parity.py): larger values are top-k near-ties resolved differently")
    return res


def cpu_baseline_dense(weights, material, n_obj, kw, seconds_budget=8.0):
    """the reference's FORMULATION on the host cores — dense one-hot Rr/Rs and `bmm` gathers in PyTorch-CPU
    (oracle/torch_dense.py restates model.py:129-313), per step a radius-graph rebuild (the C oracle's O(N^2) builder, expanded
    to one-hots as graph.py:152-155 returns them) + forward + state shift.  Bounded sample: the batch the one-hots let fit."""
    from oracle import ag_oracle as ago
    from oracle.torch_dense import dense_forward, one_hots
    cores = host_threads()
    mm = synth.MATERIALS[material]
    bsz = 4 if n_obj <= 1000 else 1
    g = synth.make_graph_inputs(material, n_obj, bsz, seed=0, **kw)
    from adaptigraph_amd.model import _MLP3, _Lin, _Dec
    model = torch.nn.Module()                                     # the reference's parameter containers only: nothing of the engine, nothing on a GPU
    model.particle_encoder, model.relation_encoder = _MLP3(6, 150, 150), _MLP3(17, 150, 150)
    model.particle_propagator, model.relation_propagator, model.non_rigid_predictor = _Lin(300, 150), _Lin(450, 150), _Dec(150, 150, 3)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    state, attrs, action, p_inst, phys = (t(g[k]) for k in ("state", "attrs", "action", "p_instance", "phys"))
    N, steps = attrs.shape[1], 2

    def rollout_once():
        st = state.clone()
        for _ in range(steps):
            n_rel, recv, send = ago.build_edges(st[:, -1].numpy(), mm["radius"], g["mask"], g["tool_mask"], mm["topk"], mm["connect_tools_all"], "batch")
            Rr, Rs = one_hots(n_rel, recv, send, N)
            pos, _ = dense_forward(model, st, attrs, Rr, Rs, p_inst, action, phys)
            cur = st[:, -1].clone()
            cur[:, :pos.shape[1]] = pos
            st = torch.cat([st[:, 1:], cur[:, None]], 1)

    # torch's CPU bmm at this size does not scale past a few dozen threads (measured on the 256-thread GPU-box host: 15.6
    # graph-steps/s at 16 threads, 9.0 at 64, 0.3 at 256), so the thread count is swept and the best one is what is reported
    best, sweep = None, {}
    with torch.no_grad():
        for th in sorted({min(cores, c) for c in (8, 16, 32)}):
            torch.set_num_threads(th)
            rollout_once()                                   # warm-up (thread pool, allocator)
            t0 = time.perf_counter()
            rollout_once()
            sweep[th] = bsz * steps / (time.perf_counter() - t0)
            if best is None or sweep[th] > sweep[best]:
                best = th
        torch.set_num_threads(best)
        t0, reps = time.perf_counter(), 0
        while True:
            rollout_once()
            reps += 1
            dt = time.perf_counter() - t0
            if dt > seconds_budget * 0.5:
                break
    return {"value": bsz * steps * reps / dt, "unit": "graph-steps/s", "cores": best, "host_threads": cores, "kind": "port",
            "formulation": "dense one-hot Rr/Rs + bmm in PyTorch-CPU (the reference's formulation, model.py:129-313)",
            "thread_sweep": {str(k): round(v, 2) for k, v in sweep.items()},
            "sample": f"{material} n_obj={n_obj}, batch {bsz}, {steps}-step rollout x {reps} reps ({dt:.1f} s), torch.set_num_threads({best}) "
                      f"(best of the sweep; the host has {cores} threads)"}


class Engine:
    """One model + one workload on this rank's GPU; `run()` times `steps` passes of dynamics()."""

    def __init__(self, material, weights, dev, world):
        self.material, self.dev, self.world = material, dev, world
        self.model = DynamicsPredictor(configs.model_config(), configs.material_config(material),
                                       configs.dataset_config(material), dev)
        self.model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
        self.model = self.model.to(dev).eval()
        self.ppm = configs.ppm_optimizer_stub(material)
        self.ppm.physics_param = {material: torch.tensor([0.5], device=dev)}
        self.L = _lib.lib()
        self.h = self.model.handle(torch.device(dev))

    def opt(self, name, value):
        _lib.check(self.L.ag_set_option(self.h, name.encode(), int(value)), f"ag_set_option({name})")

    def get(self, name):
        """The model's CURRENT value of an engine option (ag_get_option: what the library runs with, whatever set it — default, environment, ag_set_option)."""
        v = ctypes.c_int()
        _lib.check(self.L.ag_get_option(self.h, name.encode(), ctypes.byref(v)), f"ag_get_option({name})")
        return int(v.value)

    def sync(self):
        torch.cuda.synchronize()
        if self.world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def run(self, batch, T, precision, streams, steps, warmup, profile=True, global_batch=None, tag="main", keep=False, dump=False):
        """`batch` graphs per GPU (weak scaling) or, with `global_batch`, that many graphs split over the ranks (strong scaling:
        BASELINE configs[3] = cloth batch 512 over 8 GPUs).  `tag`: name of this run's wall-clock legs; `keep`: return the predicted states
        (numpy) so that the CPU leg can hold them against the oracle's rollout of the same inputs; `dump`: return host copies of everything
        the last timed pass returned (`outputs`, for --dump-outputs)."""
        if tag == "main":          # the headline run is split into its own legs (set-up, warm-up, timed, roofline pass)
            return self._run(batch, T, precision, streams, steps, warmup, profile, global_batch, tag, keep, dump)
        with leg(tag):
            return self._run(batch, T, precision, streams, steps, warmup, profile, global_batch, tag, keep, dump)

    def _run(self, batch, T, precision, streams, steps, warmup, profile, global_batch, tag, keep, dump=False):
        wl = WORKLOADS[self.material]
        sub = (lambda n: leg(f"main_{n}")) if tag == "main" else (lambda n: contextlib.nullcontext())
        B_global = batch * self.world if global_batch is None else global_batch
        batch = -(-B_global // self.world)
        with sub("setup"):
            state_np, act_np = synth.make_mpc_inputs(self.material, wl["n_obj"], B_global, seed=0, len_lo=T, len_hi=T + 0.9, **wl["kw"])
            state = torch.from_numpy(state_np).to(self.dev)           # inputs resident in HBM before the timed region
            action = torch.from_numpy(act_np).to(self.dev)
        timing = {} if self.world > 1 else None

        def one_pass(tm=None):
            # copy=False: the gathered states are consumed before the next pass, so the receive buffer is returned as is
            return agdist.dynamics_sharded(dynamics, state, action, self.model, self.dev, self.ppm, timing=tm, copy=False)

        self.opt("precision", PRECISIONS[precision])
        self.opt("rollout_streams", streams)
        with sub("warmup"):          # (the first pass also sizes the workspace and loads the code objects)
            for _ in range(warmup):
                out = one_pass()
            self.sync()
        # the model's sticky numeric status (ag_model_status) is read-and-cleared by every dynamics() call: OR what those reads see, so the
        # line says whether ANY timed pass left the arithmetic's range (the final read below covers the last pass)
        status, take = [int(self.model.take_status())], self.model.take_status

        def recording_take(device=None):
            v = take(device)
            status[0] |= int(v)
            return v

        self.model.take_status = recording_take
        t0 = time.perf_counter()
        for _ in range(steps):
            out = one_pass(timing)
        self.sync()
        dt = time.perf_counter() - t0
        if tag == "main":
            LEGS["main_timed"] = dt
        self.model.take_status = take
        status[0] |= int(self.model.take_status())
        assert out["state_seqs"].shape == (B_global, 1, wl["n_obj"], 3) and bool(torch.isfinite(out["state_seqs"]).all())
        outputs = capture_outputs(out) if dump else None      # before the roofline pass: with copy=False it reuses the gather buffers
        mm = synth.MATERIALS[self.material]
        prm = _lib.RolloutParams(batch, wl["n_obj"] + mm["n_tools"], wl["n_obj"], 1, mm["topk"], 1 if mm["connect_tools_all"] else 0, mm["n_tools"], T, 0, 0.0)
        res = {"B_global": B_global, "dt": dt, "ms_per_step": dt / steps * 1e3, "value": B_global * T * steps / dt,
               "streams": int(self.L.ag_rollout_streams_for(self.h, ctypes.byref(prm))), "timed_s": dt,
               "roofline": None, "roofline_hbm": None, "kernels": None, "model_status": status[0],
               "out": out["state_seqs"][:, 0].cpu().numpy() if keep else None, "outputs": outputs}
        if timing:
            res["rank_ms"] = (agdist.elapsed_ms(timing["rollout"]) / steps, agdist.elapsed_ms(timing["gather"]) / steps)
        if profile:
            with sub("roofline"):
                res.update(self.roofline_pass(one_pass, batch, precision, streams, min(3, max(1, steps))))
        return res

    def roofline_pass(self, one_pass, batch, precision, streams, n_prof):
        """The same workload with the rollout on ONE stream (outside the timed region), so every kernel has the GPU to
        itself and a launch duration means what a roofline needs it to mean; HIP events recorded by the library on the
        launch stream around every launch (ag_profile_*)."""
        L, h = self.L, self.h
        self.opt("rollout_streams", 1)
        one_pass()
        _lib.check(L.ag_profile_enable(h, 1), "ag_profile_enable")
        for _ in range(n_prof):
            one_pass()
        ms = (ctypes.c_double * 6)()
        cnt = (ctypes.c_int64 * 6)()
        edges = ctypes.c_int64()
        _lib.check(L.ag_profile_read(h, ms, cnt, ctypes.byref(edges)), "ag_profile_read")
        _lib.check(L.ag_profile_enable(h, 0), "ag_profile_enable")
        self.opt("rollout_streams", streams)
        kernels = {name: {"ms_per_launch": ms[i] / max(int(cnt[i]), 1), "launches": int(cnt[i])}
                   for i, name in enumerate(_lib.KERNEL_CLASSES)}
        roof = roof_hbm = None
        k = _lib.KERNEL_CLASSES.index("edge_encode")
        if cnt[k] > 0 and ms[k] > 0:
            avg_s = ms[k] / cnt[k] * 1e-3
            e_per = edges.value / cnt[k]
            b3 = precision != "f32"
            peak = PEAK_BF16_MFMA_TFLOPS if b3 else PEAK_FP32_MFMA_TFLOPS
            achieved = FLOP_PER_EDGE * e_per / avg_s / 1e12           # algorithmic (F_min) FLOP only
            traffic, src = pmc_traffic(self.material, batch, precision, "edge_encode")
            kname = {"f32": "edge_encode_kernel<PrecF32>", "bf16x3": "edge_encode_kernel<PrecB3>",
                     "fast": "edge_encode_ws_kernel"}[precision]       # (its per-node input rows ride the edge builder's launches since r05: class build_edges)
            roof = {"bound": "mfma", "kernel": kname, "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
                    "frac": achieved / peak, "traffic": traffic, "traffic_source": src,
                    "mfma_issue_util": EDGE_PRODUCTS[precision] * achieved / peak,
                    "sustained_peak_measured": SUSTAINED_MFMA_TFLOPS[precision],
                    "issue_frac_of_sustained": EDGE_PRODUCTS[precision] * achieved / SUSTAINED_MFMA_TFLOPS[precision],
                    "algorithmic_bytes": e_per * ((320 if precision == "fast" else 640) + 68),
                    "avg_launch_ms": ms[k] / cnt[k], "edges_per_launch": e_per, "flop_per_edge": FLOP_PER_EDGE,
                    "mfma": {"f32": "v_mfma_f32_32x32x2_f32", "bf16x3": "v_mfma_f32_32x32x16_bf16, 3 per fp32 product (hi*hi + hi*lo + lo*hi)",
                             "fast": "10 x v_mfma_f32_32x32x16_f16 (f16(W).f16(x)) + 5 x v_mfma_scale_f32_32x32x64_f8f6f4 (corrections) per out-tile"}[precision],
                    "measured": f"HIP events on the launch stream, {n_prof} single-stream passes after the timed region"}
            ka = _lib.KERNEL_CLASSES.index("aggregate")
            if cnt[ka] > 0 and ms[ka] > 0:
                # segment reduce: Eterm streamed once (640 B/edge fp32, 320 B f16), Hs rows gathered (first touch from
                # HBM once per node, then L2), Hr read + agg written per node (SURVEY §8d B_alg terms)
                n_nodes = batch * (WORKLOADS[self.material]["n_obj"] + synth.MATERIALS[self.material]["n_tools"])
                # node tables per launch: Hr read + Hs first-touch + agg write = 3 x 640 B per node; with the node encoder de-duplicated
                # (default) round 0 reads Hr / Hs from a few compact rows, so the three rounds average (1 + 3 + 3) / 3 tables.  In the default
                # mode the rounds after the first gather Hs from q16 rows (320 B per node): 2.5 tables there
                # (r06, option agg_q16, the default mode's default: `agg` leaves as q16 rows too: 320 B per node)
                aggw = 0.5 if (precision == "fast" and self.get("agg_q16")) else 1.0
                later = 1.5 + aggw if precision == "fast" else 3.0
                tables = (2.0 + aggw + 2 * later) / 3.0 if self.get("node_dedup") == 0 else (aggw + 2 * later) / 3.0
                nbytes = e_per * (320 if precision == "fast" else 640) + n_nodes * tables * 640
                a_s = ms[ka] / cnt[ka] * 1e-3
                t2, src2 = pmc_traffic(self.material, batch, precision, "aggregate")
                roof_hbm = {"bound": "hbm", "kernel": "aggregate_half_kernel" if precision == "fast" else "aggregate_kernel", "achieved": nbytes / a_s / 1e9, "peak": PEAK_HBM_GBS,
                            "unit": "GB/s", "frac": nbytes / a_s / 1e9 / PEAK_HBM_GBS, "traffic": t2, "traffic_source": src2,
                            "avg_launch_ms": ms[ka] / cnt[ka], "bytes_per_launch": nbytes, "node_tables_per_launch": tables,
                            # what a plain 7 : 1 read : write float4 streaming loop reaches on this kind of box (tools/ubench/hbm_bw.hip,
                            # profiles/r03_hbm_bw_ubench.txt: 5.6-6.0 TB/s; read-only 5.3-5.6, copy 4.5-5.3)
                            "stream_ceiling_measured": MEASURED_STREAM_GBS, "frac_of_stream_ceiling": nbytes / a_s / 1e9 / MEASURED_STREAM_GBS}
        return {"roofline": roof, "roofline_hbm": roof_hbm, "kernels": kernels}


def stub_dynamics(state, action, *_args, **_kw):
    """--dry-run stand-in for the engine (CPU, no GPU needed): the result depends only on the sample's action, so the sharded / gathered
    result can be checked against the unsharded call (tests/test_host_logic.py)."""
    seq = action[:, :, :3].sum(-1)[:, :, None, None] + state[None, None]
    return {"state_seqs": seq.float(), "action_seqs": action * 2.0}


class DryEngine(Engine):
    """bench.py --dry-run: everything of an N-rank run EXCEPT the engine — process group (gloo, CPU tensors), batch sharding, the all-gather,
    the max-over-ranks timing and the JSON line — so the launch line, argument and key contract of the SCALE run can be exercised without
    GPUs.  Its numbers mean nothing and the line says so ("data": "dry-run")."""

    def __init__(self, material, dev, world):
        self.material, self.dev, self.world = material, dev, world

    def opt(self, name, value):
        pass

    def sync(self):
        if self.world > 1:
            dist.barrier()

    def run(self, batch, T, precision, streams, steps, warmup, profile=True, global_batch=None, tag="main", keep=False, dump=False):
        wl = WORKLOADS[self.material]
        B_global = batch * self.world if global_batch is None else global_batch
        state_np, act_np = synth.make_mpc_inputs(self.material, wl["n_obj"], B_global, seed=0, len_lo=T, len_hi=T + 0.9, **wl["kw"])
        state, action = torch.from_numpy(state_np), torch.from_numpy(act_np)
        t_roll = t_gather = 0.0
        self.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            a = time.perf_counter()
            out = agdist.dynamics_sharded(stub_dynamics, state, action, copy=False)
            t_roll += time.perf_counter() - a
        self.sync()
        dt = time.perf_counter() - t0
        full = stub_dynamics(state, action)
        assert out["state_seqs"].shape == (B_global, 1, wl["n_obj"], 3) and torch.equal(out["state_seqs"], full["state_seqs"])
        return {"B_global": B_global, "dt": dt, "ms_per_step": dt / steps * 1e3, "value": B_global * T * steps / dt, "roofline": None,
                "roofline_hbm": None, "kernels": None, "model_status": 0, "rank_ms": (t_roll / steps * 1e3, t_gather / steps * 1e3),
                "outputs": capture_outputs(out) if dump else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--material", default="rope", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=256, help="action samples (graphs) per GPU (weak scaling: the default)")
    ap.add_argument("--global-batch", type=int, default=None,
                    help="total graphs, split over the ranks (strong scaling), e.g. --material cloth --global-batch 512 --rollout-steps 20 "
                         "= BASELINE configs[3]; overrides --batch")
    ap.add_argument("--weights", default="seed0", help="seed0 (reference default init) or a trained set of tools/gen_trained.py, e.g. trained_rope")
    ap.add_argument("--rollout-steps", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: the per-kernel roofline pass, the extra workloads and the CPU baselines "
                         "(a plain run only sets up, warms up, times --steps passes and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed pass returned as DIR/<name>.npy (float32; at most 64 MB, a seeded sample of the batch beyond)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-profile", action="store_true", help="with --full: skip the per-kernel HIP-event roofline pass")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the extra workloads (f32 mode, granular-2k, cloth-4k)")
    ap.add_argument("--precision", default="fast", choices=sorted(PRECISIONS),
                    help="engine arithmetic mode: f32 = exact fp32 MFMA, bf16x3 = split-bf16, fast (default) = bf16x3 node stacks + fp16 edge stack "
                         "with fp8 corrections + q16 table; all three hold the 1e-4 gate at any motion size with model_status 0 "
                         "(tests/test_gpu_parity.py, tools/fuzz_parity.py)")
    ap.add_argument("--streams", type=int, default=0, help="rollout batch parts on separate streams (0 = the engine's choice by workload, its default)")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU, no engine: process group on gloo with CPU tensors, sharding, all-gather, timing reduction and the JSON line only "
                         "(launch-line / key contract of the multi-GPU run; the numbers are meaningless)")
    ap.add_argument("--cu-split", type=int, default=None,
                    help="CUs (multiple of 8) of the MFMA partition of the CU-partitioned rollout, 0 = off (default: the engine's own choice)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full:
        args.no_profile = args.no_extra = args.no_cpu_baseline = True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if args.dry_run:
        dev = "cpu"
        args.no_profile = args.no_extra = args.no_cpu_baseline = True
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo")
    else:
        assert torch.cuda.is_available(), "bench.py needs MI355X GPUs (the engine has no CPU fallback)"
        local %= max(1, torch.cuda.device_count())       # (a box with fewer GPUs than ranks — the 2-rank test on one GPU — wraps around)
        torch.cuda.set_device(local)
        dev = f"cuda:{local}"
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            backend = os.environ.get("AG_DIST_BACKEND", "nccl")             # "nccl" is RCCL on ROCm; tests on a 1-GPU box use "gloo"
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=torch.device(dev))
            else:
                dist.init_process_group(backend)

    LEGS["process_group"] = time.perf_counter() - _T_START - LEGS["import"]
    weights = dict(np.load(os.path.join(ROOT, "tests", "golden", f"weights_{args.weights}.npz")))
    with leg("engine_build"):      # library load + weight packing + the first HIP context on this process
        eng = DryEngine(args.material, dev, world) if args.dry_run else Engine(args.material, weights, dev, world)
        if args.cu_split is not None:
            eng.opt("cu_split", args.cu_split)
    T = args.rollout_steps
    want_drift = world == 1 and not args.no_cpu_baseline and not args.dry_run and args.global_batch is None and args.batch == 256
    r = eng.run(args.batch, T, args.precision, args.streams, args.steps, args.warmup, profile=not args.no_profile,
                global_batch=args.global_batch, keep=want_drift, dump=args.dump_outputs is not None and rank == 0)
    if r["outputs"] is not None:
        dump_outputs(r.pop("outputs"), args.dump_outputs)
    gpu_out = {args.precision: r.get("out")}
    per_gpu = -(-r["B_global"] // world)

    tmax = torch.tensor([r["dt"]], dtype=torch.float64, device=dev)
    ranks = None
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        mine = torch.tensor([r["ms_per_step"], r["rank_ms"][0], r["rank_ms"][1]], dtype=torch.float64, device=dev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        tab = torch.stack(allr).cpu().numpy()
        ranks = {"ms_per_step": {"min": float(tab[:, 0].min()), "max": float(tab[:, 0].max())},
                 "rollout_ms": {"min": float(tab[:, 1].min()), "max": float(tab[:, 1].max())},
                 "all_gather_ms": {"min": float(tab[:, 2].min()), "max": float(tab[:, 2].max())},
                 "note": "per step; rollout/all_gather from CUDA events around the local rollout and the collective"}
        # first-contact record: did the collective library see N ranks, each on its own device?
        devs = [None] * world
        dist.all_gather_object(devs, {"rank": rank, "local_rank": local, "device": None if args.dry_run else torch.cuda.current_device(),
                                      "device_name": None if args.dry_run else torch.cuda.get_device_name(), "pid": os.getpid()})
        nccl_v = None
        try:
            nccl_v = ".".join(map(str, torch.cuda.nccl.version())) if not args.dry_run else None
        except Exception as e:      # noqa: BLE001
            nccl_v = repr(e)
        ranks["rccl"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "nccl_version": nccl_v,
                         "devices": devs, "distinct_devices": len({d["device"] for d in devs}),
                         "visible_gpus": 0 if args.dry_run else torch.cuda.device_count()}
    dt = float(tmax.item())

    extra = None
    if world == 1 and not args.no_extra and args.material == "rope":
        extra = {}
        if args.precision != "f32":
            e = eng.run(args.batch, T, "f32", args.streams, max(2, args.steps // 2), 1, profile=not args.no_profile, tag="f32", keep=want_drift)
            gpu_out["f32"] = e.get("out")
            extra["f32_mode"] = {"value": e["value"], "unit": "graph-steps/s", "ms_per_step": e["ms_per_step"], "model_status": e["model_status"],
                                 "arithmetic": DTYPE["f32"], "roofline": e["roofline"],
                                 "note": "same workload, ag_set_option(precision, 0): the mode that matches every reference rollout golden"}
        if args.precision == "fast":      # the middle mode: split-bf16 everywhere, fp32 per-edge table
            e = eng.run(args.batch, T, "bf16x3", args.streams, max(2, args.steps // 2), 1, profile=False, tag="bf16x3", keep=want_drift)
            gpu_out["bf16x3"] = e.get("out")
            extra["bf16x3_mode"] = {"value": e["value"], "unit": "graph-steps/s", "ms_per_step": e["ms_per_step"], "arithmetic": DTYPE["bf16x3"],
                                    "model_status": e["model_status"],
                                    "note": "same workload, ag_set_option(precision, 1)"}
        if not args.no_profile:       # the SAME workload with ag_set_option("shared_state", 1): reported beside the headline, never as it (the headline is full per-sample work)
            eng.opt("shared_state", 1)
            e = eng.run(args.batch, T, args.precision, args.streams, max(2, args.steps // 2), 1, profile=True, tag="shared_state", keep=want_drift)
            eng.opt("shared_state", 0)
            ke = e["roofline"]["edges_per_launch"] if e["roofline"] else None
            extra["shared_state"] = {"value": e["value"], "unit": "graph-steps/s", "ms_per_step": e["ms_per_step"], "model_status": e["model_status"],
                                     "edges_per_model_step": ke, "plain_edges_per_model_step": r["roofline"]["edges_per_launch"] if r["roofline"] else None,
                                     "equal_to_plain": bool(want_drift and np.array_equal(e["out"], r["out"])) if want_drift else None, "kernels": e["kernels"],
                                     "note": "ag_set_option(shared_state, 1): dynamics() rolls ONE cloud out under all action samples; the tool-less base trajectory "
                                             "is computed once and per sample only the rows that can differ from it; bit-identical results (equal_to_plain)"}
        if args.weights == "seed0":       # throughput does not depend on the weights; the numeric status must stay clean on trained ones too
            with leg("trained"):
                et = Engine(args.material, dict(np.load(os.path.join(ROOT, "tests", "golden", "weights_trained_rope.npz"))), dev, world)
            x = et.run(args.batch, T, args.precision, args.streams, max(2, args.steps // 2), 1, profile=False, tag="trained")
            extra["trained_weights"] = {"value": x["value"], "unit": "graph-steps/s", "ms_per_step": x["ms_per_step"], "precision": args.precision,
                                        "weights": "trained_rope (the reference's train() on a toy dataset, tools/gen_trained.py)",
                                        "model_status": x["model_status"]}
            del et
        extra["workloads"] = {}
        for mat, b, t, tag in (("granular", 128, 10, "BASELINE configs[2]"), ("cloth", 64, 20, "BASELINE configs[3], per-GPU share of batch 512 on 8 GPUs")):
            with leg(mat):
                e2 = Engine(mat, weights, dev, world)
            x = e2.run(b, t, args.precision, args.streams, 3, 1, profile=not args.no_profile, tag=mat)
            extra["workloads"][mat] = {"workload": f"{mat} {WORKLOADS[mat]['n_obj']} particles, batch {b}, {t}-step rollout ({tag})",
                                       "value": x["value"], "unit": "graph-steps/s", "ms_per_step": x["ms_per_step"], "model_status": x["model_status"],
                                       "precision": args.precision, "kernels": x["kernels"], "roofline": x["roofline"],
                                       "roofline_hbm": x["roofline_hbm"]}
            del e2

        try:        # BASELINE configs[4] on one GPU: per-iteration wall-clock of the MPPI loop (bench_mpc.py measures it at N GPUs)
            import bench_mpc
            with leg("mpc"):
                ms_full, r_full = bench_mpc.mppi_bench(torch.device(dev), 1000, 1024, 15, steps=3, warmup=1, precision=args.precision, shared_state=0)
                ms_it, r_sh = bench_mpc.mppi_bench(torch.device(dev), 1000, 1024, 15, steps=3, warmup=1, precision=args.precision, shared_state=1)
            extra["mpc"] = {"workload": "MPPI iteration: 1024 sampled pushes x 15-step rollout on rope-1000, chamfer + penalty cost, softmax update "
                                        "(BASELINE configs[4], 1 GPU)", "value": ms_it, "unit": "ms per iteration", "higher_is_better": False,
                            "graph_steps_per_s": 1024 * 15 / ms_it * 1e3, "precision": args.precision,
                            "engine_option": "shared_state 1: the 1024 pushes roll ONE cloud out — the tool-less base trajectory once, per sample only the rows that "
                                             "can differ from it (bit-identical to the plain rollout: rewards_equal below)",
                            "plain_rollout_ms": ms_full, "rewards_equal": bool(torch.equal(r_full, r_sh))}
        except Exception as e:      # noqa: BLE001
            extra["mpc"] = {"error": repr(e)}

    if rank == 0:
        wl = WORKLOADS[args.material]
        line = {
            "metric": "rollout graph-steps/s (batch x rollout steps / wall; edge build + GNN forward + state update per graph-step)",
            "value": r["B_global"] * T * args.steps / dt, "unit": "graph-steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak" if args.global_batch is None else "strong",
            "vs_baseline": None, "dtype": DTYPE_TOKEN[args.precision], "data": "dry-run (no engine: contract check only)" if args.dry_run else "synthetic",
            "config": {"workload": f"{args.material} {wl['n_obj']}+tool particles, batch {per_gpu}/GPU, "
                                   f"{T}-step rollout (BASELINE configs[1])" if args.material == "rope" else
                                   f"{args.material} {wl['n_obj']} particles, batch {per_gpu}/GPU"
                                   + (f" (global batch {r['B_global']} over {world} GPUs)" if args.global_batch else "") + f", {T}-step rollout",
                       "global_batch": r["B_global"], "rollout_steps": T, "parallelism": f"batch-shard x{world} + all-gather",
                       "rollout_streams": r.get("streams", args.streams), "weights": "seed-0 random init (reference default init)" if args.weights == "seed0" else
                                  f"{args.weights} (the reference's train() on a toy dataset, tools/gen_trained.py)",
                       "precision": args.precision, "arithmetic": ARITH_SHORT[args.precision],
                       # 0 = no timed pass left the arithmetic's range (include/adaptigraph_hip.h: ag_model_status)
                       "model_status": r["model_status"],
                       # engine options the timed region ran with (ag_get_option): self-loops as one table row per attribute class (exact, r06);
                       # shared_state 0 = every sample computed in full (the option's numbers are the separate shared_state_* / mpc_ms keys)
                       "self_edges": -1 if args.dry_run else eng.get("self_edges"), "shared_state": -1 if args.dry_run else eng.get("shared_state"),
                       "agg_q16": -1 if args.dry_run else eng.get("agg_q16")},
            "arithmetic": DTYPE[args.precision],
            "roofline": r["roofline"], "roofline_hbm": r["roofline_hbm"], "kernels": r["kernels"],
        }
        if extra:       # the driver's record keeps the SCALAR keys of `config` only (nested dicts and `extra` are dropped, long strings cut):
            cfg = line["config"]                                   # per-mode throughputs and statuses of the same workload as flat numbers
            for key, name in (("f32_mode", "f32"), ("bf16x3_mode", "bf16x3"), ("trained_weights", "trained")):
                if key in extra:
                    cfg[f"{name}_value"] = round(extra[key]["value"], 1)
                    cfg[f"{name}_status"] = extra[key]["model_status"]
            for mat, v in extra.get("workloads", {}).items():
                cfg[f"{mat}_value"] = round(v["value"], 1)
                cfg[f"{mat}_status"] = v["model_status"]
            if "value" in extra.get("mpc", {}):
                cfg["mpc_ms"] = round(extra["mpc"]["value"], 2)                       # with the shared-state rollout (bit-identical)
                cfg["mpc_plain_ms"] = round(extra["mpc"]["plain_rollout_ms"], 2)      # every sample in full (r05: 105.7)
                cfg["mpc_rewards_equal"] = extra["mpc"]["rewards_equal"]
            if "shared_state" in extra:
                cfg["shared_state_value"] = round(extra["shared_state"]["value"], 1)
                cfg["shared_state_edges_per_step"] = extra["shared_state"]["edges_per_model_step"]
                cfg["plain_edges_per_step"] = extra["shared_state"]["plain_edges_per_model_step"]
        if ranks:
            line["ranks"] = ranks
        if extra:
            line["extra"] = extra
        if not args.no_cpu_baseline and world == 1:
            with leg("cpu_port"):
                line["cpu_baseline"] = cpu_baseline(weights, args.material, wl["n_obj"], wl["kw"], T, gpu_out if want_drift else None)
            line["gpu_over_cpu"] = line["value"] / line["cpu_baseline"]["value"]
            for mode, d in line["cpu_baseline"].get("drift", {}).items():      # flat keys the driver's record keeps (VERDICT r05 weak #1a)
                line["config"][f"{mode}_drift"] = float(f"{d:.3g}")
            for mode, d in line["cpu_baseline"].get("drift_frac_over_1e-4", {}).items():
                line["config"][f"{mode}_drift_frac_over_gate"] = float(f"{d:.3g}")
            if "drift_fast_vs_f32_engine" in line["cpu_baseline"]:
                line["config"]["fast_vs_f32_engine_drift"] = float(f"{line['cpu_baseline']['drift_fast_vs_f32_engine']:.3g}")
            try:        # second baseline object: the reference's dense formulation (slower than the sparse port above, so the headline ratio stays conservative)
                with leg("cpu_dense"):
                    line["cpu_baseline_dense_bmm"] = cpu_baseline_dense(weights, args.material, wl["n_obj"], wl["kw"])
            except Exception as e:      # noqa: BLE001 — a baseline leg must never lose the measured line
                line["cpu_baseline_dense_bmm"] = {"error": repr(e)}
        LEGS["total"] = time.perf_counter() - _T_START
        line["legs_s"] = {k: round(v, 2) for k, v in LEGS.items()}
        line["config"]["bench_wall_s"] = round(LEGS["total"], 1)
        print(json.dumps(line))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
