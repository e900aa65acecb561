"""The inference engine at the configurations its code branches on — `pstep` (first round = last round, no middle round, several middle rounds, odd
and even buffer swaps), `phys_dim` 0 / 1 / 2 (the columns of the narrow first layer, the row the classifier compares, phys = NULL), `n_instance` 0 / 1 /
2 / 3 (the instance loops of the edge encoder, the weight-stationary edge encoder switched off) — and through the life of its weights after
ag_model_create (ag_model_update_weights, the fp16-range fallback of the edge stack, edits the version counter does not see).

Whole forwards and rollouts against the float64 restatement of the step (tests/test_grad_rollout.py `_step64`), at the tolerances of
tests/test_gpu_parity.py; kernel choices, drivers and repacked weights against each other bit for bit.  The references are computed once per
(shape, configuration, weight set) and shared by every test that needs them; nothing writes to them."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rescale_edge_stack
from adaptigraph_amd import _lib, configs, synth
from adaptigraph_amd import graph as aggraph
from adaptigraph_amd.forward_dynamics import rollout
from oracle import ag_oracle as ago
from test_gpu_parity import DEV, PRECISIONS, TOL_BY_PREC, TOL_FWD, csr_from_lists, t
from test_grad_rollout import _lin, _mlp, _step64
from test_scripted_rollout import inputs as scripted_inputs, scripted, step_loop

#          (phys_dim, n_instance, pstep)
CONFIGS = [(1, 1, 1), (1, 1, 2), (1, 1, 4), (1, 1, 5), (0, 1, 3), (2, 1, 3), (1, 0, 3), (1, 2, 3), (1, 3, 3), (0, 0, 1), (2, 3, 4), (2, 2, 2)]
ROLLOUT_CONFIGS = [(1, 1, 1), (1, 1, 2), (1, 1, 4), (0, 1, 3), (2, 2, 3), (1, 0, 2)]
SCRIPTED_CONFIGS = [(1, 1, 1), (1, 1, 4), (2, 2, 3)]
WEIGHT_SETS = ("weights_seed0", "weights_trained_rope")
SHAPES = {"rope93": (93, 3, 7), "rope300": (300, 2, 0), "rope150x5": (150, 5, 0), "rope300x5": (300, 5, 0)}      # objects, samples, padded slots
RADIUS, TOPK = synth.MATERIALS["rope"]["radius"], synth.MATERIALS["rope"]["topk"]
W0 = "particle_encoder.model.0.weight"      # (F, attr 2 | phys | action 3): the physics column(s) start at 2
TOL_REFS = 1e-6        # the fp32 oracle against the float64 step: 1 / 20 of the tightest engine tolerance


def cfg_id(c):
    return "phys%d-inst%d-pstep%d" % c


# ------------------------------------------------------------------------------------------------------ weights, model, inputs, reference
@functools.lru_cache(maxsize=None)
def weights_np(name, phys_dim):
    """A golden weight set with the first node layer cut or widened to `phys_dim` physics columns: 0 drops column 2, 2 inserts behind it a seeded
    permutation of it (another column of the same scale, so that the two physics inputs do not act alike)."""
    w = {k: v.copy() for k, v in load_golden(name).items()}
    if phys_dim == 0:
        w[W0] = np.delete(w[W0], 2, axis=1)
    elif phys_dim == 2:
        col = w[W0][np.random.default_rng(2).permutation(w[W0].shape[0]), 2]
        w[W0] = np.insert(w[W0], 3, col, axis=1)
    else:
        assert phys_dim == 1
    assert w[W0].shape[1] == 5 + phys_dim
    return w


def material_config(phys_dim):
    params = [{"name": "particle_radius", "use": False, "min": 0.0, "max": 1.0}]
    params += [{"name": f"param{i}", "use": True, "min": 0.0, "max": 1.0} for i in range(phys_dim)]
    return {"material_index": {"rope": 0}, "rope": {"physics_params": params}}


def make_model(w, phys_dim, pstep, prec):
    from adaptigraph_amd.model import DynamicsPredictor
    cfg = configs.model_config()
    cfg["pstep"] = pstep
    m = DynamicsPredictor(cfg, material_config(phys_dim), configs.dataset_config("rope"), DEV)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    m = m.to(DEV).eval()
    m.set_option("precision", PRECISIONS[prec])
    return m


@functools.lru_cache(maxsize=None)
def graph_inputs(shape):
    """The configuration-independent inputs of a shape and its edge lists from the oracle's builder."""
    n_obj, B, n_pad = SHAPES[shape]
    g = synth.make_graph_inputs("rope", n_obj, B, seed=4, spacing=0.1, n_pad=n_pad)
    n_rel, recv, send = ago.build_edges(g["state"][:, -1], RADIUS, g["mask"], g["tool_mask"], TOPK, False, "batch")
    g["n_rel"], g["recv"], g["send"] = n_rel, recv, send
    g["lists"] = [(recv[b, :n], send[b, :n]) for b, n in enumerate(n_rel)]
    return g


@functools.lru_cache(maxsize=None)
def config_inputs(shape, phys_dim, n_inst):
    """phys uniform in [0.1, 0.9], p_instance one random one-hot column per object particle (zero rows for padded slots)."""
    g = graph_inputs(shape)
    B, n_p, n_obj = g["state"].shape[0], g["n_p"], g["n_obj"]
    rng = np.random.default_rng(4)
    phys = rng.uniform(0.1, 0.9, (B, phys_dim)).astype(np.float32)
    p_inst = np.zeros((B, n_p, n_inst), np.float32)
    if n_inst:
        col = rng.integers(0, n_inst, (B, n_obj))
        p_inst[np.arange(B)[:, None], np.arange(n_obj)[None], col] = 1
    return phys, p_inst


def step64(W, state, attrs, p_inst, delta, phys, edges, pstep):
    """`_step64` of tests/test_grad_rollout.py (one model step in float64 over per-sample edge lists), returning the motion as well:
    -> (state + clamp(motion), motion)."""
    B, H, N, _ = state.shape
    n_p = p_inst.shape[1]
    sn = torch.cat([state[:, 1:] - state[:, :-1], state[:, -1:]], 1).transpose(1, 2).reshape(B, N, -1)
    ph = torch.cat([phys[:, None].expand(B, n_p, -1), phys.new_zeros(B, N - n_p, phys.shape[1])], 1)
    p_in = torch.cat([attrs, ph, delta], 2)
    grp = torch.cat([p_inst, p_inst.new_zeros(B, N - n_p, p_inst.shape[2])], 1)
    pos, mot = [], []
    for b in range(B):
        r, s = (torch.from_numpy(e.astype(np.int64)) for e in edges[b])
        rel = torch.cat([attrs[b][r], attrs[b][s], (grp[b][r] - grp[b][s]).abs().sum(1, keepdim=True), sn[b][r] - sn[b][s]], 1)
        enc_n, enc_e = _mlp(W, p_in[b], "particle_encoder"), _mlp(W, rel, "relation_encoder")
        h = enc_n
        for _ in range(pstep):
            eff = F.relu(_lin(W, torch.cat([enc_e, h[r], h[s]], 1), "relation_propagator.linear"))
            agg = torch.zeros_like(h).index_add(0, r, eff)
            h = F.relu(_lin(W, torch.cat([enc_n, agg], 1), "particle_propagator.linear") + h)
        m = _lin(W, F.relu(_lin(W, F.relu(_lin(W, h[:n_p], "non_rigid_predictor.linear_0")), "non_rigid_predictor.linear_1")),
                 "non_rigid_predictor.linear_2")
        mot.append(m)
        pos.append(state[b, -1, :n_p] + m.clamp(-100, 100))
    return torch.stack(pos), torch.stack(mot)


def d64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def ref64_of(w, g, phys, p_inst, pstep):
    W = {k: d64(v) for k, v in w.items()}
    pos, mot = step64(W, d64(g["state"]), d64(g["attrs"]), d64(p_inst), d64(g["action"]), d64(phys), g["lists"], pstep)
    return pos.numpy(), mot.numpy()


@functools.lru_cache(maxsize=None)
def ref64(shape, wname, cfg):
    """(pos, motion) of the float64 step for a shape, weight set and configuration: computed once, never written to."""
    phys_dim, n_inst, pstep = cfg
    phys, p_inst = config_inputs(shape, phys_dim, n_inst)
    return ref64_of(weights_np(wname, phys_dim), graph_inputs(shape), phys, p_inst, pstep)


# ------------------------------------------------------------------------------------------------------ 1. the two references (CPU)
def test_inputs_are_the_ragged_ones():
    g = graph_inputs("rope93")
    assert int(g["n_rel"].sum()) == 1813 and g["attrs"].shape[:2] == (3, 101) and not g["mask"][:, 93:100].any()
    assert (3 * 101) % 32 != 0 and 1813 % 128 != 0 and 1813 % 32 != 0
    for n_inst in (0, 1, 2, 3):
        phys, p_inst = config_inputs("rope93", 1, n_inst)
        assert p_inst.shape == (3, 100, n_inst) and (p_inst[:, :93].sum(-1) == (1 if n_inst else 0)).all() and not p_inst[:, 93:].any()
        assert n_inst < 2 or all(p_inst[:, :93, c].any() for c in range(n_inst))
    assert config_inputs("rope93", 0, 1)[0].shape == (3, 0) and 0.1 <= config_inputs("rope93", 2, 1)[0].min()


def test_restated_float64_step_is_the_suites():
    g = graph_inputs("rope93")
    phys, p_inst = config_inputs("rope93", 2, 3)
    W = {k: d64(v) for k, v in weights_np("weights_seed0", 2).items()}
    args = (W, d64(g["state"]), d64(g["attrs"]), d64(p_inst), d64(g["action"]), d64(phys), g["lists"])
    assert torch.equal(step64(*args, 4)[0], _step64(*args, pstep=4))


@pytest.mark.parametrize("wname", WEIGHT_SETS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
def test_oracle_forward_agrees_with_the_float64_step(cfg, wname):
    """The fp32 CPU oracle (`ago.forward(..., pstep=...)`) and the float64 step, neither of which had run at these configurations, within
    1e-6 max-abs on the motion (measured on these inputs over the 3 x 4 x 5 grid of configurations: at most 1.35e-7, max|motion| 0.03 .. 0.18)."""
    phys_dim, n_inst, pstep = cfg
    g = graph_inputs("rope93")
    phys, p_inst = config_inputs("rope93", phys_dim, n_inst)
    pos, mot = ago.forward(weights_np(wname, phys_dim), g["state"], g["attrs"], g["action"], p_inst, phys, g["n_rel"], g["recv"], g["send"], pstep=pstep)
    ref_pos, ref_mot = ref64("rope93", wname, cfg)
    err = float(np.abs(mot - ref_mot).max())
    print(f"{cfg_id(cfg)} {wname}: oracle vs float64 {err:.3e}, max|motion| {np.abs(ref_mot).max():.3f}")
    assert mot.shape == ref_mot.shape == (3, 100, 3) and 0.01 < np.abs(ref_mot).max() < 1.0
    assert err <= TOL_REFS and float(np.abs(pos - ref_pos).max()) <= TOL_REFS + 2.0 ** -21      # (+ the rounding of the fp32 addition to |state| < 16)


def perturbed_refs(shape, wname, cfg):
    """Max-abs change of the float64 motion when an input is perturbed -> dict.  Instances: "merged" every particle of every sample moved to
    instance 0 (membership erased), "column0_only" every column but the first dropped (what an encoder that reads column 0 alone computes),
    "columns_permuted" the columns of sample 0 reversed.  Physics: "second_phys" the second value of every sample raised by 2.0 (a
    physics value is an unbounded input of a linear layer: the size of the step is free), "second_phys_as_first" the first value in its place (what an encoder that reads column 0 alone computes)."""
    phys_dim, n_inst, pstep = cfg
    w, g = weights_np(wname, phys_dim), graph_inputs(shape)
    phys, p_inst = config_inputs(shape, phys_dim, n_inst)
    base, out = ref64(shape, wname, cfg)[1], {}
    if n_inst >= 2:
        merged, first, cols = np.zeros_like(p_inst), p_inst.copy(), p_inst.copy()
        merged[:, :g["n_obj"], 0] = 1
        first[:, :, 1:] = 0
        cols[0] = p_inst[0][:, ::-1]
        for name, pi in (("merged", merged), ("column0_only", first), ("columns_permuted", cols)):
            out[name] = float(np.abs(ref64_of(w, g, phys, pi, pstep)[1] - base).max())
    if phys_dim >= 2:
        far, same = phys.copy(), phys.copy()
        far[:, 1] += 2.0
        same[:, 1] = phys[:, 0]
        for name, ph in (("second_phys", far), ("second_phys_as_first", same)):
            out[name] = float(np.abs(ref64_of(w, g, ph, p_inst, pstep)[1] - base).max())
    return out


@pytest.mark.parametrize("wname", WEIGHT_SETS)
@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c[1] >= 2 or c[0] == 2], ids=cfg_id)
def test_reference_is_sensitive_to_instances_and_to_the_second_physics_value(cfg, wname):
    """The value checks below can only catch a kernel that ignores an input if the output depends on it.  In float64, erasing the instance membership
    and raising the second physics value by 2.0 each change the motion by more than 100 x the widest forward tolerance (TOL_BY_PREC of
    `fast`).  Permuting the instance COLUMNS of a sample changes nothing, in float64 as in the engine: the edge input is sum_c |g_r[c] - g_s[c]|, a
    symmetric function of the columns — so it is the membership that is perturbed here.
    The two single-column misreadings — instance column 0 alone, the first physics value in place of the second — are smaller perturbations; they
    move the motion by more than 10 x that tolerance, so a kernel that makes one of them misses its value check by an order of magnitude."""
    d = perturbed_refs("rope93", wname, cfg)
    print(f"{cfg_id(cfg)} {wname}: " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
    tol = max(TOL_BY_PREC.values())
    for k, v in d.items():
        if k == "columns_permuted":
            assert v <= 1e-12, (k, v)
        else:
            assert v > (100 if k in ("merged", "second_phys") else 10) * tol, (k, v)


# ------------------------------------------------------------------------------------------------------ 2. forward at every configuration (GPU)
def engine_forward(m, g, csr, phys, p_inst):
    pos, mot = m(t(g["state"]), t(g["attrs"]), csr, None, t(p_inst), action=t(g["action"]), rope_physics_param=t(phys))
    return pos.clone(), mot.clone()


FORWARD_CASES = [("rope93", c) for c in CONFIGS] + [("rope300", c) for c in CONFIGS if c[2] in (1, 2, 4) or c[1] in (0, 2)]


def record(line):
    """AG_MODEL_CONFIGS_PROFILE=<file>: the measured deviations as lines of that file (profiles/model_configs_fwd_err.txt is such a run)."""
    path = os.environ.get("AG_MODEL_CONFIGS_PROFILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("wname", WEIGHT_SETS)
@pytest.mark.parametrize("shape,cfg", FORWARD_CASES, ids=[f"{s}-{cfg_id(c)}" for s, c in FORWARD_CASES])
def test_forward_at_every_configuration_vs_float64(shape, cfg, wname, prec):
    """model(...) against the float64 step: |motion - ref| <= TOL_BY_PREC[prec] and |pos - ref| <= TOL_FWD for pstep <= 3; for pstep 4 and 5, which
    nobody had measured, the hard bound is the gate TOL_FWD on both (measured: profiles/model_configs_fwd_err.txt, every configuration, weight set
    and precision — the four- and five-round models too stay inside TOL_BY_PREC).  Status 0.  The same bits under node_dedup 0 / 2 and
    node_stationary 0 / 1, in `fast` also under edge_stationary 0 / 1 and fuse_aggregate 0 / 2, and — the edge input being symmetric in the
    instance columns, a sum of exact 0 / 1 terms — with the instance columns reversed.  rope300 x 2: several 128-row tiles and a partial last one,
    of edges and of nodes."""
    phys_dim, n_inst, pstep = cfg
    g = graph_inputs(shape)
    phys, p_inst = config_inputs(shape, phys_dim, n_inst)
    B, N = g["attrs"].shape[:2]
    if shape == "rope300":
        n_edges = int(g["n_rel"].sum())
        assert (B, N) == (2, 301) and n_edges > 3 * 128 and n_edges % 128 != 0 and B * N > 3 * 128 and (B * N) % 128 != 0
    m = make_model(weights_np(wname, phys_dim), phys_dim, pstep, prec)
    csr = csr_from_lists(g["n_rel"], g["recv"], g["send"], N)
    pos, mot = engine_forward(m, g, csr, phys, p_inst)
    ref_pos, ref_mot = ref64(shape, wname, cfg)
    e_mot, e_pos = float(np.abs(mot.cpu().numpy() - ref_mot).max()), float(np.abs(pos.cpu().numpy() - ref_pos).max())
    status = m.take_status()
    line = (f"{shape:8s} {cfg_id(cfg):20s} {wname:20s} {prec:6s} status {status} motion max-abs {e_mot:.3e} pos max-abs {e_pos:.3e} "
            f"(|motion| max {np.abs(ref_mot).max():.3f}, TOL_BY_PREC {TOL_BY_PREC[prec]:.0e}{', ABOVE IT' if e_mot > TOL_BY_PREC[prec] else ''})")
    print(line)
    record(line)
    assert mot.shape == ref_mot.shape and bool(torch.isfinite(mot).all()) and status == 0
    assert e_mot <= (TOL_BY_PREC[prec] if pstep <= 3 else TOL_FWD), line
    assert e_pos <= TOL_FWD, line
    options = [("node_dedup", 0), ("node_dedup", 2), ("node_stationary", 0), ("node_stationary", 1)]
    if prec == "fast":
        options += [("edge_stationary", 0), ("edge_stationary", 1), ("fuse_aggregate", 2), ("fuse_aggregate", 0)]
    for name, value in options:
        was = m.get_option(name)
        m.set_option(name, value)
        got = engine_forward(m, g, csr, phys, p_inst)
        m.set_option(name, was)
        assert torch.equal(got[1], mot) and torch.equal(got[0], pos), (name, value, float((got[1] - mot).abs().max()))
    if n_inst >= 2:
        got = engine_forward(m, g, csr, phys, np.ascontiguousarray(p_inst[:, :, ::-1]))
        assert torch.equal(got[1], mot), ("instance columns reversed", float((got[1] - mot).abs().max()))
    assert m.take_status() == 0


# ------------------------------------------------------------------------------------------------------ 3. rollouts at the configurations (GPU)
REPEAT = np.array([4, 1, 3, 4, 2], np.int32)      # per-sample action_repeat of the four-step rollouts
ROLLOUT_OPTIONS = [("self_edges", 0), ("node_dedup", 0), ("node_dedup", 2), ("rollout_streams", 2), ("shared_state", 1), ("node_stationary", 0)]
ROLLOUT_OPTIONS_FAST = [("edge_stationary", 0), ("fuse_aggregate", 2)]


def rollout_call(m, g, state, phys, p_inst, repeat, n_steps):
    B = state.shape[0]
    thr = aggraph.threshold_sq(RADIUS, B, torch.device(DEV), _lib.AG_VARIANT_BATCH)
    seq, fin = rollout(m, state, t(g["action"]), t(g["attrs"]), t(p_inst), t(phys), t(g["mask"]), t(g["tool_mask"]), thr, t(repeat), n_steps, TOPK, False,
                       g["n_tools"], return_state=True)
    return seq.clone(), fin.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("wname", WEIGHT_SETS)
@pytest.mark.parametrize("cfg", ROLLOUT_CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("shape", ["rope150x5", "rope300x5"])
def test_rollout_at_the_configurations(shape, cfg, wname, prec):
    """The raw rollout(...), five samples with their own clouds and step counts.
    One step against float64: the engine's edge lists equal the oracle's, and out_seq of a one-step rollout is within the forward's tolerance of
    state + clamp(motion) — TOL_BY_PREC[prec] plus half an ulp of the largest position (the one fp32 addition that makes a position of a motion)
    for pstep <= 3, the gate TOL_FWD for pstep 4, and TOL_FWD in any case.
    Four steps against four chained one-step rollouts, each fed the previous state_final: state_final, and out_seq of every sample at the step its
    `repeat` names, bit for bit.  The chained calls encode the nodes afresh and start from unswapped Hr / Hs buffers every step; the one call encodes
    once (node_dedup 2) and carries the swap parity of an odd or even pstep from step to step.
    The same bits under self_edges 0, node_dedup 0 and 2, rollout_streams 2, shared_state 1, node_stationary 0, and in `fast` edge_stationary 0 and
    fuse_aggregate 2; status 0."""
    phys_dim, n_inst, pstep = cfg
    g = graph_inputs(shape)
    phys, p_inst = config_inputs(shape, phys_dim, n_inst)
    B, N = g["attrs"].shape[:2]
    m = make_model(weights_np(wname, phys_dim), phys_dim, pstep, prec)
    state0, ones = t(g["state"]), np.ones(B, np.int32)

    lists = aggraph.build_edges(state0[:, -1], RADIUS, t(g["mask"]), t(g["tool_mask"]), TOPK, False, "batch", max_tools=g["n_tools"]).to_lists()
    for b, (r, s) in enumerate(lists):
        assert np.array_equal(r, g["lists"][b][0]) and np.array_equal(s, g["lists"][b][1]), f"edge lists of sample {b}"
    one, _ = rollout_call(m, g, state0, phys, p_inst, ones, 1)
    ref_pos = ref64(shape, wname, cfg)[0]
    err = float(np.abs(one.cpu().numpy() - ref_pos).max())
    half_ulp = float(np.spacing(np.float32(np.abs(ref_pos).max()))) / 2
    bound = min(TOL_FWD, TOL_BY_PREC[prec] + half_ulp) if pstep <= 3 else TOL_FWD
    print(f"{shape} {cfg_id(cfg)} {wname} {prec}: one step vs float64 {err:.3e} (bound {bound:.3e})")
    assert err <= bound

    seq4, fin4 = rollout_call(m, g, state0, phys, p_inst, REPEAT, 4)
    state, chained = state0, []
    for k in range(4):
        out, state = rollout_call(m, g, state, phys, p_inst, ones, 1)
        chained.append(out)
    assert torch.equal(chained[0], one) and not torch.equal(chained[3], chained[2])
    assert torch.equal(fin4, state), float((fin4 - state).abs().max())
    for b in range(B):
        assert torch.equal(seq4[b], chained[REPEAT[b] - 1][b]), (b, int(REPEAT[b]))

    for name, value in ROLLOUT_OPTIONS + (ROLLOUT_OPTIONS_FAST if prec == "fast" else []):
        was = m.get_option(name)
        m.set_option(name, value)
        got = rollout_call(m, g, state0, phys, p_inst, REPEAT, 4)
        m.set_option(name, was)
        assert torch.equal(got[0], seq4) and torch.equal(got[1], fin4), (name, value)
    assert bool(torch.isfinite(fin4).all()) and m.take_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("cfg", SCRIPTED_CONFIGS, ids=cfg_id)
@pytest.mark.parametrize("name", ["rope50", "rope300"])
def test_scripted_rollout_equals_the_step_loop_at_the_configurations(name, cfg, prec):
    """ag_rollout_scripted against the loop of build_edges + forward it replaces (tests/test_scripted_rollout.py asserts this at pstep 3, one
    physics parameter, one instance): every step's prediction and the final state bit for bit."""
    phys_dim, n_inst, pstep = cfg
    c = scripted_inputs(name)
    rng = np.random.default_rng(7)
    p_inst = np.zeros((c.B, c.n_p, n_inst), np.float32)
    p_inst[np.arange(c.B)[:, None], np.arange(c.n_p)[None], rng.integers(0, n_inst, (c.B, c.n_p))] = 1
    c = types.SimpleNamespace(**dict(vars(c), phys=t(rng.uniform(0.1, 0.9, (c.B, phys_dim)).astype(np.float32)), p_instance=t(p_inst)))
    m = make_model(weights_np("weights_seed0", phys_dim), phys_dim, pstep, prec)
    pred_ref, state_ref, lists = step_loop(m, c)
    out = scripted(m, c)
    assert any(len(a[0]) != len(b[0]) or not np.array_equal(a[1], b[1]) for a, b in zip(lists[0], lists[-1])), "the edge lists never change"
    assert torch.equal(out["pred_seq"], pred_ref), float((out["pred_seq"] - pred_ref).abs().max())
    assert torch.equal(out["state_final"], state_ref)
    assert bool(torch.isfinite(out["pred_seq"]).all()) and m.take_status() == 0


# ------------------------------------------------------------------------------------------------------ 4. the life of the weights (GPU)
W1_NAME, W2_NAME = WEIGHT_SETS


def tensors(w):
    return {k: torch.from_numpy(v.copy()) for k, v in w.items()}


def life_run(m):
    """A rope-93 forward and a three-step rollout of a one-physics-parameter, one-instance model -> (pos, motion, out_seq, state_final)."""
    g = graph_inputs("rope93")
    phys, p_inst = config_inputs("rope93", 1, 1)
    csr = csr_from_lists(g["n_rel"], g["recv"], g["send"], g["attrs"].shape[1])
    return engine_forward(m, g, csr, phys, p_inst) + rollout_call(m, g, t(g["state"]), phys, p_inst, np.array([3, 1, 2], np.int32), 3)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def fresh_run(wkey, prec, edge_products=2):
    """The outputs of a model CREATED with a weight set ("w1", "w2", "w3": the rescaled W1): the yardstick of every repacked model."""
    m = make_model(life_weights(wkey), 1, 3, prec)
    m.set_option("edge_products", edge_products)
    out = life_run(m)
    assert m.take_status() == 0
    return out


@functools.lru_cache(maxsize=None)
def edge_rescale():
    """The smallest power of two s for which rescale_edge_stack(W1, s) holds an edge-stack weight or bias beyond fp16's 65504."""
    w1 = weights_np(W1_NAME, 1)
    s = 2.0
    while max(float(np.abs(v).max()) for k, v in rescale_edge_stack(w1, s).items() if k.startswith("relation_encoder")) <= 65504.0:
        s *= 2.0
    return s


def life_weights(key):
    if key == "w3":
        return rescale_edge_stack(weights_np(W1_NAME, 1), edge_rescale())
    return weights_np({"w1": W1_NAME, "w2": W2_NAME}[key], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_repacked_weights_equal_a_fresh_models(prec):
    """One model runs W1 -> load_state_dict(W2) -> W1 again (ag_model_update_weights repacks every chunk image into the live allocation): each
    output equals a freshly created model's with those weights bit for bit, and the third equals the first."""
    m = make_model(life_weights("w1"), 1, 3, prec)
    first = life_run(m)
    m.load_state_dict(tensors(life_weights("w2")))
    second = life_run(m)
    m.load_state_dict(tensors(life_weights("w1")))
    third = life_run(m)
    assert not torch.equal(first[1], second[1])
    assert same(first, fresh_run("w1", prec)) and same(second, fresh_run("w2", prec)) and same(third, fresh_run("w1", prec)) and same(third, first)
    assert m.take_status() == 0


@pytest.mark.gpu
def test_edge_weights_beyond_fp16_keep_the_split_bf16_edge_stack():
    """W3 = rescale_edge_stack(W1, s), s the smallest power of two that puts an edge-stack weight beyond 65504: the same function (the float64
    output does not move), but the fp16 edge stack of `fast` cannot hold it.  A `fast` model created with W3 stays within TOL_BY_PREC["fast"] of
    float64 with status 0, equals the same model with edge_products 3 bit for bit, and gives the same bits with edge_stationary 0 and 1 (neither
    applies).  A power-of-two rescale commutes with every rounding of the split-bf16 path, so the bits are also those of W1 with edge_products 3."""
    w1, w3, s = life_weights("w1"), life_weights("w3"), edge_rescale()
    edge = [k for k in w3 if k.startswith("relation_encoder")]
    assert max(float(np.abs(w3[k]).max()) for k in edge) > 65504.0 >= max(float(np.abs(rescale_edge_stack(w1, s / 2)[k]).max()) for k in edge)
    g = graph_inputs("rope93")
    phys, p_inst = config_inputs("rope93", 1, 1)
    ref_pos, ref_mot = ref64("rope93", W1_NAME, (1, 1, 3))
    pos3, mot3 = ref64_of(w3, g, phys, p_inst, 3)
    assert float(np.abs(mot3 - ref_mot).max()) <= 1e-13 and float(np.abs(pos3 - ref_pos).max()) <= 1e-13
    m = make_model(w3, 1, 3, "fast")
    out = life_run(m)
    err = float(np.abs(out[1].cpu().numpy() - ref_mot).max())
    print(f"edge stack x {s:g}: fast vs float64 {err:.3e}")
    assert err <= TOL_BY_PREC["fast"] and m.take_status() == 0
    for name, value in (("edge_products", 3), ("edge_stationary", 0), ("edge_stationary", 1)):
        m.set_option(name, value)
        assert same(life_run(m), out), (name, value)
    assert m.take_status() == 0
    assert same(out, fresh_run("w1", "fast", 3)), float((out[1] - fresh_run("w1", "fast", 3)[1]).abs().max())
    assert not same(out, fresh_run("w1", "fast"))      # (and not the fp16 edge stack's)


def workspace_bytes(m):
    g = graph_inputs("rope93")
    B, N = g["attrs"].shape[:2]
    L, h = _lib.lib(), m.handle(torch.device(DEV))
    prm = _lib.RolloutParams(B, N, g["n_p"], 1, TOPK, 0, g["n_tools"], 3, _lib.AG_HEIGHT_MIN, 0.0)
    return L.ag_forward_workspace_bytes_for(h, B, N, int(g["n_rel"].sum())), L.ag_rollout_workspace_bytes_for(h, ctypes.byref(prm))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_update_across_the_fp16_range_flips_the_edge_stack(prec):
    """A model created with W1 is updated to W3 (out of fp16's range: `fast` must leave its fp16 edge stack) and back (must return to it): each
    output equals the fresh model's bit for bit, the workspace queries equal the fresh model's after each update, and the rollout right after a
    flip runs on the Python workspace cache as the previous path left it."""
    m = make_model(life_weights("w1"), 1, 3, prec)
    fresh = {k: make_model(life_weights(k), 1, 3, prec) for k in ("w1", "w3")}
    for step, key in enumerate(("w1", "w3", "w1", "w3")):
        if step:
            m.load_state_dict(tensors(life_weights(key)))
        assert same(life_run(m), fresh_run(key, prec)), key
        assert workspace_bytes(m) == workspace_bytes(fresh[key]), key
        assert m.take_status() == 0
    if prec == "fast":
        assert not same(fresh_run("w1", prec), fresh_run("w3", prec))


class CountingLib:
    """_lib.lib() with the calls of ag_model_update_weights counted."""

    def __init__(self, L):
        self._L, self.updates = L, 0

    def __getattr__(self, name):
        return getattr(self._L, name)

    def ag_model_update_weights(self, *args):
        self.updates += 1
        return self._L.ag_model_update_weights(*args)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_weight_edits_reach_the_engine(prec, monkeypatch):
    """An in-place edit under no_grad bumps the parameter's version counter and is repacked on the next call by itself; an edit through `.data`
    does not bump it (the engine would go on with the old weights) and reaches the engine after model.sync_weights(force=True); an unforced
    sync_weights() on unchanged weights does not repack."""
    counting = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    key = "particle_propagator.linear.weight"
    w1 = life_weights("w1")
    edited = dict(w1, **{key: w1[key] * np.float32(1.25)})
    edited2 = dict(w1, **{key: w1[key] * np.float32(1.25) * np.float32(0.5)})
    want1, want2 = life_run(make_model(edited, 1, 3, prec)), life_run(make_model(edited2, 1, 3, prec))
    m = make_model(w1, 1, 3, prec)
    before = life_run(m)
    assert same(before, fresh_run("w1", prec)) and not same(before, want1) and not same(want1, want2)
    p = dict(m.named_parameters())[key]
    n0 = counting.updates
    with torch.no_grad():
        p.mul_(1.25)
    assert same(life_run(m), want1) and counting.updates == n0 + 1
    m.sync_weights()
    life_run(m)
    assert counting.updates == n0 + 1, "an unforced sync of unchanged weights repacked"
    p.data.mul_(0.5)
    m.sync_weights(force=True)
    assert counting.updates == n0 + 2
    assert same(life_run(m), want2)
    assert counting.updates == n0 + 2 and m.take_status() == 0
