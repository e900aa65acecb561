"""Scripted-tool rollout on the device (ag_rollout_scripted, forward_dynamics.rollout_scripted, eval_rollout's `scripted` keyword):
the C-ABI surface (CPU), and on the GPU the call against the step loop it replaces — predictions and final state bit for bit, the error
against a float64 evaluation — plus determinism, HIP-graph capture with a script rewritten between replays, no host synchronisation,
refusals as codes and the evaluation driver over the fixture dataset."""
import ctypes
import functools
import os
import pickle
import re
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from adaptigraph_amd import _lib, configs, eval_rollout as er, graph as aggraph, synth
from adaptigraph_amd.forward_dynamics import rollout_scripted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NEW = ("ag_rollout_scripted_workspace_bytes_for", "ag_rollout_scripted")


def err_bound(n_p):
    """Relative bound of the fp32 error against its float64 evaluation on the same fp32 inputs: per term one rounding in each difference, three
    products, two adds and a square root (together below 8 units), an n_p-term fp32 sum in any fixed order, one division."""
    return (n_p + 8) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------ CPU
def test_scripted_entry_points_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adaptigraph_hip.h")).read(), flags=re.S)
    declared = [n for n in re.findall(r"\b(ag_[a-z0-9_]+)\s*\(", text)]
    for name in NEW:
        assert declared.count(name) == 1, f"{name} is not declared exactly once in include/adaptigraph_hip.h"
    assert list(_lib.SIGNATURES) == declared, "the rows of _lib.SIGNATURES are not in the header's order"
    assert declared.index(NEW[0]) + 1 == declared.index(NEW[1]) == declared.index("ag_rollout") + 2
    ret, args = _lib.SIGNATURES["ag_rollout_scripted"]
    assert ret is ctypes.c_int and len(args) == 20 and args[-2] is ctypes.c_size_t and args[1]._type_ is _lib.ScriptedParams
    assert [f[0] for f in _lib.ScriptedParams._fields_] == ["B", "N", "n_p", "n_instance", "topk", "connect_tools_all", "max_tools", "variant",
                                                            "n_steps"]
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), f"{name} is not exported by the built library"
    # the size query needs no GPU: it grows with the batch, and sizes that the call refuses give 0
    q = lambda *v: L.ag_rollout_scripted_workspace_bytes_for(None, ctypes.byref(_lib.ScriptedParams(*v)))      # noqa: E731
    assert q(4, 101, 100, 1, 10, 0, 1, 0, 5) > q(2, 101, 100, 1, 10, 0, 1, 0, 5) > 2 * 101 * 10 * 160 * 4
    assert q(2, 101, 100, 1, 10, 0, 1, 0, 5) == q(2, 101, 100, 1, 10, 0, 1, 0, 50), "the workspace does not depend on the number of steps"
    assert q(2, 101, 102, 1, 10, 0, 1, 0, 5) == 0 and q(2, 101, 100, 1, 10, 0, 1, 0, 0) == 0 and q(2, 101, 100, 1, 65, 0, 1, 0, 5) == 0


def test_drivers_keep_the_reference_signature_and_take_the_keyword_last():
    import inspect
    names = list(inspect.signature(er.rollout_from_start_graph).parameters)
    assert names == ["graph", "fps_idx_list", "dataset_config", "material_config", "model", "device", "eef_pos", "obj_pos", "current_start",
                     "current_end", "get_next_pair_or_break_func", "pairs", "save_dir", "viz", "imgs", "cam_info", "scripted"]      # rollout.py:20-23
    for fn in (er.rollout_batch, er.rollout_from_start_graph, er.rollout_episode_pushes, er.rollout_dataset):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "scripted" and last.default is False, fn.__name__


# ------------------------------------------------------------------------------------------------------ GPU
def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def engine_model(material, precision=None, node_dedup=None):
    """One model per (material, options); `precision` None = the engine's default mode."""
    return _engine_model(material, precision, node_dedup)


@functools.lru_cache(maxsize=None)
def _engine_model(material, precision, node_dedup):
    from adaptigraph_amd.model import DynamicsPredictor
    w = load_golden("weights_seed0")
    m = DynamicsPredictor(configs.model_config(), configs.material_config(material), configs.dataset_config(material), DEV)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in w.items()})
    m = m.to(DEV).eval()
    if precision is not None:
        m.set_option("precision", precision)
    if node_dedup is not None:
        m.set_option("node_dedup", node_dedup)
    return m


#        name            material   objects pad tools B  T  variant
CASES = {"rope50": ("rope", 50, 0, 1, 3, 6, "single"),            # brute-force edge path
         "granular200": ("granular", 200, 0, 5, 2, 4, "batch"),   # five tool slots, the material's connect_tools_all and top-k 20
         "rope300": ("rope", 300, 0, 1, 2, 4, "batch"),           # uniform-grid edge path (N >= 256)
         "rope700": ("rope", 700, 0, 1, 2, 3, "single"),          # 3N > 2048: more than one chunk per sample in the step kernel
         "cloth64": ("cloth", 64, 0, 1, 2, 3, "batch"),           # connect_tools_all on
         "masked": ("rope", 60, 7, 1, 3, 4, "single")}            # invalid object slots at the end of the object range


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The inputs of a case on the device: synth.make_graph_inputs with the tool lifted 2.0 above the cloud, and a script that drives it into
    the cloud — back to where make_graph_inputs had put it — at step 1 and along x from there, so that the tool has no edge to the cloud at
    step 0 and some later."""
    material, n_obj, n_pad, n_t, B, T, variant = CASES[name]
    g = synth.make_graph_inputs(material, n_obj, B, seed=11, n_pad=n_pad, spacing=0.1)
    assert g["n_tools"] == n_t
    n_p, N = g["n_p"], g["n_p"] + n_t
    rng = np.random.default_rng(5)
    if name == "masked":       # sample 1: five more invalid slots in front of the padding
        lo = n_obj - 5
        g["mask"][1, lo:n_obj] = False
        g["attrs"][1, lo:n_obj] = 0
        g["p_instance"][1, lo:n_obj] = 0
        g["state"][1, :, lo:n_obj] = 0
    tool0 = g["state"][:, -1, n_p:].copy()                          # (B, n_t, 3): where make_graph_inputs put the tool, inside the cloud
    g["state"][:, :, n_p:, 1] += 2.0
    tool_pos = np.zeros((B, T, n_t, 3), np.float32)
    for k in range(T):
        tool_pos[:, k] = tool0 + np.array([0.05 * k, 0.0, 0.0], np.float32)
    tool_delta = np.zeros_like(tool_pos)
    tool_delta[:, :-1] = tool_pos[:, 1:] - tool_pos[:, :-1]
    tool_delta[:, -1] = tool_delta[:, -2]
    tool_pos[:, 0] = 77.0                                           # entry 0 is never read
    tool_delta[:, 0] = 77.0
    g["action"][:, n_p:] = np.array([0.05, -2.0, 0.0], np.float32)
    gt = g["state"][:, -1:, :n_p] + rng.normal(0, 0.02, (B, T, n_p, 3)).astype(np.float32)
    M = synth.MATERIALS[material]
    dev = torch.device(DEV)
    var = _lib.AG_VARIANT_SINGLE if variant == "single" else _lib.AG_VARIANT_BATCH
    return types.SimpleNamespace(
        material=material, B=B, T=T, N=N, n_p=n_p, n_t=n_t, variant=variant, radius=M["radius"], topk=M["topk"], connect=M["connect_tools_all"],
        state0=t(g["state"]), action0=t(g["action"]), attrs=t(g["attrs"]), p_instance=t(g["p_instance"]), phys=t(g["phys"]), mask=t(g["mask"]),
        tool_mask=t(g["tool_mask"]), tool_pos=t(tool_pos), tool_delta=t(tool_delta), gt=t(gt.astype(np.float32)),
        obj_mask=t(g["mask"][:, :n_p].copy()), thr_sq=aggraph.threshold_sq(M["radius"], B, dev, var))


def step_loop(model, c, tool_pos=None, tool_delta=None):
    """The loop the call replaces, eval_rollout.rollout_batch's: build_edges on state[:, -1], the model, cat and shift.
    -> (pred_seq, state_final, the edge lists of every step)."""
    tool_pos = c.tool_pos if tool_pos is None else tool_pos
    tool_delta = c.tool_delta if tool_delta is None else tool_delta
    state, action, preds, lists = c.state0, c.action0, [], []
    for k in range(c.T):
        edges = aggraph.build_edges(state[:, -1], c.radius, c.mask, c.tool_mask, c.topk, c.connect, c.variant, max_tools=c.n_t)
        lists.append(edges.to_lists())
        pred, _ = model(state, c.attrs, edges, None, c.p_instance, action=action, **{c.material + "_physics_param": c.phys})
        preds.append(pred)
        if k + 1 < c.T:
            nxt = torch.cat([pred, tool_pos[:, k + 1]], 1)
            state = torch.cat([state[:, 1:], nxt[:, None]], 1)
            action = torch.zeros_like(action)
            action[:, c.n_p:] = tool_delta[:, k + 1]
    return torch.stack(preds, 1), state, lists


def scripted(model, c, **kw):
    kw = dict(dict(gt=c.gt, obj_mask=c.obj_mask, return_state=True), **kw)
    tool_pos, tool_delta = kw.pop("tool_pos", c.tool_pos), kw.pop("tool_delta", c.tool_delta)
    return rollout_scripted(model, c.state0, c.action0, tool_pos, tool_delta, c.attrs, c.p_instance, c.phys, c.mask, c.tool_mask, c.thr_sq, c.topk,
                            c.connect, c.n_t, variant=c.variant, **kw)


def run(name, precision=None, node_dedup=None):
    """(inputs, the step loop's results, the call's results) of a case: computed once, shared by the tests, never written to."""
    return _run(name, precision, node_dedup)


@functools.lru_cache(maxsize=None)
def _run(name, precision, node_dedup):
    c, model = inputs(name), engine_model(CASES[name][0], precision, node_dedup)
    ref = step_loop(model, c)
    out = scripted(model, c)
    torch.cuda.synchronize()
    return c, ref, out


RUNS = [("rope50", 0, None), ("rope50", 1, None), ("rope50", 2, None), ("rope300", 0, None), ("rope300", 1, None), ("rope300", 2, None),
        ("granular200", None, None), ("rope700", None, None), ("cloth64", None, None), ("masked", None, None),
        ("rope50", None, 2)]      # (the last: node-encoder de-duplication forced, whose work list is rebuilt every step here)


def lists_differ(a, b):
    return any(len(x[0]) != len(y[0]) or not (np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])) for x, y in zip(a, b))


def tool_edges(lists, n_p):
    """Edges between a tool slot and an object slot, over the batch."""
    return sum(int(((r < n_p) != (s < n_p)).sum()) for r, s in lists)


@pytest.mark.gpu
@pytest.mark.parametrize("name,precision,node_dedup", RUNS)
def test_scripted_call_equals_the_step_loop_bit_for_bit(name, precision, node_dedup):
    c, (pred_ref, state_ref, lists), out = run(name, precision, node_dedup)
    assert lists_differ(lists[0], lists[-1]), "the edge lists of step 0 and of the last step are the same: the case shows nothing"
    contact = [tool_edges(x, c.n_p) for x in lists]
    print(f"{name}: tool-object edges per step: {contact}")
    assert contact[0] == 0 and max(contact) > 0, "the script does not drive the tool into the cloud"
    assert out["pred_seq"].shape == (c.B, c.T, c.n_p, 3) and out["state_final"].shape == c.state0.shape and out["err"].shape == (c.B, c.T)
    assert torch.equal(out["pred_seq"], pred_ref), f"pred_seq differs: max abs {float((out['pred_seq'] - pred_ref).abs().max()):.3e}"
    assert torch.equal(out["state_final"], state_ref)
    assert bool(torch.isfinite(out["pred_seq"]).all()) and engine_model(CASES[name][0], precision, node_dedup).take_status() == 0


def err_float64(pred_seq, gt, obj_mask):
    d = (pred_seq.double() - gt.double()).pow(2).sum(-1).sqrt()
    w = torch.ones_like(d[:, 0]) if obj_mask is None else obj_mask.double()
    return (d * w[:, None]).sum(-1) / w.sum(-1).clamp_min(1)[:, None]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rope50", "granular200", "rope700", "masked"])
def test_error_matches_a_float64_evaluation(name):
    c, _, out = run(name)
    want = err_float64(out["pred_seq"], c.gt, c.obj_mask)
    rel = ((out["err"].double() - want).abs() / want).max()
    print(f"{name}: err vs float64, max relative deviation {float(rel):.3e} (bound {err_bound(c.n_p):.3e})")
    assert bool((want > 0).all()) and float(rel) <= err_bound(c.n_p)
    if name == "masked":
        assert not bool(c.obj_mask.all()) and int(c.obj_mask[1].sum()) == int(c.obj_mask[0].sum()) - 5


@pytest.mark.gpu
def test_error_of_an_empty_sample_is_zero_and_a_null_mask_counts_every_slot():
    c, _, out = run("masked")
    model = engine_model("rope")
    empty = c.obj_mask.clone()
    empty[2] = False
    got = scripted(model, c, obj_mask=empty, return_pred=False, return_state=False)
    assert set(got) == {"err"}
    assert bool((got["err"][2] == 0).all()) and torch.equal(got["err"][:2], out["err"][:2])
    ones = scripted(model, c, obj_mask=torch.ones_like(c.obj_mask), return_state=False)
    null = scripted(model, c, obj_mask=None, return_state=False)
    assert torch.equal(null["err"], ones["err"]) and torch.equal(null["pred_seq"], out["pred_seq"])
    want = err_float64(null["pred_seq"], c.gt, None)
    assert float(((null["err"].double() - want).abs() / want).max()) <= err_bound(c.n_p)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rope300", "rope700"])
def test_two_calls_give_the_same_bits(name):
    c, _, out = run(name)
    again = scripted(engine_model("rope"), c)
    for k in ("err", "pred_seq", "state_final"):
        assert torch.equal(again[k], out[k]), k


@pytest.mark.gpu
def test_outputs_are_optional_and_no_tool_slot_needs_no_script():
    c, _, out = run("rope50", 2)
    model = engine_model("rope", 2)
    only_state = scripted(model, c, gt=None, obj_mask=None, return_pred=False)
    assert set(only_state) == {"state_final"} and torch.equal(only_state["state_final"], out["state_final"])
    # a cloud without tool slots (N == n_p): the scripts may be None, the number of steps then comes from gt
    n = c.n_p
    args = (c.state0[:, :, :n].contiguous(), c.action0[:, :n].contiguous(), None, None, c.attrs[:, :n].contiguous(), c.p_instance, c.phys,
            c.mask[:, :n].contiguous(), c.tool_mask[:, :n].contiguous(), c.thr_sq, c.topk, c.connect, 0)
    free = rollout_scripted(model, *args, variant=c.variant, gt=c.gt, return_state=True)
    state, preds = args[0], []
    for _ in range(c.T):
        edges = aggraph.build_edges(state[:, -1], c.radius, args[7], args[8], c.topk, c.connect, c.variant, max_tools=0)
        preds.append(model(state, args[4], edges, None, c.p_instance, action=torch.zeros_like(args[1]) if preds else args[1],
                           rope_physics_param=c.phys)[0])
        if len(preds) < c.T:
            state = torch.cat([state[:, 1:], preds[-1][:, None]], 1)
    assert torch.equal(free["pred_seq"], torch.stack(preds, 1)) and torch.equal(free["state_final"], state)


@pytest.mark.gpu
def test_scripted_rollout_is_hip_graph_capturable_and_follows_a_rewritten_script():
    c, _, out = run("rope50", 2)
    model = engine_model("rope", 2)
    tool_pos, tool_delta = c.tool_pos.clone(), c.tool_delta.clone()
    call = lambda: scripted(model, c, tool_pos=tool_pos, tool_delta=tool_delta)      # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        got = call()
    for _ in range(3):
        for v in got.values():
            v.fill_(7.0)
        gr.replay()
        torch.cuda.synchronize()
        for k, v in got.items():
            assert torch.equal(v, out[k]), k
    # another script in the same buffers: the tool comes down further along the rope, with other motions
    new_pos = c.tool_pos + torch.tensor([0.3, 0.0, 0.0], device=DEV)
    new_delta = c.tool_delta * 0.5
    want = scripted(model, c, tool_pos=new_pos, tool_delta=new_delta)
    assert not torch.equal(want["pred_seq"], out["pred_seq"])
    tool_pos.copy_(new_pos)
    tool_delta.copy_(new_delta)
    gr.replay()
    torch.cuda.synchronize()
    for k, v in got.items():
        assert torch.equal(v, want[k]), k
    assert model.take_status() == 0


@pytest.mark.gpu
def test_scripted_rollout_does_not_synchronise_the_host():
    c, _, out = run("rope300")
    model = engine_model("rope")
    scripted(model, c)                     # (warm: the scratch buffer exists)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = scripted(model, c)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for k in ("err", "pred_seq", "state_final"):
        assert torch.equal(got[k], out[k]), k


@pytest.mark.gpu
def test_refusals_are_codes_with_messages_and_launch_nothing():
    c = inputs("rope50")
    model = engine_model("rope", 2)
    L, dev = _lib.lib(), torch.device(DEV)
    h = model.handle(dev)
    prm = dict(B=c.B, N=c.N, n_p=c.n_p, n_instance=1, topk=c.topk, connect_tools_all=0, max_tools=c.n_t, variant=_lib.AG_VARIANT_SINGLE, n_steps=c.T)
    need = L.ag_rollout_scripted_workspace_bytes_for(h, ctypes.byref(_lib.ScriptedParams(**prm)))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    pred_seq = torch.full((c.B, c.T, c.n_p, 3), 5.0, device=dev)
    err = torch.full((c.B, c.T), 5.0, device=dev)
    state_final = torch.full_like(c.state0, 5.0)
    mask_u8, tool_u8, obj_u8 = _lib._u8(c.mask), _lib._u8(c.tool_mask), _lib._u8(c.obj_mask)
    good = dict(m=h, state0=c.state0, action0=c.action0, tool_pos=c.tool_pos, tool_delta=c.tool_delta, attrs=c.attrs, p_instance=c.p_instance,
                phys=c.phys, mask=mask_u8, tool_mask=tool_u8, thr_sq=c.thr_sq, gt=c.gt, obj_mask=obj_u8, pred_seq=pred_seq, err=err,
                state_final=state_final, workspace=ws, workspace_bytes=need)
    order = ("state0", "action0", "tool_pos", "tool_delta", "attrs", "p_instance", "phys", "mask", "tool_mask", "thr_sq", "gt", "obj_mask", "pred_seq",
             "err", "state_final", "workspace")

    def refused(code, message, params=None, **change):
        a = dict(good, **change)
        p = None if params == "null" else ctypes.byref(_lib.ScriptedParams(**dict(prm, **(params or {}))))
        ptr = lambda v: v.data_ptr() if isinstance(v, torch.Tensor) else v      # noqa: E731
        rc = L.ag_rollout_scripted(a["m"], p, *[ptr(a[k]) for k in order], a["workspace_bytes"], _lib._stream_ptr(dev))
        assert rc == code, (message, rc, L.ag_last_error())
        with pytest.raises(RuntimeError, match=message):
            _lib.check(rc, "ag_rollout_scripted")

    ARG, WS = -1, -3
    for name in ("m", "state0", "action0", "attrs", "p_instance", "mask", "tool_mask", "thr_sq", "workspace"):
        refused(ARG, "null argument", **{name: None})
    refused(ARG, "null argument", params="null")
    refused(ARG, "null tool script", tool_pos=None)
    refused(ARG, "null tool script", tool_delta=None)
    refused(ARG, "gt and err are given together", err=None)
    refused(ARG, "gt and err are given together", gt=None)
    refused(ARG, "no output", gt=None, err=None, pred_seq=None, state_final=None)
    refused(ARG, r"n_steps=0", params=dict(n_steps=0))
    refused(ARG, r"n_steps=-3", params=dict(n_steps=-3))
    refused(ARG, r"n_p=52 \(<= N=51\)", params=dict(n_p=c.N + 1))
    refused(ARG, r"topk=0 \(1\.\.64\)", params=dict(topk=0))
    refused(ARG, r"topk=65 \(1\.\.64\)", params=dict(topk=65))
    refused(ARG, "bad sizes", params=dict(variant=2))
    refused(ARG, "bad sizes", params=dict(B=0))
    refused(ARG, "phys is null", phys=None)
    refused(WS, f"workspace {need - 1} < ", workspace=ws[:need - 1], workspace_bytes=need - 1)
    torch.cuda.synchronize()
    for out in (pred_seq, err, state_final):
        assert bool((out == 5.0).all()), "a refused call wrote to an output"
    # and the same arguments unchanged are accepted
    rc = L.ag_rollout_scripted(h, ctypes.byref(_lib.ScriptedParams(**prm)), *[good[k].data_ptr() for k in order], need, _lib._stream_ptr(dev))
    assert rc == 0, L.ag_last_error()
    torch.cuda.synchronize()
    assert torch.equal(pred_seq, run("rope50", 2)[2]["pred_seq"])


# ------------------------------------------------------------------------------------------------------ the evaluation driver
def write_dataset(root, g):
    """The fixture in the reference's on-disk format (adaptigraph_amd/load.py)."""
    name = str(g["data_name"])
    prep = os.path.join(root, "preprocess", name)
    os.makedirs(os.path.join(prep, "frame_pairs"))
    eef, obj = [], []
    for e in range(len(g["n_frames"])):
        os.makedirs(os.path.join(root, "sim_data", name, f"{e:06}"))
        with open(os.path.join(root, "sim_data", name, f"{e:06}", "property_params.pkl"), "wb") as f:
            pickle.dump({"particle_radius": 0.03, "stiffness": float(g["stiffness"][e])}, f)
        n = int(g["n_frames"][e])
        eef.append(g["eef_pos"][e, :n])
        obj.append(g["obj_pos"][e, :n])
        for k in range(int(g["n_push"][e])):
            np.savetxt(os.path.join(prep, "frame_pairs", f"{e:06}_{k + 1:02}.txt"), g[f"pairs_{e}_{k + 1}"], fmt="%d")
    with open(os.path.join(prep, "positions.pkl"), "wb") as f:
        pickle.dump({"eef_pos": eef, "obj_pos": obj}, f)


def make_config(root, g):
    ds = configs.dataset_config("rope")
    ds.update(data_dir=os.path.join(root, "sim_data"), prep_data_dir=os.path.join(root, "preprocess"), device=DEV,
              ratio={"train": [0, 0.34], "valid": [0.34, 1.0]},
              datasets=[dict(name="rope", max_nobj=int(g["max_nobj"]), max_nR=int(g["max_nR"]), fps_radius_range=[0.18, 0.22],
                             adj_radius_range=[0.48, 0.52], topk=10, connect_tool_all=False)])
    mat = configs.material_config("rope")
    mat["rope"]["physics_params"][1].update(min=0.0, max=1.0)
    return {"dataset_config": ds, "material_config": mat, "model_config": configs.model_config(),
            "train_config": {"random_seed": 42, "out_dir": os.path.join(root, "log")}, "rollout_config": {"out_dir": os.path.join(root, "rollout")}}


@pytest.fixture()
def dataset(tmp_path):
    g = load_golden("evalrollout_rope")
    write_dataset(str(tmp_path), g)
    return g, make_config(str(tmp_path), g), str(tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [0, 2])
def test_rollout_dataset_scripted_matches_the_step_loop_and_the_reference(dataset, precision):
    g, cfg, root = dataset
    model = engine_model("rope", precision)
    curves = {}
    for scripted_flag in (False, True):
        out = os.path.join(root, f"out{int(scripted_flag)}")
        os.makedirs(out)
        np.random.seed(int(g["seed"]))
        curves[scripted_flag] = er.rollout_dataset(model, DEV, cfg, out, scripted=scripted_flag)
    loop, one_call = curves[False], curves[True]
    assert one_call.shape == loop.shape == g["error_short"].shape
    rel = np.abs(one_call - loop) / np.abs(loop)
    print(f"precision {precision}: scripted vs step loop, max relative deviation {rel.max():.3e} (bound {err_bound(int(g['max_nobj'])):.3e}); "
          f"vs the reference {np.abs(one_call - g['error_short']).max():.3e}")
    assert rel.max() <= err_bound(int(g["max_nobj"]))
    assert np.abs(one_call - g["error_short"]).max() <= 2e-5
    assert np.abs(np.loadtxt(os.path.join(root, "out1", "error_short.txt")) - g["error_short"]).max() <= 2e-5
    for e in (1, 2):
        for k in (1, 2):
            assert np.abs(np.loadtxt(os.path.join(root, "out1", str(e), "short", f"error_{k}.txt")) - g[f"error_{e}_{k}"]).max() <= 2e-5


@pytest.mark.gpu
def test_single_graph_signature_and_config_switch_take_the_scripted_path(dataset, monkeypatch):
    g, cfg, root = dataset
    ds = cfg["dataset_config"]
    model = engine_model("rope", 0)
    np.random.seed(int(g["seed"]))
    pair = g["pairs_1_1"][0]
    graph, fidx = er.construct_graph(ds, cfg["material_config"], g["eef_pos"][1], g["obj_pos"][1], 4, pair, {"rope": g["phys_norm"][1]}, DEV)
    pairs_e1 = g["pair_lists"][g["pair_lists"][:, 0] == 1][:, 1:]
    calls = []
    import adaptigraph_amd.forward_dynamics as fd
    real = fd.rollout_scripted
    monkeypatch.setattr(fd, "rollout_scripted", lambda *a, **k: calls.append(k["variant"]) or real(*a, **k))
    args = (graph, fidx, ds, cfg["material_config"], model, DEV, g["eef_pos"][1], g["obj_pos"][1], pair[3], pair[4],
            er.get_next_pair_or_break_episode_pushes, pairs_e1)
    errs = er.rollout_from_start_graph(*args, scripted=True)
    assert calls == ["single"] and np.abs(np.array(errs) - g["error_1_1"]).max() <= 2e-5
    loop = er.rollout_from_start_graph(*args)
    assert calls == ["single"], "the default is the step loop"
    assert len(loop) == len(errs) and (np.abs(np.array(errs) - np.array(loop)) <= err_bound(int(g["max_nobj"])) * np.abs(np.array(loop))).all()
    # rollout(config, epoch) reads rollout_config["scripted"]
    ck = os.path.join(root, "log", "rope", "checkpoints")
    os.makedirs(ck)
    torch.save({k: torch.from_numpy(v) for k, v in load_golden("weights_seed0").items()}, os.path.join(ck, "model_7.pth"))
    cfg["rollout_config"]["scripted"] = True
    step_error = er.rollout(cfg, 7)
    assert calls == ["single", "single"] and np.abs(step_error - g["error_short"]).max() <= 2e-5
