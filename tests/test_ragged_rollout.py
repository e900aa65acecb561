"""Ragged rollout on the GPU (`ag_rollout_order`, `ag_rollout_ragged`, `DynamicsPredictor.ragged_rollout`): a sample is computed for exactly
repeat[b] model steps and every recorded bit is the plain rollout's.  Everything is compared with torch.equal: graphs of a batch never
interact, so leaving a finished sample out changes nothing that is recorded."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
from adaptigraph_amd import _lib, configs, synth
from adaptigraph_amd import graph as aggraph
from adaptigraph_amd.forward_dynamics import dynamics, dynamics_masked, rollout, rollout_order
from adaptigraph_amd.model import DynamicsPredictor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = {"fast": 2, "bf16x3": 1, "f32": 0}
S = _lib.AG_RAGGED_MAX_STEPS
SENTINEL = 7.25      # what the output rows hold before a call: rows no step records must keep it


def t(x, dtype=None):
    r = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return r if dtype is None else r.to(dtype)


def make_model(weights, material="rope", prec="fast", **options):
    m = DynamicsPredictor(configs.model_config(), configs.material_config(material), configs.dataset_config(material), DEV)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in weights.items()})
    m = m.to(DEV).eval()
    m.set_option("precision", PRECISIONS[prec])
    for name, value in options.items():
        m.set_option(name, value)
    return m


def _ppm(material):
    ppm = configs.ppm_optimizer_stub(material)
    ppm.physics_param = {material: torch.tensor([0.5], device=DEV)}
    return ppm


# ------------------------------------------------------------------------------------------------------------ 1. the ordering
def order_cases(B, rng):
    return {"equal": np.full(B, 9), "zeros": np.zeros(B), "negatives": rng.integers(-4, 3, B), "above_1024": rng.integers(1018, 1032, B),
            "random_0_15": rng.integers(0, 16, B)}


@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 257, 1025, 20000])
def test_order_kernel_is_the_stable_descending_sort_and_the_counts(B):
    """ag_rollout_order against the CPU form of the same arithmetic (a stable torch.sort(descending=True) of the repeats clamped at 0, and the
    per-step counts), word for word, and two calls against each other."""
    rng = np.random.default_rng(B)
    for name, rep in order_cases(B, rng).items():
        rep = torch.from_numpy(rep.astype(np.int32))
        want_order, want_active = rollout_order(rep)
        assert torch.equal(want_order.long(), torch.sort(rep.clamp_min(0), descending=True, stable=True).indices), name
        order, active = rollout_order(rep.to(DEV))
        again = rollout_order(rep.to(DEV))
        assert order.dtype == torch.int32 and active.shape == (S + 1,)
        assert torch.equal(order.cpu(), want_order) and torch.equal(active.cpu(), want_active), (name, B)
        assert torch.equal(order, again[0]) and torch.equal(active, again[1]), (name, B)


# ------------------------------------------------------------------------------------------------------------ the raw rollout
class Case:
    """The inputs of one raw rollout call on the GPU, every sample with its own perturbed cloud, tool pose, tool motion and physics row."""

    def __init__(self, material, n_obj, B, seed, masked=False):
        mm = synth.MATERIALS[material]
        rng = np.random.default_rng(seed)
        g = synth.make_graph_inputs(material, n_obj, B, seed=seed, **(dict(spacing=0.1) if material == "rope" else {}))
        self.n_p, self.n_t, self.B = g["n_p"], g["n_tools"], B
        g["state"][:, :, :n_obj] += rng.normal(0, 0.002, (B, 1, n_obj, 3)).astype(np.float32)
        g["state"][:, :, self.n_p:] += rng.normal(0, 0.05, (B, 1, 1, 3)).astype(np.float32)
        g["action"][:, self.n_p:] = rng.normal(0, 0.08, (B, 1, 3)).astype(np.float32)
        g["phys"][:] = rng.uniform(0.3, 0.9, (B, 1)).astype(np.float32)
        self.topk, self.connect = mm["topk"], mm["connect_tools_all"]
        self.thr = aggraph.threshold_sq(mm["radius"], B, torch.device(DEV), _lib.AG_VARIANT_BATCH)
        self.per_sample = [t(g[k]) for k in ("state", "action", "attrs", "p_instance", "phys", "mask", "tool_mask")]
        self.obj_mask = t(g["mask"][:, :self.n_p]) if masked else None
        self.height = _lib.AG_HEIGHT_MASKED_MEAN if masked else _lib.AG_HEIGHT_MIN

    def _call(self, m, tensors, obj_mask, rep, n_steps, **kw):
        out = torch.full((self.B, self.n_p, 3), SENTINEL, device=DEV)
        res = rollout(m, *tensors, self.thr, rep, n_steps, self.topk, self.connect, self.n_t, self.height, obj_mask, 0.0, return_state=True, out=out, **kw)
        return res[0].clone(), res[1].clone()

    def plain(self, m, rep, n_steps):
        return self._call(m, self.per_sample, self.obj_mask, rep, n_steps)

    def ragged(self, m, rep, order=None, active=None, out_index="order"):
        """The batch gathered into `order` (default: ag_rollout_order's), run with `active` (default: its counts), scattered through out_index."""
        dev_order, dev_active = rollout_order(rep)
        order = dev_order if order is None else order
        active = dev_active.cpu() if active is None else active
        n_steps = int(torch.count_nonzero(active[:-1]))
        sel = order.long()
        tensors = [x.index_select(0, sel) for x in self.per_sample]
        obj_mask = None if self.obj_mask is None else self.obj_mask.index_select(0, sel)
        return self._call(m, tensors, obj_mask, rep.index_select(0, sel), n_steps, order=order if out_index == "order" else out_index, active=active)


def scramble_workspaces():
    torch.cuda.synchronize()
    for buf in _lib._WS.values():
        buf.random_(0, 256)


def check_against_plain(m, case, rep_list):
    """out_seq = the plain call's on the unsorted batch (rows of repeat 0 untouched), state_final[b] = the plain call's after repeat[b] steps, status 0;
    the ragged call runs on workspaces full of random bytes."""
    rep = torch.tensor(rep_list, dtype=torch.int32, device=DEV)
    want_seq, _ = case.plain(m, rep, max(rep_list))
    want_fin = torch.empty_like(case.per_sample[0])
    for r in sorted(set(rep_list)):
        rows = torch.nonzero(rep == r)[:, 0]
        want_fin[rows] = case.plain(m, rep, r)[1][rows]
    case.ragged(m, rep)
    scramble_workspaces()
    got_seq, got_fin = case.ragged(m, rep)
    assert torch.equal(got_seq, want_seq)
    untouched = torch.tensor([r < 1 for r in rep_list], device=DEV)
    assert bool((got_seq[untouched] == SENTINEL).all()) and bool(torch.isfinite(got_seq).all())
    assert torch.equal(got_fin, want_fin)
    assert m.take_status() == 0


RAW_CASES = [(p, s, {}) for p in PRECISIONS for s in (0, 1)] + [
    ("fast", s, o) for s in (0, 1) for o in ({"node_dedup": 2}, {"node_dedup": 0}, {"self_edges": 0}, {"node_stationary": 0})]


@pytest.mark.parametrize("prec,shared,options", RAW_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_ragged_rollout_is_bitwise_the_plain_rollout(weights, prec, shared, options):
    """rope-60 + 1 tool (N = 61), B = 9, repeats [3,0,5,1,3,5,0,1,3]: prefix lengths 7, 5, 5, 2, 2."""
    m = make_model(weights, "rope", prec, shared_state=shared, **options)
    rep = [3, 0, 5, 1, 3, 5, 0, 1, 3]
    assert rollout_order(torch.tensor(rep, dtype=torch.int32))[1][:6].tolist() == [7, 5, 5, 2, 2, 0]
    check_against_plain(m, Case("rope", 60, 9, seed=11), rep)


@pytest.mark.parametrize("shared", [0, 1])
@pytest.mark.parametrize("name", ["single_running_sample", "b33", "cloth81_connect_tools_all", "granular80_five_tools_top20", "masked_mean"])
def test_ragged_rollout_edges(weights, shared, name):
    rng = np.random.default_rng(5)
    material, n_obj, rep, masked = {
        "single_running_sample": ("rope", 60, [1, 4], False),                        # steps 2..4 run one sample; shared-state B1 = 2
        "b33": ("rope", 60, rng.integers(0, 4, 33).tolist(), False),                # prefixes whose B N is no multiple of 32
        "cloth81_connect_tools_all": ("cloth", 81, [2, 3, 1, 3, 0], False),
        "granular80_five_tools_top20": ("granular", 80, [1, 3, 2, 2, 3, 1], False),
        "masked_mean": ("rope", 60, [2, 1, 3, 3, 0, 2], True)}[name]
    if name == "b33":
        assert any((61 * n) % 32 for n in rollout_order(torch.tensor(rep, dtype=torch.int32))[1][:3].tolist())
    m = make_model(weights, material, "fast", shared_state=shared)
    check_against_plain(m, Case(material, n_obj, len(rep), seed=21, masked=masked), rep)


def profiled(m, fn):
    """fn() under the engine's per-launch counters -> (result, edges the edge encoder walked WITHOUT the class rows of elided self-loops it adds per
    launch, edge-encoder launches)."""
    L, h = _lib.lib(), m.handle(torch.device(DEV))
    _lib.check(L.ag_profile_enable(h, 1), "ag_profile_enable")
    res = fn()
    ms, cnt, edges = (ctypes.c_double * 6)(), (ctypes.c_int64 * 6)(), ctypes.c_int64()
    _lib.check(L.ag_profile_read(h, ms, cnt, ctypes.byref(edges)), "ag_profile_read")
    _lib.check(L.ag_profile_enable(h, 0), "ag_profile_enable")
    launches = cnt[_lib.KERNEL_CLASSES.index("edge_encode")]
    per_launch = 64 if m.get_option("self_edges") else 0      # AG_SELF_ROWS
    return res, edges.value - launches * per_launch, launches


@pytest.mark.parametrize("shared", [0, 1])
def test_equal_repeats_do_the_plain_calls_work(weights, shared):
    """All repeats equal: nothing retires early — the same outputs and the same number of encoded edges as the plain call."""
    m = make_model(weights, "rope", "fast", shared_state=shared)
    case = Case("rope", 60, 6, seed=3)
    rep = torch.full((6,), 3, dtype=torch.int32, device=DEV)
    (want, _), e_plain, n_plain = profiled(m, lambda: case.plain(m, rep, 3))
    (got, _), e_ragged, n_ragged = profiled(m, lambda: case.ragged(m, rep))
    assert torch.equal(got, want) and (e_ragged, n_ragged) == (e_plain, n_plain) and e_plain > 0 and n_plain == 3
    assert m.take_status() == 0


def test_retired_samples_cost_no_edges(weights):
    """B = 8, repeats [5,5,5,5,1,1,1,1]: the ragged call encodes exactly the edges of the plain call on the long half (5 steps) plus the plain call
    on the short half (1 step), fewer than the plain call on all eight (counts without the rows the counter adds per launch)."""
    m = make_model(weights, "rope", "fast")
    case = Case("rope", 60, 8, seed=4)
    rep = torch.tensor([5, 5, 5, 5, 1, 1, 1, 1], dtype=torch.int32, device=DEV)
    halves = []
    for rows, steps in ((slice(0, 4), 5), (slice(4, 8), 1)):
        half = Case("rope", 60, 4, seed=4)
        half.per_sample = [x[rows].contiguous() for x in case.per_sample]
        halves.append(profiled(m, lambda: half.plain(m, rep[rows].contiguous(), steps)))
    (want, _), e_all, n_all = profiled(m, lambda: case.plain(m, rep, 5))
    (got, _), e_ragged, n_ragged = profiled(m, lambda: case.ragged(m, rep))
    assert torch.equal(got, want) and torch.equal(got, torch.cat([h[0][0] for h in halves]))
    print(f"edges encoded: ragged {e_ragged} ({n_ragged} launches), plain {e_all} ({n_all}), halves {halves[0][1]} + {halves[1][1]}")
    assert n_ragged == 5 and e_ragged == halves[0][1] + halves[1][1]
    assert 0 < e_ragged < e_all


@pytest.mark.parametrize("shared", [0, 1])
def test_misuse_is_flagged_and_the_next_call_is_clean(weights, shared):
    m = make_model(weights, "rope", "fast", shared_state=shared)
    case = Case("rope", 60, 9, seed=11)
    rep_list = [3, 0, 5, 1, 3, 5, 0, 1, 3]
    rep = torch.tensor(rep_list, dtype=torch.int32, device=DEV)
    want, _ = case.plain(m, rep, 5)
    assert m.take_status() == 0

    def status():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return m.take_status()

    identity = torch.arange(9, dtype=torch.int32, device=DEV)
    case.ragged(m, rep, order=identity)                     # the unsorted batch with the sorted counts
    assert status() & _lib.AG_STATUS_ORDER
    bad = rollout_order(rep)[0].clone()
    bad[2] = 9                                              # an output row outside the batch
    got, _ = case.ragged(m, rep, out_index=bad)
    assert status() & _lib.AG_STATUS_ORDER
    skipped = int(rollout_order(rep)[0][2])                 # the sample whose row was out of range: nothing of it is written anywhere
    assert bool((got[skipped] == SENTINEL).all()) and bool((got[rep < 1] == SENTINEL).all())
    with pytest.warns(RuntimeWarning, match="ragged rollout"):
        case.ragged(m, rep, order=identity)
        m.take_status()
    got, _ = case.ragged(m, rep)
    assert m.take_status() == 0 and torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------------ 6. the Python drivers
@pytest.mark.parametrize("shared", [0, 1])
@pytest.mark.parametrize("name", ["dyn_rope60", "dyn_rope60_look2", "dyn_granular80", "dyn_cloth81", "dynmask_granular60", "dynmask_rope40"])
def test_drivers_with_the_attribute_on_equal_the_attribute_off(weights, name, shared):
    g = load_golden(name)
    material = str(g["material"])
    m = make_model(weights, material, "fast", shared_state=shared)
    assert m.ragged_rollout is False and "ragged_rollout" not in vars(m)

    def run():
        if name.startswith("dynmask_"):
            return dynamics_masked(t(g["state_init"]), t(g["state_mask"]), t(g["action"]), m, DEV, _ppm(material))["state_seqs"].clone()
        return dynamics(t(g["state"]), t(g["action"]), m, DEV, _ppm(material))["state_seqs"].clone()

    want = run()
    m.ragged_rollout = True
    got = run()
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert m.take_status() == 0


def test_driver_takes_one_host_read_and_hands_long_pushes_to_the_plain_call(weights, monkeypatch):
    """dynamics() with the attribute on: every rollout of a normal batch is the ragged entry point; a push of more than AG_RAGGED_MAX_STEPS steps
    makes its column's last count non-zero and the column goes to the plain call."""
    from adaptigraph_amd import forward_dynamics as fd
    m = make_model(weights, "rope", "fast")
    m.ragged_rollout = True
    state, act = synth.make_mpc_inputs("rope", 60, 6, n_look=2, seed=2, len_lo=1, len_hi=3.9, spacing=0.1)
    names = []
    real = _lib.call
    monkeypatch.setattr(fd._lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    dynamics(t(state), t(act), m, DEV, _ppm("rope"))
    assert [n for n in names if n.startswith("ag_rollout")] == ["ag_rollout_order"] * 2 + ["ag_rollout_ragged"] * 2
    assert names.count("ag_model_status") == 1
    order, active = rollout_order(torch.tensor([2, S + 1, 0], dtype=torch.int32, device=DEV))
    assert order.tolist() == [1, 0, 2] and int(active[-1]) == 1 and fd._ragged_steps(active.cpu()) is None
    assert fd._ragged_steps(rollout_order(torch.tensor([2, S, 0], dtype=torch.int32))[1]) == S


@pytest.mark.parametrize("shared_state", [0, 1])
def test_chunked_planner_with_the_attribute_on(weights, shared_state):
    """`ChunkedPlanner` at (C, S) = (3, 8) on rope-60, the set-up of test_chunked_planner_is_the_loop_of_planners: the planned action, the best rollout and
    its reward with ragged rollouts equal those without."""
    from adaptigraph_amd import mpc
    from test_chunked_plan import planner_setup
    cfg, cost, state, samples, C, _, push, _ = planner_setup(weights, shared_state)
    model = cfg["model_rollout_fn"].keywords["model"]
    res = []
    for on in (False, True):
        model.ragged_rollout = on
        planner = mpc.ChunkedPlanner(dict(cfg, n_update_iter=2, n_chunk=C, cost=cost, push_length=push))
        res.append(planner.trajectory_optimization(state, samples[0][0], samples=samples[:2]))
    off, on = res
    assert torch.equal(on["act_seq"], off["act_seq"])
    assert torch.equal(on["best_model_output"]["state_seqs"], off["best_model_output"]["state_seqs"])
    assert torch.equal(on["best_eval_output"]["reward_seqs"], off["best_eval_output"]["reward_seqs"])
    assert model.take_status() == 0


# ------------------------------------------------------------------------------------------------------------ 7. capture
@pytest.mark.parametrize("shared", [0, 1])
def test_ragged_rollout_is_hip_graph_capturable(weights, shared):
    """One ragged call captured on a single stream, replayed three times on rewritten inputs with the same repeats: the eager results.
    active_per_step is read when the call is enqueued, so the graph holds the launches of those counts."""
    m = make_model(weights, "rope", "fast", shared_state=shared)
    rep_list = [4, 4, 3, 2, 2, 1, 0]
    B = len(rep_list)
    cases = [Case("rope", 60, B, seed=30 + k) for k in range(4)]
    rep = torch.tensor(rep_list, dtype=torch.int32, device=DEV)      # already in order: the identity is its order
    order, active = rollout_order(rep)
    assert order.tolist() == list(range(B))
    active = active.cpu()
    c0 = cases[0]
    static = [x.clone() for x in c0.per_sample]
    out = torch.zeros((B, c0.n_p, 3), device=DEV)

    def run():
        return rollout(m, *static, c0.thr, rep, 4, c0.topk, c0.connect, c0.n_t, c0.height, None, 0.0, return_state=True, out=out, order=order, active=active)

    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, fin = run()
    for k in (1, 2, 3):
        for dst, src in zip(static, cases[k].per_sample):
            dst.copy_(src)
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone(), fin.clone()
        want = cases[k].ragged(m, rep)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), k
    assert m.take_status() == 0
