"""The persistent kernels of the inference engine at every trip count per workgroup.

A workgroup of an MLP kernel handles block blockIdx.x, then blockIdx.x + gridDim.x, ...; the number of blocks one workgroup walks (`n_i`) is what
the prologues, epilogues, LDS rings and tail blocks of `edge_encode_ws_kernel` and `node_update_nws_kernel`, and the tile loops of the streaming
kernels, depend on.  The grids come from the option "max_blocks" (default 2 x #CUs), so at the suite's small shapes every workgroup walks 0 or 1
block.  Here "max_blocks" is chosen, per case, from the case's block count, so that small shapes reach n_i = 1, 2, 3, 4, 7 (ring periods 2 and 3,
and the period + 1), unequal trips within one launch, a single workgroup walking everything, each with a full and with a partial last block.

1. (CPU) `trip_plan` mirrors how each launcher turns "max_blocks" into a grid, and the case table is held to the trip counts it must reach.
2. (GPU) the forward on every kernel path of `resolve_path` x the case table: bit-equal to the default grid, within TOL_BY_PREC of the float64
   step, status 0, repeatable — on workspaces filled with random bytes.
3. (GPU) the rollout drivers at a single workgroup and at unequal trips, bit for bit against the default grid.

Rows never interact across workgroups (no kernel reduces across them), so a row's bits cannot depend on the grid: every comparison between grids
is torch.equal.  The forward runs on a caller's CSR, where no self-loop is elided (AgFwdArgs::self_rows = 0): the per-edge table has exactly E
rows in section 2; the rollouts of section 3 run with "self_edges" 1 (AG_SELF_ROWS more rows per launch) unless a test says otherwise.
Inputs are those of tests/test_model_configs.py, trimmed to their first samples, padded with isolated invalid slots behind the tool (rows), or
with trailing object slots declared invalid before the oracle builds the edge lists (edges), to reach the remainders 0, 1 and 31 mod 32."""
import collections
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib
from adaptigraph_amd.forward_dynamics import dynamics
from oracle import ag_oracle as ago
from test_gpu_parity import DEV, PRECISIONS, TOL_BY_PREC, csr_from_lists, t
from test_model_configs import RADIUS, TOPK, cfg_id, config_inputs, engine_forward, graph_inputs, make_model, ref64, ref64_of, weights_np
from test_ragged_rollout import Case, _ppm, check_against_plain, scramble_workspaces
from test_ragged_rollout import make_model as case_model
from test_scripted_rollout import inputs as scripted_inputs, scripted, step_loop


# ------------------------------------------------------------------------------------------------------ the launchers, mirrored
def header_int(file, name):
    return int(re.search(r"#define %s (\d+)" % name, open(os.path.join(_lib.CSRC, file)).read()).group(1))


MLP_THREADS = header_int("ag_common.h", "AG_MLP_THREADS")
ROWS_PER_BLOCK = 32 * (MLP_THREADS // 64)                     # AG_ROWS_PER_BLOCK (ag_common.h:31): a row tile of the streaming kernels
MLP_WG_PER_CU = 512 // MLP_THREADS                            # AG_MLP_WG_PER_CU (ag_common.h:32)
H3_WG_PER_CU = header_int("ag_edge_encode.hip", "AG_H3_WG_PER_CU")
SELF_ROWS = header_int("ag_common.h", "AG_SELF_CLASSES") * header_int("ag_common.h", "AG_SELF_REPL")      # AG_SELF_ROWS
WS_BLOCK = 32                                                 # rows / edges of a block of the two weight-stationary kernels
DEFAULT_MAX_BLOCKS = MLP_WG_PER_CU * 256                      # ag_model.hip:126 on the MI355X's 256 CUs (the GPU tests read the model's own value)


def ceil_div(a, b):
    return (a + b - 1) // b


def grid_for(rows, max_blocks):
    """ag_mlp_dev.h:817."""
    tiles = ceil_div(rows, ROWS_PER_BLOCK)
    return (tiles if tiles > 0 else 1) if tiles < max_blocks else max_blocks


def ws_blocks(call_blocks, model_blocks):
    """setup_args, ag_engine.hip:133-134: `call_blocks` is the call's (a rollout part's) share of the model's "max_blocks"."""
    full, share = model_blocks // MLP_WG_PER_CU, call_blocks // MLP_WG_PER_CU * 3 // 2
    return max(share, 1) if share < full else max(full, 1)


def deal(blocks, grid):
    """Blocks per workgroup of a static grid stride (blockIdx, blockIdx + grid, ...), workgroups without a block left out -> sorted list."""
    return sorted((n for n in ((blocks - b + grid - 1) // grid for b in range(grid)) if n > 0), reverse=True)


WS_KERNELS = ("node_update_ws", "edge_encode_ws")
STREAM_KERNELS = ("node_encode", "node_update", "edge_encode", "edge_encode_h3")


def trip_plan(rows, edges, max_blocks, model_blocks=None, self_rows=0):
    """Trips per workgroup of every persistent kernel of one model step over `rows` node rows and `edges` edges, kernel -> sorted list.
    node_encode (per node) and the streaming node_update: grid_for(B N, max_blocks) over 128-row tiles, static stride (ag_node_encode.hip:192,
    ag_node_update.hip:207).  edge_encode<PrecF32 | PrecB3>: grid_for(E, max_blocks) (ag_edge_encode.hip:186-187); <PrecH3>: max_blocks /
    AG_MLP_WG_PER_CU (at least 1) x AG_H3_WG_PER_CU (:181, :185).  These three claim their tiles from an atomic counter (TileQueue), so the list is the
    static deal of the same grid: the sum is exact, and some workgroup walks at least the largest entry; with one workgroup it is exact.
    node_update_nws_kernel: max(max_blocks / AG_MLP_WG_PER_CU, 1) workgroups over ceil(B N / 32) blocks (ag_node_update_ws.hip:276-277).
    edge_encode_ws_kernel: `ws_blocks` workgroups over ceil((E + self_rows) / 32) blocks (ag_edge_encode_ws.hip:477-481)."""
    model_blocks = max_blocks if model_blocks is None else model_blocks
    e = edges + self_rows
    node_tiles, edge_tiles = ceil_div(rows, ROWS_PER_BLOCK), ceil_div(e, ROWS_PER_BLOCK)
    node_blk, edge_blk = ceil_div(rows, WS_BLOCK), ceil_div(e, WS_BLOCK)
    h3_blocks = max(max_blocks // MLP_WG_PER_CU, 1) * H3_WG_PER_CU
    return {"node_encode": deal(node_tiles, grid_for(rows, max_blocks)),
            "node_update": deal(node_tiles, grid_for(rows, max_blocks)),
            "edge_encode": deal(edge_tiles, grid_for(e, max_blocks)),
            "edge_encode_h3": deal(edge_tiles, grid_for(e, h3_blocks)),
            "node_update_ws": deal(node_blk, min(node_blk, max(max_blocks // MLP_WG_PER_CU, 1))),
            "edge_encode_ws": deal(edge_blk, min(edge_blk, ws_blocks(max_blocks, model_blocks)))}


def rollout_parts(B, want):
    """rollout_parts / part_range, ag_drivers.hip:85-96 -> samples per part."""
    parts = min(max(want, 1), 4)
    while parts > 1 and B // parts < 8:
        parts -= 1
    per = ceil_div(B, parts)
    return [min(per, B - k * per) for k in range(parts)]


def rollout_node_plans(B, N, streams, max_blocks):
    """node_update_nws_kernel of every part of an ag_rollout call: part_blocks = max(max_blocks / parts, 1) (ag_drivers.hip:441)."""
    parts = rollout_parts(B, streams)
    part_blocks = max(max_blocks // len(parts), 1)
    return [trip_plan(b * N, 0, part_blocks, max_blocks)["node_update_ws"] for b in parts]


def is_unequal(trips):
    """Workgroups of one launch with n_i and n_i - 1 blocks, both at work."""
    return len(set(trips)) == 2 and max(trips) - min(trips) == 1 and min(trips) >= 1


def solve(kernel, rows, edges, want):
    """The smallest "max_blocks" at which `kernel` reaches `want`: an int k (the longest trip is k — ceil(blocks / k) workgroups), "unequal" or
    "single" (one workgroup walks everything)."""
    for mb in range(1, 2 * max(ceil_div(rows, WS_BLOCK), ceil_div(edges, WS_BLOCK)) + 2):
        trips = trip_plan(rows, edges, mb)[kernel]
        if (want == "single" and len(trips) == 1) or (want == "unequal" and is_unequal(trips)) or (want == max(trips) and want != 1) or \
                (want == 1 and max(trips) == 1 and len(trips) > 1):
            return mb
    raise AssertionError((kernel, rows, edges, want))


# ------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def trip_inputs(shape, B, n_extra, masked):
    """The first B samples of a shape of tests/test_model_configs.py; the last masked[0] object slots of sample B - 1 and the last masked[1] of
    sample 0 made invalid object slots (mask False, zero attributes and positions, as the padded slots of the shape) BEFORE the oracle builds the
    edge lists; `n_extra` isolated invalid slots (all zero, no edge) appended behind the tool of every sample.  Never written to."""
    g0 = graph_inputs(shape)
    n_obj, n_p = g0["n_obj"], g0["n_p"]
    state, attrs, action, mask, tool = (g0[k][:B].copy() for k in ("state", "attrs", "action", "mask", "tool_mask"))
    gone = np.zeros((B, n_p), bool)
    gone[B - 1, n_obj - masked[0]:n_obj] = True
    gone[0, n_obj - masked[1]:n_obj] = True
    if gone.any():
        for b, i in zip(*np.nonzero(gone)):
            mask[b, i] = False
            attrs[b, i] = 0
            state[b, :, i] = 0
        n_rel, recv, send = ago.build_edges(state[:, -1], RADIUS, mask, tool, TOPK, False, "batch")
    else:
        n_rel, recv, send = g0["n_rel"][:B], g0["recv"][:B], g0["send"][:B]
    if n_extra:
        state = np.concatenate([state, np.zeros(state.shape[:2] + (n_extra, 3), np.float32)], 2)
        attrs = np.concatenate([attrs, np.zeros((B, n_extra, 2), np.float32)], 1)
        action = np.concatenate([action, np.zeros((B, n_extra, 3), np.float32)], 1)
        mask, tool = (np.concatenate([x, np.zeros((B, n_extra), bool)], 1) for x in (mask, tool))
    g = dict(state=state, attrs=attrs, action=action, mask=mask, tool_mask=tool, n_p=n_p, n_obj=n_obj, n_tools=g0["n_tools"], n_rel=n_rel, recv=recv,
             send=send, lists=[(recv[b, :n], send[b, :n]) for b, n in enumerate(n_rel)], gone=gone, rows=B * attrs.shape[1], edges=int(n_rel.sum()))
    return g


def trip_config_inputs(key, phys_dim, n_inst):
    shape, B, _, _ = key
    phys, p_inst = config_inputs(shape, phys_dim, n_inst)
    p_inst = p_inst[:B].copy()
    p_inst[trip_inputs(*key)["gone"]] = 0
    return phys[:B], p_inst


@functools.lru_cache(maxsize=None)
def trip_ref(key, wname, cfg):
    """(pos, motion) of the float64 step on the inputs `key`.  Isolated slots behind the tool change no other node's result, so inputs that are
    only trimmed and padded take the rows of the cached reference of tests/test_model_configs.py (held to 1e-12 by the table test); inputs with
    other edge lists get a float64 step of their own."""
    shape, B, n_extra, masked = key
    if masked == (0, 0):
        pos, mot = ref64(shape, wname, cfg)
        return pos[:B], mot[:B]
    phys, p_inst = trip_config_inputs(key, cfg[0], cfg[1])
    return ref64_of(weights_np(wname, cfg[0]), trip_inputs(shape, B, 0, masked), phys, p_inst, cfg[2])


@functools.lru_cache(maxsize=None)
def masked_for(shape, B, remainder):
    """The fewest trailing object slots to declare invalid — of the last sample, then of sample 0 as well — for an edge count of `remainder`
    mod 32 (every count comes from the oracle's builder on the masked cloud)."""
    for first in range(16):
        for last in range(48):
            if trip_inputs(shape, B, 0, (last, first))["edges"] % WS_BLOCK == remainder:
                return (last, first)
    raise AssertionError((shape, B, remainder))


# 3 x (101 + 38) = 417 = 13 x 32 + 1 and 3 x (101 + 48) = 447 = 13 x 32 + 31 rows; 2 x (101 + 123) = 448 = 14 x 32: fourteen blocks each, which
# deal as 1 (14 workgroups), 2 (7), 3 | 2 (5), 4 | 3 (4), 7 (2) and 14 (1)
NODE_INPUTS = {"r1": ("rope93", 3, 38, (0, 0)), "r31": ("rope93", 3, 48, (0, 0)), "r0": ("rope93", 2, 123, (0, 0))}
STREAM_INPUTS = ("rope150x5", 5, 0, (0, 0))       # 755 rows = 5 tiles + 115 rows, 5923 edges = 46 tiles + 35 edges
WANTS = (1, 2, 3, 4, 7, "unequal", "single")
FEW_WANTS = (3, "single")
TripCase = collections.namedtuple("TripCase", "name key max_blocks")      # max_blocks None: the model's default


def _names():
    names = []
    for kernel, tags in (("nws", tuple(NODE_INPUTS)), ("ews", ("e1", "e0", "e31"))):
        for tag in tags:
            names += [f"{kernel}-{tag}-{w}" for w in (FEW_WANTS if tag.endswith("31") else WANTS)]
    names += ["stream-default", "stream-mb1", "stream-mb2", "stream-mb3"]
    names += [f"stream-edge_encode-{w}" for w in (2, 3)]      # (edge_encode<PrecH3> has the same grids there: an even "max_blocks")
    return names


CASE_NAMES = _names()


@functools.lru_cache(maxsize=None)
def trip_cases():
    """name -> TripCase.  "max_blocks" of every case comes from the case's own block count (`solve`); the edge counts are the oracle's."""
    edge_inputs = {f"e{r}": ("rope93", 3, 0, masked_for("rope93", 3, r)) for r in (1, 0, 31)}
    cases = []
    for kernel, short, table in (("node_update_ws", "nws", NODE_INPUTS), ("edge_encode_ws", "ews", edge_inputs)):
        for tag, key in table.items():
            g = trip_inputs(*key)
            cases += [TripCase(f"{short}-{tag}-{w}", key, solve(kernel, g["rows"], g["edges"], w)) for w in (FEW_WANTS if tag.endswith("31") else WANTS)]
    g = trip_inputs(*STREAM_INPUTS)
    cases += [TripCase("stream-default", STREAM_INPUTS, None)] + [TripCase(f"stream-mb{v}", STREAM_INPUTS, v) for v in (1, 2, 3)]
    cases += [TripCase(f"stream-edge_encode-{w}", STREAM_INPUTS, solve("edge_encode", g["rows"], g["edges"], w)) for w in (2, 3)]
    assert [c.name for c in cases] == CASE_NAMES
    return {c.name: c for c in cases}


def case_plan(c):
    g = trip_inputs(*c.key)
    return trip_plan(g["rows"], g["edges"], DEFAULT_MAX_BLOCKS if c.max_blocks is None else c.max_blocks)


# ------------------------------------------------------------------------------------------------------ 1. the trip plan (CPU)
def test_mirrored_launch_constants_and_grids():
    assert (MLP_THREADS, ROWS_PER_BLOCK, MLP_WG_PER_CU, H3_WG_PER_CU, SELF_ROWS) == (256, 128, 2, 2, 64)
    assert [grid_for(r, 512) for r in (0, 1, 128, 129, 128 * 600)] == [1, 1, 1, 2, 512] and grid_for(1000, 3) == 3
    assert (ws_blocks(512, 512), ws_blocks(1, 1), ws_blocks(2, 2), ws_blocks(128, 512), ws_blocks(1, 2)) == (256, 1, 1, 96, 1)
    assert deal(14, 4) == [4, 4, 3, 3] and deal(3, 8) == [1, 1, 1] and deal(57, 1) == [57]
    p = trip_plan(755, 5923, 1)
    assert p["node_update"] == [6] and p["edge_encode"] == [47] and p["edge_encode_h3"] == [24, 23] and p["node_update_ws"] == [24] and p["edge_encode_ws"] == [186]
    assert rollout_parts(33, 4) == [9, 9, 9, 6] and rollout_parts(33, 2) == [17, 16] and rollout_parts(20, 4) == [10, 10] and rollout_parts(9, 0) == [9]


def test_case_table_reaches_every_trip_count():
    """Per kernel, the trips per workgroup the table reaches (printed once), held to what the file's docstring promises."""
    cases = trip_cases()
    plans = {name: case_plan(c) for name, c in cases.items()}
    sizes = {name: trip_inputs(*c.key) for name, c in cases.items()}
    for kernel, prefix in zip(WS_KERNELS + STREAM_KERNELS, ("nws", "ews") + ("stream",) * 4):      # (the cases made for the kernel; the rest in the summary line)
        print(kernel)
        for name, c in cases.items():
            g, trips = sizes[name], plans[name][kernel]
            if name.startswith(prefix):
                print(f"  {name:24s} rows {g['rows']:4d} edges {g['edges']:5d} max_blocks {str(c.max_blocks):>4s}: {len(trips):3d} workgroups, "
                      f"trips x workgroups {dict(collections.Counter(trips))}")
        print(f"  trips reached over the {len(cases)} cases: {sorted(set().union(*(plans[n][kernel] for n in cases)))}")
    for kernel, what in zip(WS_KERNELS, ("rows", "edges")):
        for partial in (False, True):
            reached = [plans[n][kernel] for n in cases if (sizes[n][what] % WS_BLOCK != 0) == partial]
            for k in (1, 2, 3, 4, 7):
                assert any(k in trips for trips in reached), (kernel, partial, k)
            assert any(is_unequal(trips) for trips in reached), (kernel, partial, "unequal")
            assert any(len(trips) == 1 and trips[0] > 7 for trips in reached), (kernel, partial, "single")
        assert {1, 31} <= {sizes[n][what] % WS_BLOCK for n in cases}, (kernel, "remainders 1 and 31")
    for kernel, what in zip(STREAM_KERNELS, ("rows", "rows", "edges", "edges")):
        longest = {max(plans[n][kernel]) for n in cases}
        assert {1, 2, 3} <= longest and max(longest) >= 5, (kernel, sorted(longest))
        assert any(sizes[n][what] % ROWS_PER_BLOCK for n in cases) and any(c.max_blocks == 1 for c in cases.values())
        assert any(len(plans[n][kernel]) == 1 and plans[n][kernel][0] >= 5 for n in cases if cases[n].max_blocks == 1) or kernel == "edge_encode_h3"
    assert plans["stream-mb1"]["edge_encode_h3"] == [24, 23]      # (one CU's worth: AG_H3_WG_PER_CU workgroups)
    for c in cases.values():
        assert c.max_blocks is None or c.max_blocks >= 1
    # the rollouts of section 3: one workgroup per part at "max_blocks" 2, unequal trips in every part at 64 (33 samples of 61 rows)
    for streams in (1, 2, 4):
        assert len(rollout_parts(33, streams)) == streams
        assert all(len(trips) == 1 for trips in rollout_node_plans(33, 61, streams, 2)), streams
        assert all(is_unequal(trips) for trips in rollout_node_plans(33, 61, streams, 64)), streams
    assert is_unequal(trip_plan(9 * 61, 0, 16)["node_update_ws"]) and is_unequal(trip_plan(2 * 301, 0, 20)["node_update_ws"])


def test_padding_behind_the_tool_leaves_the_float64_reference_alone():
    """The cached reference of the unpadded shape is used for inputs with isolated slots appended: the float64 step on the padded inputs gives
    the same rows (1e-12: a BLAS may block a taller matrix differently)."""
    key, cfg = NODE_INPUTS["r1"], (1, 1, 3)
    g = trip_inputs(*key)
    assert g["state"].shape == (3, 4, 139, 3) and g["rows"] == 417 and g["edges"] == 1813 and not g["gone"].any()
    phys, p_inst = trip_config_inputs(key, 1, 1)
    pos, mot = ref64_of(weights_np("weights_seed0", 1), g, phys, p_inst, 3)
    want_pos, want_mot = trip_ref(key, "weights_seed0", cfg)
    assert np.abs(mot - want_mot).max() <= 1e-12 and np.abs(pos - want_pos).max() <= 1e-12
    e = trip_inputs("rope93", 3, 0, masked_for("rope93", 3, 1))
    assert e["edges"] % 32 == 1 and e["gone"].any() and not e["mask"][e["gone"].nonzero()].any() and e["rows"] == 303


# ------------------------------------------------------------------------------------------------------ 2. forward: every path x the plan (GPU)
#        name                   (precision, (phys_dim, n_instance, pstep), weights, options)
PATHS = {"f32": ("f32", (1, 1, 3), "weights_seed0", {}),
         "f32-dedup2": ("f32", (1, 1, 3), "weights_seed0", {"node_dedup": 2}),
         "bf16x3-node_ws": ("bf16x3", (1, 1, 3), "weights_seed0", {"node_stationary": 1}),
         "bf16x3-node_stream": ("bf16x3", (1, 1, 3), "weights_seed0", {"node_stationary": 0}),
         "bf16x3-dedup2": ("bf16x3", (1, 1, 3), "weights_seed0", {"node_dedup": 2}),
         "fast-h3ws": ("fast", (1, 1, 3), "weights_seed0", {"edge_stationary": 1}),
         "fast-h3ws-trained": ("fast", (1, 1, 3), "weights_trained_rope", {"edge_stationary": 1}),
         "fast-h3": ("fast", (1, 1, 3), "weights_seed0", {"edge_stationary": 0}),
         "fast-b3-q16table": ("fast", (1, 1, 3), "weights_seed0", {"edge_products": 3}),
         "fast-inst2-h3": ("fast", (1, 2, 3), "weights_seed0", {}),
         "fast-agg_q16-0": ("fast", (1, 1, 3), "weights_seed0", {"agg_q16": 0}),
         "fast-agg_q16-0-node_stream": ("fast", (1, 1, 3), "weights_seed0", {"agg_q16": 0, "node_stationary": 0}),
         "fast-node_stream": ("fast", (1, 1, 3), "weights_seed0", {"node_stationary": 0}),
         "fast-fused": ("fast", (1, 1, 3), "weights_seed0", {"fuse_aggregate": 2}),
         "fast-dedup0": ("fast", (1, 1, 3), "weights_seed0", {"node_dedup": 0}),
         "fast-dedup2": ("fast", (1, 1, 3), "weights_seed0", {"node_dedup": 2}),
         "fast-pstep4": ("fast", (1, 1, 4), "weights_seed0", {})}      # (the Hr / Hs buffers end on the other swap parity)


@functools.lru_cache(maxsize=None)
def model_for(wname, phys_dim, pstep, prec):
    return make_model(weights_np(wname, phys_dim), phys_dim, pstep, prec)


class Options:
    """Options set on a shared model for the length of a test, then put back (and "max_blocks" with them)."""

    def __init__(self, m, options):
        self.m, self.options = m, dict(options)

    def __enter__(self):
        self.was = {name: self.m.get_option(name) for name in list(self.options) + ["max_blocks"]}
        for name, value in self.options.items():
            self.m.set_option(name, value)
        return self.was["max_blocks"]

    def __exit__(self, *exc):
        for name, value in self.was.items():
            self.m.set_option(name, value)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
def test_forward_at_every_trip_count(path):
    """model(...) of one kernel path over the whole case table.  Per case: one run at the default grid; "max_blocks" set to the case's value,
    the workspaces filled with random bytes, a second run; the workspaces filled again, a third.  (a) pred_pos and pred_motion of the second run
    equal the default grid's bit for bit; (b) its motion is within TOL_BY_PREC[precision] of the float64 step; (c) the status is 0; (d) the third
    run equals the second.  Every case is run before the failures are reported together."""
    prec, cfg, wname, options = PATHS[path]
    phys_dim, n_inst, pstep = cfg
    m = model_for(wname, phys_dim, pstep, prec)
    failures, worst, base = [], 0.0, {}
    with Options(m, options) as default_blocks:
        for name, c in trip_cases().items():
            g = trip_inputs(*c.key)
            phys, p_inst = trip_config_inputs(c.key, phys_dim, n_inst)
            csr = csr_from_lists(g["n_rel"], g["recv"], g["send"], g["attrs"].shape[1])
            if c.key not in base:
                m.set_option("max_blocks", default_blocks)
                base[c.key] = engine_forward(m, g, csr, phys, p_inst)
                if m.take_status() != 0:
                    failures.append((name, "status at the default grid"))
            m.set_option("max_blocks", default_blocks if c.max_blocks is None else c.max_blocks)
            scramble_workspaces()
            got = engine_forward(m, g, csr, phys, p_inst)
            status = m.take_status()
            scramble_workspaces()
            again = engine_forward(m, g, csr, phys, p_inst)
            status_again = m.take_status()
            err = float(np.abs(got[1].cpu().numpy() - trip_ref(c.key, wname, cfg)[1]).max())
            worst = max(worst, err)
            ok = {"a": same(got, base[c.key]), "b": err <= TOL_BY_PREC[prec] and bool(torch.isfinite(got[1]).all()), "c": status == 0 and status_again == 0,
                  "d": same(again, got)}
            print(f"{path:28s} {name:32s} max_blocks {str(c.max_blocks):>7s} motion max-abs {err:.3e} (TOL_BY_PREC {TOL_BY_PREC[prec]:.0e}) "
                  + " ".join(f"({k}) {'holds' if v else 'FAILS'}" for k, v in ok.items()))
            if not all(ok.values()):
                failures.append((name, c.max_blocks, f"{err:.3e}", float((got[1] - base[c.key][1]).abs().max()), [k for k, v in ok.items() if not v]))
    print(f"{path} ({cfg_id(cfg)}, {wname}): worst motion max-abs over {len(trip_cases())} cases {worst:.3e}, TOL_BY_PREC {TOL_BY_PREC[prec]:.0e}")
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------ 3. the drivers at a small grid (GPU)
@functools.lru_cache(maxsize=None)
def rollout_case():
    return Case("rope", 60, 33, seed=17)      # 33 samples of 61 rows: four parts of 9, 9, 9 and 6 samples exist (B / parts >= 8)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("streams", [1, 2, 4])
def test_rollout_parts_at_a_single_workgroup_and_at_unequal_trips(weights, streams, prec):
    """ag_rollout, three steps, "rollout_streams" 1 / 2 / 4: at "max_blocks" 2 every part runs its weight-stationary kernels on one workgroup
    (part_blocks = 1), at 64 every part's node update has workgroups with n_i and n_i - 1 blocks (the table test holds both).  out_seq and
    state_final equal the default grid's bit for bit on scrambled workspaces; status 0."""
    m = case_model(weights, "rope", prec, rollout_streams=streams)
    case = rollout_case()
    prm = _lib.RolloutParams(case.B, case.n_p + case.n_t, case.n_p, 1, case.topk, 0, case.n_t, 3, _lib.AG_HEIGHT_MIN, 0.0)
    assert _lib.lib().ag_rollout_streams_for(m.handle(torch.device(DEV)), ctypes.byref(prm)) == streams
    rep = torch.tensor([b % 3 + 1 for b in range(case.B)], dtype=torch.int32, device=DEV)
    want = case.plain(m, rep, 3)
    assert bool(torch.isfinite(want[1]).all()) and m.take_status() == 0
    for mb in (2, 64, 1):
        m.set_option("max_blocks", mb)
        scramble_workspaces()
        got = case.plain(m, rep, 3)
        assert same(got, want), (mb, float((got[0] - want[0]).abs().max()))
        assert m.take_status() == 0, mb


@pytest.mark.gpu
@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_shared_state_rollout_with_idle_workgroups_and_with_one(weights, prec):
    """ "shared_state" 1: the row and edge counts are device words and the grids upper bounds, so workgroups past the lists have n_i = 0.
    dynamics() of a 100-particle rope under 12 pushes (13 x 101 rows bound the grid: 42 blocks).  "max_blocks" 84: one workgroup per block of the
    bound, every workgroup past the compact row set idle; 8: four workgroups; 2 and 1: a single workgroup walks everything.  state_seqs equal
    the shared-state rollout's at the default grid and the plain rollout's, bit for bit, on scrambled workspaces; status 0."""
    from adaptigraph_amd import synth
    m = case_model(weights, "rope", prec)
    state, act = synth.make_mpc_inputs("rope", 100, 12, n_look=1, seed=13, len_lo=3, len_hi=3.9, spacing=0.1)

    def run():
        return dynamics(t(state), t(act), m, DEV, _ppm("rope"))["state_seqs"].clone()

    plain = run()
    m.set_option("shared_state", 1)
    shared = run()
    assert bool(torch.isfinite(plain).all()) and torch.equal(shared, plain)
    moved = [not torch.equal(plain[b], plain[0]) for b in range(12)]      # (four pushes reach the rope, eight leave it to the base trajectory)
    assert any(moved) and not all(moved[1:])
    for mb in (2 * ceil_div(13 * 101, WS_BLOCK), 8, 2, 1):
        m.set_option("max_blocks", mb)
        run()                            # sizes the workspace
        scramble_workspaces()
        got = run()
        assert torch.equal(got, plain), (mb, float((got - plain).abs().max()))
        m.set_option("shared_state", 0)
        scramble_workspaces()
        assert torch.equal(run(), plain), ("plain", mb)
        m.set_option("shared_state", 1)
        assert m.take_status() == 0, mb


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [0, 1])
@pytest.mark.parametrize("mb", [2, 16])
def test_ragged_rollout_at_small_grids(weights, mb, shared):
    """ag_rollout_ragged through check_against_plain (rope-60 + 1 tool, B = 9, the repeats of tests/test_ragged_rollout.py) at "max_blocks" 2 — one
    workgroup — and 16 — eight workgroups over 18 blocks of the full batch, 3 and 2 each, fewer blocks as samples retire; and the plain call at
    that grid against the default grid's."""
    m = case_model(weights, "rope", "fast", shared_state=shared)
    case = Case("rope", 60, 9, seed=11)
    rep_list = [3, 0, 5, 1, 3, 5, 0, 1, 3]
    rep = torch.tensor(rep_list, dtype=torch.int32, device=DEV)
    want = case.plain(m, rep, 5)
    m.set_option("max_blocks", mb)
    check_against_plain(m, case, rep_list)
    scramble_workspaces()
    assert same(case.plain(m, rep, 5), want) and m.take_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("prec", list(PRECISIONS))
@pytest.mark.parametrize("self_edges", [0, 1])
@pytest.mark.parametrize("name", ["rope50", "rope300"])
def test_scripted_rollout_equals_the_step_loop_at_small_grids(name, self_edges, prec):
    """ag_rollout_scripted against step_loop (build_edges + forward per step), with and without self-edge elision, at the default grid, at
    "max_blocks" 2 (one workgroup) and at 20 (rope300: ten workgroups over 19 node blocks, 2 and 1 each): every step's prediction and the final
    state bit for bit, between the two and between the grids."""
    c = scripted_inputs(name)
    m = model_for("weights_seed0", 1, 3, prec)
    with Options(m, {"self_edges": self_edges}) as default_blocks:
        pred_ref, state_ref, _ = step_loop(m, c)
        for mb in (default_blocks, 2, 20):
            m.set_option("max_blocks", mb)
            scramble_workspaces()
            out = scripted(m, c)
            assert torch.equal(out["pred_seq"], pred_ref), (mb, float((out["pred_seq"] - pred_ref).abs().max()))
            assert torch.equal(out["state_final"], state_ref), mb
            scramble_workspaces()
            loop = step_loop(m, c)
            assert torch.equal(loop[0], pred_ref) and torch.equal(loop[1], state_ref), mb
            assert bool(torch.isfinite(out["pred_seq"]).all()) and m.take_status() == 0


@pytest.mark.gpu
def test_rollout_at_a_small_grid_is_hip_graph_capturable(weights):
    """One three-step rollout at "max_blocks" 16 (unequal trips) captured on the model's default stream count and replayed twice, after the
    capture pattern of test_rollout_is_hip_graph_capturable: the eager result of the default grid."""
    from adaptigraph_amd.forward_dynamics import rollout
    m = case_model(weights, "rope", "fast")
    case = Case("rope", 60, 9, seed=11)
    rep = torch.tensor([3, 1, 2, 3, 3, 2, 1, 3, 2], dtype=torch.int32, device=DEV)
    ref = case.plain(m, rep, 3)[0]
    m.set_option("max_blocks", 16)
    out = torch.zeros((case.B, case.n_p, 3), device=DEV)

    def run():
        return rollout(m, *case.per_sample, case.thr, rep, 3, case.topk, case.connect, case.n_t, case.height, None, 0.0, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(out, ref)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
    assert m.take_status() == 0
