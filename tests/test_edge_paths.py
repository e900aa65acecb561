"""The edge builder (csrc/ag_edges_select.hip, ag_edges.hip) on the selection paths that the synth clouds of tests/test_gpu_parity.py never reach, against the oracle
(oracle/ag_oracle.c, pinned to the reference by tests/test_oracle_golden.py), exactly: the same edge counts and the same (receiver, sender) lists.

Which kernel serves a call is NOT observed: it is read from `ag_launch_build_edges` and the kernels it launches, and the CPU tests of part 1 tie
every input of part 2 to the branch it is meant for.  They restate these constants of the builder's sources; when one of them changes, the reach tests
are what has to follow:
    256                  N >= 256 bins the sample into cells (bin_kernel), below that the brute-force select_kernel scans it
    {5, 10, 20}          the top-k values with a lane-per-receiver kernel; every other top-k at N >= 256 takes select_cells_kernel
    jb <= 16             jb = ceil(log2 N) bits of sender index in a packed key: N <= 65 536 select_lanes_packed_kernel, above it select_lanes_kernel
    kCand 384            candidate list of a wave (select_cells_kernel, select_kernel): pruned in the loop once it holds more than 320
    kKeepFast 8          finalize_connect_kernel merges kept lists of top-k <= 8 from LDS, longer ones from global memory
    kToolListMax 8192    top-k + max_tools above it: finalize_connect_sweep_kernel
    kSelfStageMax        256 x 40 ints: rows of more than 40 slots (top-k + max_tools) take scan_partial_kernel's global-memory self-loop search
    kCellMax 8192        cells of bin_kernel's histogram: the cell size doubles while the grid has more cells ...
    8000                 ... or an axis spans 8000 cells or more; the first cell size is sqrt(thr) * 1.002

Part 1 (no GPU): reach, the decomposition behind the large-N reference, and the oracle against a plain numpy restatement at top-k values it has
hardly been used with.  Part 2 (gpu): the cases."""
import functools
import time

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib, configs, synth
from adaptigraph_amd import graph as aggraph
from adaptigraph_amd.forward_dynamics import rollout
from adaptigraph_amd.model import DynamicsPredictor
from oracle import ag_oracle as ago

gpu = pytest.mark.gpu
DEV = "cuda:0"
GENERIC_TOPK = (1, 3, 7, 32, 64)
SHIPPED_TOPK = (5, 10, 20)


def t(x, dtype=None):
    r = torch.from_numpy(np.array(x)).to(DEV)      # (a copy: the shared clouds are read-only arrays)
    return r if dtype is None else r.to(dtype)


def frozen(**kw):
    """A cloud: pos (B,N,3) float32, mask / tool (B,N) bool, radius (a float, or float32 per sample), n_tools.  Shared between tests: read-only."""
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return kw


def assemble(obj, tools=None, radius=0.5, noise=(1, 1, 1)):
    """Batch 2 from one sample: objects first, tools behind them; sample 1 is sample 0 with its objects moved by N(0, 0.003^2), as synth does."""
    obj = np.asarray(obj, np.float32)
    tools = np.zeros((0, 3), np.float32) if tools is None else np.asarray(tools, np.float32)
    n, nt = len(obj), len(tools)
    pos = np.zeros((2, n + nt, 3), np.float32)
    pos[:, :n] = obj
    pos[:, n:] = tools
    pos[1, :n] += (np.random.default_rng(99).normal(0, 0.003, obj.shape) * noise).astype(np.float32)
    mask = np.ones((2, n + nt), bool)
    tool = np.zeros((2, n + nt), bool)
    tool[:, n:] = True
    return frozen(pos=pos, mask=mask, tool=tool, radius=radius, n_tools=nt)


def from_synth(material, n_obj, batch, seed, **kw):
    g = synth.make_graph_inputs(material, n_obj, batch, seed=seed, **kw)
    return dict(pos=g["state"][:, -1].copy(), mask=g["mask"].copy(), tool=g["tool_mask"].copy(), radius=synth.MATERIALS[material]["radius"],
                n_tools=g["n_tools"])


def ring_points(n_obj, seed):
    """The cloud of test_edges_topk20_packed_key_boundary_vs_oracle: rings of ~45 senders at the same distance up to a few ulps around every
    centre, 20 exact duplicates and a dense remainder."""
    rng = np.random.default_rng(seed)
    n_c = max(n_obj // 50, 1)
    centres = rng.uniform(0, 1.0 * np.sqrt(n_c), (n_c, 2))
    pts = []
    for c in centres:
        m = 45
        ang = rng.uniform(0, 2 * np.pi, m)
        rad = 0.3 * (1 + rng.integers(-3, 4, m) * 6e-8)
        pts.append(np.stack([c[0] + rad * np.cos(ang), np.zeros(m), c[1] + rad * np.sin(ang)], 1))
        pts.append(np.array([[c[0], 0.0, c[1]]]))
    pts = np.concatenate(pts)[:n_obj]
    if len(pts) < n_obj:
        pts = np.concatenate([pts, rng.uniform(0, 0.5, (n_obj - len(pts), 3)) * [1, 0.05, 1]])
    pts[n_obj // 3: n_obj // 3 + 20] = pts[0]
    return pts.astype(np.float32)


def punch_holes(c, n_obj, seed):
    """20 % of the object slots of samples 0 and 1 invalid, with garbage positions (1e3 or 0); sample 2: every slot invalid; sample 3: one valid object."""
    rng = np.random.default_rng(seed)
    pos, mask = c["pos"], c["mask"]
    for b in range(4):
        dead = rng.uniform(size=n_obj) < 0.2
        if b == 2:
            mask[b] = False
            dead[:] = True
        if b == 3:
            dead[:] = True
            dead[n_obj // 2 + 7] = False
        mask[b, :n_obj] = ~dead
        pos[b, :n_obj][dead] = np.where(rng.uniform(size=(int(dead.sum()), 1)) < 0.5, np.float32(1e3), np.float32(0.0))
    return frozen(**c)


@functools.lru_cache(maxsize=None)
def cloud(name):
    rng = np.random.default_rng(7)
    if name == "lattice":       # 16^3 points, spacing 0.25, indices permuted: every distance is exact in fp32 and most rows cut inside a group of equal ones
        g = np.arange(16) * 0.25
        pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        return assemble(pts[rng.permutation(len(pts))])
    if name == "blob":          # everything within reach of everything: more candidates per row than a wave's list holds
        return assemble(rng.uniform(0, 0.4, (700, 3)), [[0.2, 0.2, 0.2]])
    if name == "plane":         # the blob with y = 0 in both samples: zero extent in one axis
        pts = rng.uniform(0, 0.4, (700, 3))
        pts[:, 1] = 0
        return assemble(pts, [[0.2, 0.0, 0.2]], noise=(1, 0, 1))
    if name == "point":         # 300 coincident points: zero extent in every axis (sample 1: an extent of ~0.02)
        return assemble(np.tile(np.float32([0.3, -0.7, 1.1]), (300, 1)))
    if name == "ring":
        c = from_synth("granular", 2000, 2, 2)
        c["pos"][0, :2000] = ring_points(2000, 2)
        return frozen(**dict(c, radius=0.4))
    if name == "line":          # 1500 groups of three along 5000 units of x: more than 8000 cells of the first size in one axis
        x = np.repeat(np.linspace(0, 5000, 1500), 3)
        return assemble(np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1) + rng.uniform(-0.15, 0.15, (4500, 3)))
    if name == "cube":          # 300 clusters of ten in a 30^3 box: 60^3 cells of the first size
        centres = np.repeat(rng.uniform(0, 30, (300, 3)), 10, 0)
        return assemble(centres + rng.uniform(-0.2, 0.2, centres.shape))
    if name == "offset":        # far from the origin: coordinates quantised to ~1e-4
        return assemble(rng.uniform(0, 3, (1000, 3)) + [1000.0, -2000.0, 500.0])
    if name == "holes_rope":
        return punch_holes(from_synth("rope", 1000, 4, 41, spacing=0.1), 1000, 42)
    if name == "holes_granular":
        return punch_holes(from_synth("granular", 2000, 4, 43), 2000, 44)
    if name == "radii":         # one radius per sample: four different grids in one call, the last one a handful of cells
        return frozen(**dict(from_synth("rope", 1000, 4, 45, spacing=0.1), radius=np.float32([0.12, 0.5, 1.5, 6.0])))
    if name == "cloth1024":
        return frozen(**from_synth("cloth", 1024, 2, 46))
    if name == "granular600":
        return frozen(**from_synth("granular", 600, 2, 47))
    raise KeyError(name)


def many_tools(n_tools, scattered, seed):
    """Batch 1: a 300-particle rope and `n_tools` tool points next to particles of it, behind the objects or scattered through the index range."""
    rng = np.random.default_rng(seed)
    obj, _ = synth.rope_cloud(300, 0.1, rng)
    tools = obj[rng.choice(300, n_tools, replace=False)] + rng.uniform(-0.2, 0.2, (n_tools, 3)).astype(np.float32)
    N = 300 + n_tools
    tool = np.zeros(N, bool)
    tool[rng.choice(N, n_tools, replace=False) if scattered else np.arange(300, N)] = True
    pos = np.zeros((N, 3), np.float32)
    pos[~tool], pos[tool] = obj, tools
    return frozen(pos=pos[None], mask=np.ones((1, N), bool), tool=tool[None], radius=0.5, n_tools=n_tools)


SWEEP_N, SWEEP_TOOLS, SWEEP_TOPK = 9000, 8300, 5


@functools.lru_cache(maxsize=None)
def sweep_cloud(tools_near):
    """Batch 1, 9000 slots: 700 objects in a 6 x 6 sheet and 8300 tools scattered through the index range, over the sheet or 100 units above it."""
    rng = np.random.default_rng(11)
    tool = np.zeros(SWEEP_N, bool)
    tool[rng.choice(SWEEP_N, SWEEP_TOOLS, replace=False)] = True
    pos = np.zeros((SWEEP_N, 3), np.float32)
    n_obj = SWEEP_N - SWEEP_TOOLS
    pos[~tool] = np.stack([rng.uniform(0, 6, n_obj), rng.normal(0, 0.01, n_obj), rng.uniform(0, 6, n_obj)], 1)
    pos[tool] = np.stack([rng.uniform(0, 6, SWEEP_TOOLS), rng.uniform(0.05, 0.3, SWEEP_TOOLS) + (0.0 if tools_near else 100.0),
                          rng.uniform(0, 6, SWEEP_TOOLS)], 1)
    return frozen(pos=pos[None], mask=np.ones((1, SWEEP_N), bool), tool=tool[None], radius=0.75, n_tools=SWEEP_TOOLS)


LARGE = {65536: (32, 2048), 66000: (33, 2000)}      # N: (clusters, points per cluster)
LARGE_RADIUS = 0.4


@functools.lru_cache(maxsize=None)
def clusters(C, n, seed=13):
    """(C, n, 3) float32: C granular-like slabs (n points, 40 to 90 per radius-0.4 disc) whose origins sit on a 4 x 3 x k arrangement with gaps of
    more than 4 radii, coordinates already shifted."""
    rng = np.random.default_rng(seed)
    side_max = float(np.sqrt(n / 80.0))
    pitch = np.array([side_max + 2.0, 2.0, side_max + 2.0])
    out = np.zeros((C, n, 3), np.float32)
    for c in range(C):
        pts, _ = synth.granular_cloud(n, rng, density=(80.0, 120.0, 180.0)[c % 3])
        out[c] = (pts + np.array([c % 4, (c // 4) % 3, c // 12]) * pitch).astype(np.float32)
    out.setflags(write=False)
    return out


def interleave(cl):
    """Global index = local * C + c: the clusters alternate through the index range, the order inside a cluster is kept."""
    C, n, _ = cl.shape
    return np.ascontiguousarray(cl.transpose(1, 0, 2).reshape(1, C * n, 3))


def per_cluster_reference(cl, radius, topk):
    """The oracle on the clusters as a batch of C samples, mapped to the interleaved indices, in ascending (receiver, sender) order."""
    C, n, _ = cl.shape
    ones, zeros = np.ones((C, n), bool), np.zeros((C, n), bool)
    n_rel, recv, send = ago.build_edges(cl, radius, ones, zeros, topk, False, "batch")
    r = np.concatenate([recv[c, :n_rel[c]] * C + c for c in range(C)])
    s = np.concatenate([send[c, :n_rel[c]] * C + c for c in range(C)])
    order = np.argsort(r, kind="stable")      # a receiver's edges all come from its own cluster, senders ascending
    return r[order].astype(np.int32), s[order].astype(np.int32)


SELF_OBJ, SELF_TOOLS, SELF_TOPK = 300, 40, 5


@functools.lru_cache(maxsize=None)
def self_loop_inputs():
    """A cloth-like sample (15 x 20 sheet, spacing 0.25) with 40 tool points over it, batch 2, in synth.make_graph_inputs' layout."""
    rng = np.random.default_rng(17)
    xx, zz = np.meshgrid(np.arange(15) * 0.25, np.arange(20) * 0.25, indexing="ij")
    obj = np.stack([xx.ravel(), np.zeros(SELF_OBJ), zz.ravel()], 1) + rng.normal(0, 0.01, (SELF_OBJ, 3))
    tools = np.stack([rng.uniform(0, 3.5, SELF_TOOLS), np.full(SELF_TOOLS, 0.05), rng.uniform(0, 4.75, SELF_TOOLS)], 1)
    B, H, N = 2, 4, SELF_OBJ + SELF_TOOLS
    state = np.zeros((B, H, N, 3), np.float32)
    for b in range(B):
        cur = np.concatenate([obj + rng.normal(0, 0.003, obj.shape) * (b > 0), tools])
        for h in range(H):
            state[b, h] = cur + rng.normal(0, 0.01, (N, 3))
    attrs = np.zeros((B, N, 2), np.float32)
    attrs[:, :SELF_OBJ, 0] = 1
    attrs[:, SELF_OBJ:, 1] = 1
    action = np.zeros((B, N, 3), np.float32)
    action[:, SELF_OBJ:] = np.float32([0.1, 0.0, 0.0])
    mask = np.ones((B, N), bool)
    tool = np.zeros((B, N), bool)
    tool[:, SELF_OBJ:] = True
    return frozen(state=state, attrs=attrs, action=action, p_instance=np.ones((B, SELF_OBJ, 1), np.float32), phys=np.full((B, 1), 0.5, np.float32),
                  mask=mask, tool=tool)


# ------------------------------------------------------------------------------------------------------------ references
def oracle_radius(radius):
    return radius if np.isscalar(radius) else np.asarray(radius, np.float32).astype(np.float64)      # the fp32 values, as the builder gets them


@functools.lru_cache(maxsize=None)
def oracle_edges(name, topk, connect=False, variant="batch"):
    c = cloud(name)
    return ago.build_edges(c["pos"], oracle_radius(c["radius"]), c["mask"], c["tool"], topk, connect, variant)


@functools.lru_cache(maxsize=None)
def numpy_nearest(name, b):
    """Sample b of a cloud, batch variant, restated plainly: fp32 ((dx*dx + dy*dy) + dz*dz), 1e10 for masked and tool-tool pairs, every row sorted
    by a stable sort (ties to the lower index).  -> the 64 nearest senders of every row and whether each is in radius, (d - thr) < 0."""
    c = cloud(name)
    pos, mask, tool = c["pos"][b], c["mask"][b], c["tool"][b]
    thr = np.float32(c["radius"]) * np.float32(c["radius"])
    near, keep = [], []
    for i0 in range(0, len(pos), 512):
        p = pos[i0:i0 + 512]
        dx, dy, dz = (p[:, None, a] - pos[None, :, a] for a in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        d[~(mask[i0:i0 + 512, None] & mask[None, :])] = np.float32(1e10)
        d[tool[i0:i0 + 512, None] & tool[None, :]] = np.float32(1e10)
        near.append(np.argsort(d, axis=1, kind="stable")[:, :64])
        keep.append((np.take_along_axis(d, near[-1], 1) - thr) < 0)
    return np.concatenate(near), np.concatenate(keep)


def numpy_edges(name, b, topk):
    """-> (recv, send) of sample b: the top-k nearest of every row that are in radius, senders ascending."""
    near, keep = numpy_nearest(name, b)
    send = [np.sort(near[i, :topk][keep[i, :topk]]) for i in range(len(near))]
    recv = [np.full(len(s), i) for i, s in enumerate(send)]
    return np.concatenate(recv).astype(np.int32), np.concatenate(send).astype(np.int32)


def grid_rule(pos, mask, radius):
    """bin_kernel's grid of one sample, in float32: -> ((nx, ny, nz), doublings: the list of the rule that caused each one)."""
    f32 = np.float32
    p = np.asarray(pos, f32)[np.asarray(mask, bool)]
    mn, mx = (p.min(0), p.max(0)) if len(p) else (np.zeros(3, f32), np.zeros(3, f32))
    thr = f32(radius) * f32(radius)
    cs = f32(np.sqrt(thr)) * f32(1.002)
    why = []
    while True:
        f = (mx - mn) / cs
        assert f.dtype == np.float32
        if (f < f32(8000)).all():
            n = tuple(int(v) + 1 for v in f)
            if n[0] * n[1] * n[2] <= 8192:
                return n, why
            why.append("8192 cells")
        else:
            why.append("8000 per axis")
        cs = cs * f32(2)


def in_radius_counts(pos, mask, tool, radius):
    thr = np.float32(radius) * np.float32(radius)
    dx, dy, dz = (pos[:, None, a] - pos[None, :, a] for a in range(3))
    d = (dx * dx + dy * dy) + dz * dz
    d[~(mask[:, None] & mask[None, :])] = 1e10
    d[tool[:, None] & tool[None, :]] = 1e10
    return ((d - thr) < 0).sum(1)


# ====================================================================================================== 1. without a GPU
def test_reach_grid_coarsening():
    """`line` coarsens by the 8000-cells-per-axis rule, `cube` by the 8192-cell histogram, `lattice`, `offset` and `blob` keep the first cell size,
    `point` is one cell, `plane` has one layer of cells, and the four radii of `radii` give four different grids, the last of a few cells."""
    def rule(name, b=0):
        c = cloud(name)
        r = c["radius"] if np.isscalar(c["radius"]) else c["radius"][b]
        return grid_rule(c["pos"][b], c["mask"][b], r)

    for b in range(2):
        n, why = rule("line", b)
        assert why and why[0] == "8000 per axis" and n[0] > 4000, (n, why)
        n, why = rule("cube", b)
        assert why and set(why) == {"8192 cells"}, (n, why)
        for name in ("lattice", "offset", "blob", "plane"):
            n, why = rule(name, b)
            assert not why and n[0] * n[1] * n[2] <= 8192, (name, n, why)
    assert rule("line")[0] == (4991, 1, 1) and len(rule("line")[1]) == 1
    assert rule("cube")[0] == (16, 16, 16) and len(rule("cube")[1]) == 2
    assert rule("lattice")[0] == (8, 8, 8) and rule("offset")[0] == (6, 6, 6)
    assert rule("point", 0) == ((1, 1, 1), []) and rule("point", 1) == ((1, 1, 1), [])
    assert np.ptp(cloud("point")["pos"][0], axis=0).max() == 0
    assert rule("plane", 0)[0][1] == 1 and rule("plane", 1)[0][1] == 1
    grids = [rule("radii", b)[0] for b in range(4)]
    assert len(set(grids)) == 4 and grids[3][0] * grids[3][1] * grids[3][2] <= 64, grids
    for name in ("holes_rope", "holes_granular"):      # the garbage positions of invalid slots never enter a grid
        c = cloud(name)
        assert grid_rule(c["pos"][2], c["mask"][2], c["radius"]) == ((1, 1, 1), []) and c["mask"][2].sum() == 0
        assert c["mask"][3][~c["tool"][3]].sum() == 1
        frac = 1 - c["mask"][0][~c["tool"][0]].mean()
        assert 0.15 < frac < 0.25 and np.abs(c["pos"][0][~c["mask"][0]]).max() == 1e3


def test_reach_sizes_and_thresholds():
    for name in ("lattice", "blob", "plane", "point", "ring", "line", "cube", "offset", "holes_rope", "holes_granular", "radii", "cloth1024",
                 "granular600"):
        assert cloud(name)["pos"].shape[1] >= 256 and cloud(name)["pos"].dtype == np.float32, name      # cell path
    assert not set(GENERIC_TOPK) & set(SHIPPED_TOPK) and min(GENERIC_TOPK) >= 1 and max(GENERIC_TOPK) <= 64
    for name in ("blob", "plane"):      # the in-loop prune: a list that would pass 384 - 64
        c = cloud(name)
        for b in range(2):
            cnt = in_radius_counts(c["pos"][b], c["mask"][b], c["tool"][b], c["radius"])
            assert cnt.min() > 320, (name, b, cnt.min())
    for N, (C, n) in LARGE.items():
        assert C * n == N and interleave(clusters(C, n)).shape == (1, N, 3)
        jb = 1
        while (1 << jb) < N:
            jb += 1
        assert jb == (16 if N == 65536 else 17)
        lo, hi = clusters(C, n).min(1), clusters(C, n).max(1)
        gap = np.maximum(lo[:, None] - hi[None, :], lo[None, :] - hi[:, None]).max(-1)      # largest per-axis gap of two bounding boxes
        assert (gap[~np.eye(C, dtype=bool)] > LARGE_RADIUS).all()
        assert (gap[~np.eye(C, dtype=bool)] > 4 * LARGE_RADIUS).all()
    assert SWEEP_TOPK + SWEEP_TOOLS > 8192 and sweep_cloud(True)["tool"].sum() == SWEEP_TOOLS and sweep_cloud(True)["pos"].shape[1] == SWEEP_N
    far = sweep_cloud(False)      # no object within reach of a tool: the batch variant's per-sample flag stays 0
    assert far["pos"][0][far["tool"][0]][:, 1].min() - far["pos"][0][~far["tool"][0]][:, 1].max() > far["radius"]
    assert (SELF_TOPK + SELF_TOOLS) * 256 > 256 * 40 and self_loop_inputs()["tool"][0].sum() == SELF_TOOLS
    assert many_tools(12, False, 51)["n_tools"] > 5 and 5 <= 8 < 10      # tool list longer than the kept list, on both sides of kKeepFast


def test_reach_lattice_cuts_inside_tie_groups():
    """An interior lattice row has 27 in-radius entries: itself, 6 at d = 0.0625, 12 at 0.125, 8 at 0.1875, and none at d == thr (0.25, excluded by
    (d - thr) < 0).  Top-k 3, 5, 10 and 20 cut an interior row inside a group of equal distances.  Top-k 7 = 1 + 6 cuts an INTERIOR row between two
    groups; it cuts inside one on the rows of the six faces (1 + 5 + 8 + 4 entries), which is where its tie-break is decided.  Top-k 1 keeps the
    self entry (d = 0) and has no tie anywhere."""
    c = cloud("lattice")
    pos = c["pos"][0]
    ijk = np.rint(pos / 0.25).astype(int)
    assert np.array_equal(ijk * np.float32(0.25), pos)
    inner = np.flatnonzero(((ijk >= 2) & (ijk <= 13)).all(1))[:40]
    face = np.flatnonzero((((ijk == 0) | (ijk == 15)).sum(1) == 1) & ((ijk != 1) & (ijk != 14)).all(1))[:40]
    thr = np.float32(0.25)

    def sorted_d(rows):
        d = ((pos[rows, None] - pos[None]) ** 2).astype(np.float32)
        d = (d[..., 0] + d[..., 1]) + d[..., 2]
        assert ((d == thr).sum(1) > 0).all()      # neighbours at exactly the radius exist; (d - thr) < 0 leaves them out
        n_in = ((d - thr) < 0).sum(1)
        return np.sort(d, 1), n_in

    d, n_in = sorted_d(inner)
    assert (n_in == 27).all()
    assert (d[:, 1:7] == 0.0625).all() and (d[:, 7:19] == 0.125).all() and (d[:, 19:27] == 0.1875).all() and (d[:, 27] == 0.25).all()
    for k in (3, 5, 10, 20):
        assert (d[:, k - 1] == d[:, k]).all(), k
    assert (d[:, 6] < d[:, 7]).all() and (d[:, 0] < d[:, 1]).all()
    d, n_in = sorted_d(face)
    assert len(face) == 40 and (n_in == 18).all() and (d[:, 6] == d[:, 7]).all()
    # the permutation: index order is not spatial order, so "lower sender index" is not "first in the cell walk"
    assert not np.array_equal(np.lexsort(ijk.T[::-1]), np.arange(len(pos)))


def test_decomposition_of_an_interleaved_cloud_into_its_clusters():
    """The reference of the large-N cases: the oracle on the whole interleaved cloud == the oracle per cluster after index mapping (4 x 500)."""
    cl = clusters(4, 500, seed=14)
    pos = interleave(cl)
    N = pos.shape[1]
    for topk in (5, 7, 20):
        n_rel, recv, send = ago.build_edges(pos, LARGE_RADIUS, np.ones((1, N), bool), np.zeros((1, N), bool), topk, False, "batch")
        r, s = per_cluster_reference(cl, LARGE_RADIUS, topk)
        assert n_rel[0] == len(r) > N and np.array_equal(recv[0, :len(r)], r) and np.array_equal(send[0, :len(s)], s)
        assert (r % 4 == s % 4).all()


@pytest.mark.parametrize("name", ["lattice", "blob"])
def test_oracle_equals_numpy_at_generic_topk(name):
    for topk in GENERIC_TOPK:
        n_rel, recv, send = oracle_edges(name, topk)
        for b in range(2):
            r, s = numpy_edges(name, b, topk)
            assert n_rel[b] == len(r) and np.array_equal(recv[b, :len(r)], r) and np.array_equal(send[b, :len(s)], s), (topk, b)


# ====================================================================================================== 2. on the GPU
def assert_edges_equal(csr, n_rel, recv, send):
    assert csr.n_rel().cpu().tolist() == n_rel.tolist()
    for b, (r, s) in enumerate(csr.to_lists()):
        assert np.array_equal(r, recv[b, :n_rel[b]]) and np.array_equal(s, send[b, :n_rel[b]]), f"sample {b}"


def gpu_edges(c, topk, connect=False, variant="batch"):
    radius = t(c["radius"]) if isinstance(c["radius"], np.ndarray) else c["radius"]
    return aggraph.build_edges(t(c["pos"]), radius, t(c["mask"]), t(c["tool"]), topk, connect, variant, max_tools=c["n_tools"])


def check_cloud(name, topk, connect=False, variant="batch"):
    assert_edges_equal(gpu_edges(cloud(name), topk, connect, variant), *oracle_edges(name, topk, connect, variant))


@gpu
@pytest.mark.parametrize("topk", GENERIC_TOPK)
@pytest.mark.parametrize("name,variant", [("lattice", "batch"), ("lattice", "single"), ("ring", "batch")])
def test_generic_topk_ties_and_ulp_rings(name, variant, topk):
    """select_cells_kernel: exact tie groups cut by the lower sender index (lattice), senders a few ulps apart and exact duplicates (ring)."""
    check_cloud(name, topk, False, variant)


@gpu
@pytest.mark.parametrize("topk", [3, 7, 64])
def test_generic_topk_in_loop_prune(topk):
    """More than 320 in-radius candidates in every row: select_cells_kernel prunes its list inside the candidate loop (the dense=True case of
    test_edges_vs_oracle_exact has the same cloud at top-k 10, which the packed kernel serves without a list)."""
    check_cloud("blob", topk)


@gpu
@pytest.mark.parametrize("variant", ["batch", "single"])
@pytest.mark.parametrize("name,topk", [("cloth1024", 7), ("cloth1024", 32), ("granular600", 7)])
def test_generic_topk_connect_tools_all(name, topk, variant):
    """select_cells_kernel's per-sample flag and kept lists into finalize_connect_kernel: top-k 7 the LDS merge, top-k 32 the generic one."""
    check_cloud(name, topk, True, variant)


GEOMETRIES = ["holes_rope", "holes_granular", "radii", "line", "cube", "offset", "point", "plane"]


@gpu
@pytest.mark.parametrize("name", GEOMETRIES)
def test_generic_topk_geometries(name):
    check_cloud(name, 7)


@gpu
@pytest.mark.parametrize("topk", SHIPPED_TOPK)
@pytest.mark.parametrize("name,variant", [(n, "batch") for n in ["lattice"] + GEOMETRIES]
                         + [("lattice", "single"), ("holes_rope", "single"), ("holes_granular", "single")])
def test_shipped_topk_geometries(name, variant, topk):
    """The packed kernels on coarsened, degenerate, far-away and per-sample grids, on exact ties, and with unbinned receivers in the middle of
    the index range (their degree is zeroed apart from the cell-ordered receivers)."""
    check_cloud(name, topk, False, variant)


@functools.lru_cache(maxsize=None)
def large_reference(N, topk):
    C, n = LARGE[N]
    return per_cluster_reference(clusters(C, n), LARGE_RADIUS, topk)


@gpu
@pytest.mark.parametrize("N,topk", [(65536, 5), (65536, 10), (65536, 20), (66000, 5), (66000, 10), (66000, 20), (66000, 7)])
def test_large_n_packed_at_16_index_bits_and_unpacked_above(N, topk):
    """N = 65 536: packed keys with 16 bits of distance (the exact redo of ambiguous boundaries is frequent); N = 66 000: select_lanes_kernel."""
    C, n = LARGE[N]
    t0 = time.perf_counter()
    r, s = large_reference(N, topk)
    t1 = time.perf_counter()
    pos = interleave(clusters(C, n))
    csr = aggraph.build_edges(t(pos), LARGE_RADIUS, t(np.ones((1, N), bool)), t(np.zeros((1, N), bool)), topk, False, "batch", max_tools=0)
    (gr, gs), = csr.to_lists()
    print(f"large N {N} top-k {topk}: {len(r)} edges, oracle {t1 - t0:.2f} s, upload + build + read back {(time.perf_counter() - t1) * 1e3:.0f} ms")
    assert int(csr.n_rel()[0]) == len(r)
    assert np.array_equal(gr, r) and np.array_equal(gs, s)


@gpu
@pytest.mark.parametrize("variant", ["batch", "single"])
@pytest.mark.parametrize("n_tools,topk,scattered", [(12, 5, False), (60, 10, True)])
def test_many_tools(n_tools, topk, scattered, variant):
    c = many_tools(n_tools, scattered, 51 + n_tools)
    ref = ago.build_edges(c["pos"], c["radius"], c["mask"], c["tool"], topk, True, variant)
    assert ref[0][0] > 300 * n_tools
    assert_edges_equal(gpu_edges(c, topk, True, variant), *ref)


@gpu
@pytest.mark.parametrize("variant,tools_near", [("single", True), ("batch", False), ("batch", True)])
def test_more_tools_than_the_tool_list_holds(variant, tools_near):
    """top-k + max_tools = 8305 > 8192: finalize_connect_sweep_kernel.  single: every object receives every tool; batch with the tools out of reach:
    the sample's flag stays 0 and no tool edge exists; batch with the tools in reach: every slot receives every tool, tools included."""
    c = sweep_cloud(tools_near)
    n_obj = SWEEP_N - SWEEP_TOOLS
    full = variant == "batch" and tools_near
    e_cap = SWEEP_N * (SWEEP_TOPK + SWEEP_TOOLS) if full else SWEEP_N * SWEEP_TOPK + n_obj * SWEEP_TOOLS
    t0 = time.perf_counter()
    n_rel, recv, send = ago.build_edges(c["pos"], c["radius"], c["mask"], c["tool"], SWEEP_TOPK, True, variant, e_cap=e_cap)
    t1 = time.perf_counter()
    csr = gpu_edges(c, SWEEP_TOPK, True, variant)
    got = csr.to_lists()
    print(f"sweep {variant} tools {'near' if tools_near else 'far'}: {n_rel[0]} edges, oracle {t1 - t0:.2f} s, "
          f"upload + build + read back {(time.perf_counter() - t1) * 1e3:.0f} ms")
    tool_edges = int(c["tool"][0][send[0, :n_rel[0]]].sum())
    assert tool_edges == (SWEEP_N * SWEEP_TOOLS if full else n_obj * SWEEP_TOOLS if variant == "single" else 0)
    assert csr.n_rel().cpu().tolist() == n_rel.tolist()
    assert np.array_equal(got[0][0], recv[0, :n_rel[0]]) and np.array_equal(got[0][1], send[0, :n_rel[0]])


@gpu
@pytest.mark.parametrize("mode", ["fast", "f32"])
def test_self_loop_elision_with_rows_longer_than_the_staging_buffer(weights, mode):
    """Rows of top-k 5 + 40 tools = 45 slots: scan_partial_kernel finds the self-loops in global memory.  A two-step rollout gives the same bits with
    the self-loops elided (self_edges 1) and kept (0); the edge lists of the start state are the oracle's."""
    g = self_loop_inputs()
    m = DynamicsPredictor(configs.model_config(), configs.material_config("cloth"), configs.dataset_config("cloth"), DEV)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in weights.items()})
    m = m.to(DEV).eval()
    m.set_option("precision", {"fast": 2, "f32": 0}[mode])
    thr = aggraph.threshold_sq(0.75, 2, torch.device(DEV), _lib.AG_VARIANT_BATCH)
    rep = torch.full((2,), 2, dtype=torch.int32, device=DEV)

    def run():
        out, state = rollout(m, t(g["state"]), t(g["action"]), t(g["attrs"]), t(g["p_instance"]), t(g["phys"]), t(g["mask"]), t(g["tool"]), thr, rep,
                             2, SELF_TOPK, True, SELF_TOOLS, return_state=True)
        return out.clone(), state.clone()

    m.set_option("self_edges", 0)
    ref_out, ref_state = run()
    m.set_option("self_edges", 1)
    out, state = run()
    assert torch.isfinite(ref_out).all() and torch.isfinite(ref_state).all() and ref_out.abs().max() > 0
    assert not torch.equal(ref_state[:, -1, :SELF_OBJ], t(g["state"])[:, -1, :SELF_OBJ])      # the steps ran
    assert torch.equal(out, ref_out) and torch.equal(state, ref_state)
    assert m.take_status() == 0
    start = dict(pos=g["state"][:, -1], mask=g["mask"], tool=g["tool"], radius=0.75, n_tools=SELF_TOOLS)
    ref = ago.build_edges(start["pos"], 0.75, g["mask"], g["tool"], SELF_TOPK, True, "batch")
    assert ref[0].min() > (SELF_OBJ + SELF_TOOLS) * SELF_TOOLS      # every slot receives every tool: rows of 40 to 45 slots
    assert_edges_equal(gpu_edges(start, SELF_TOPK, True, "batch"), *ref)
