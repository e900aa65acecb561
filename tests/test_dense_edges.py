"""Dense one-hot Rr / Rs <-> CSR on the device (`ag_edges_from_dense`, `ag_edges_to_dense`, csrc/ag_dense.hip): the kernels against the host
function `graph.csr_from_dense` and against the torch construction `CSREdges.to_dense` used before them, bit for bit; the forward on dense
inputs against the forward on the CSR they came from; HIP-graph capture of both compatibility paths; and no host synchronisation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib, configs, synth
from adaptigraph_amd import graph as aggraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NEW = ("ag_dense_edges_workspace_bytes", "ag_edges_from_dense", "ag_edges_to_dense")


# ------------------------------------------------------------------------------------------ C ABI, no GPU
def test_dense_symbols_are_exported_and_declared():
    L = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adaptigraph_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.EXPORTS, n
        assert re.search(r"\b%s\s*\(" % n, header), f"{n} is not declared in include/adaptigraph_hip.h"


def test_dense_workspace_bytes_positive_and_monotone():
    ws = _lib.lib().ag_dense_edges_workspace_bytes
    assert ws(1, 1, 1) > 0
    assert ws(128, 300, 108) >= 2 * 128 * 300 * 4 + 128 * 108 * 4          # two keys per row pair, one counter per receiver
    for B, E, N in ((1, 1, 1), (3, 65, 108), (128, 300, 108), (500, 3000, 201)):
        base = ws(B, E, N)
        assert ws(B + 1, E, N) >= base and ws(B, E + 1, N) >= base and ws(B, E, N + 1) >= base
        assert ws(2 * B + 64, E, N) > base and ws(B, 2 * E + 64, N) > base and ws(B, E, 2 * N + 256) > base


def test_dense_argument_errors_are_codes():
    L = _lib.lib()
    f = (ctypes.c_float * 64)()
    i = (ctypes.c_int32 * 64)()
    need = L.ag_dense_edges_workspace_bytes(1, 2, 4)
    assert L.ag_edges_from_dense(None, f, 1, 2, 4, i, i, i, i, need, None) == -1 and b"null" in L.ag_last_error()
    assert L.ag_edges_from_dense(f, f, 1, 2, 4, i, i, i, None, need, None) == -1
    assert L.ag_edges_from_dense(f, f, 0, 2, 4, i, i, i, i, need, None) == -1 and b"B=0" in L.ag_last_error()
    assert L.ag_edges_from_dense(f, f, 1, 0, 4, i, i, i, i, need, None) == -1
    assert L.ag_edges_from_dense(f, f, 1, 2, 0, i, i, i, i, need, None) == -1
    assert L.ag_edges_from_dense(f, f, 70000, 2, 70000, i, i, i, i, need, None) == -1          # B*N >= 2^31
    assert L.ag_edges_from_dense(f, f, 1, 2, 4, i, i, i, i, need // 2, None) == -3 and b"workspace" in L.ag_last_error()
    assert L.ag_edges_from_dense(f, f, 1, 2, 4, i, i, i, i, 0, None) == -3
    assert L.ag_edges_to_dense(None, i, i, 1, 4, 2, f, f, i, None) == -1 and b"null" in L.ag_last_error()
    assert L.ag_edges_to_dense(i, i, i, 1, 4, 2, f, f, None, None) == -1
    assert L.ag_edges_to_dense(i, i, i, 0, 4, 2, f, f, i, None) == -1
    assert L.ag_edges_to_dense(i, i, i, 1, 4, 0, f, f, i, None) == -1 and b"E_out=0" in L.ag_last_error()


def test_to_dense_of_a_host_adjacency_still_works():
    """csr_from_dense takes CPU tensors, and its result converts back on the host as it did before the kernel existed."""
    B, E, N = 2, 7, 5
    g = torch.Generator().manual_seed(3)
    valid = torch.tensor([[1, 0, 1, 1, 0, 1, 0], [0, 1, 1, 0, 0, 0, 0]], dtype=torch.bool)
    Rr = torch.zeros(B, E, N).scatter_(2, torch.randint(0, N, (B, E, 1), generator=g), valid[..., None].float())
    Rs = torch.zeros(B, E, N).scatter_(2, torch.randint(0, N, (B, E, 1), generator=g), valid[..., None].float())
    csr = aggraph.as_csr(Rr, Rs)
    assert not csr.row_ptr.is_cuda
    Dr, Ds = csr.to_dense()
    assert Dr.shape == (B, 4, N) and int(csr.overflow) == 0
    for b in range(B):          # the valid rows, stably sorted by receiver, zero rows behind
        rows = [e for e in range(E) if valid[b, e]]
        rows.sort(key=lambda e: int(Rr[b, e].argmax()))
        assert torch.equal(Dr[b, :len(rows)], Rr[b, rows]) and torch.equal(Ds[b, :len(rows)], Rs[b, rows])
        assert float(Dr[b, len(rows):].abs().sum()) == 0 and float(Ds[b, len(rows):].abs().sum()) == 0
    Pr, _ = csr.to_dense(torch.float64, e_max=6)
    assert Pr.dtype == torch.float64 and torch.equal(Pr[:, :4], Dr.double()) and float(Pr[:, 4:].abs().sum()) == 0 and int(csr.overflow) == 0
    Cr, Cs = csr.to_dense(e_max=3)
    assert torch.equal(Cr, Dr[:, :3]) and torch.equal(Cs, Ds[:, :3]) and int(csr.overflow) == 1


# ------------------------------------------------------------------------------------------ dense -> CSR
# The issue's sizes, plus the implementation's own boundaries: a wave reads 64 16-byte quads = 256 slots per trip (rows around 253..257 slots
# start a second trip, depending on where the row starts in its first quad), four waves per workgroup (E, B E not multiples of 4), 256 receivers
# per scan workgroup (B N around 256 and beyond), 64 keys per placement chunk (E 64 / 65), and cursors in LDS up to N = 8192.
SIZES = [(B, E, N) for B in (1, 3) for E in (1, 7, 64, 65, 500) for N in (1, 5, 63, 64, 65, 108, 257, 1001)]
SIZES += [(2, 9, N) for N in (252, 253, 255, 256)] + [(2, 70, 8192), (2, 70, 8193), (1, 3, 8191)]
KINDS = ("permuted", "padded", "empty_sample", "all_zero", "half_rows", "multi_hot", "views", "misaligned")


def one_hot_rows(idx, N, valid):
    """(B, E) int64 slots, (B, E) bool -> (B, E, N) fp32 on the host."""
    B, E = idx.shape
    out = torch.zeros(B, E, N)
    out.scatter_(2, idx[..., None], valid[..., None].float())
    return out


def dense_case(kind, B, E, N, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, N, (B, E), generator=g)
    s = torch.randint(0, N, (B, E), generator=g)
    vr = torch.ones(B, E, dtype=torch.bool)
    vs = vr.clone()
    if kind == "padded":            # zero rows interleaved and trailing
        vr = torch.rand(B, E, generator=g) < 0.6
        vr[:, E - E // 4:] = False
        vs = vr.clone()
    elif kind == "empty_sample":
        vr[B // 2] = False
        vs = vr.clone()
    elif kind == "all_zero":
        vr[:] = False
        vs = vr.clone()
    elif kind == "half_rows":       # Rr row set but Rs row zero, and the reverse: both dropped
        u = torch.rand(B, E, generator=g)
        vr, vs = u < 0.7, u > 0.3
    Rr, Rs = one_hot_rows(r, N, vr), one_hot_rows(s, N, vs)
    if kind == "multi_hot":
        for t_ in (Rr, Rs):
            for _ in range(2):
                t_.scatter_(2, torch.randint(0, N, (B, E, 1), generator=g), 1.0)
    Rr, Rs = Rr.to(DEV), Rs.to(DEV)
    if kind == "views":             # non-contiguous: a column window of a wider tensor / a transposed layout
        wide = torch.full((B, E, N + 3), 1.0, device=DEV)
        wide[:, :, 1:N + 1] = Rr
        Rr = wide[:, :, 1:N + 1]
        Rs = Rs.transpose(0, 1).contiguous().transpose(0, 1)
        assert (B * E == 1 or not Rr.is_contiguous()) and (B == 1 or E == 1 or not Rs.is_contiguous())
    if kind == "misaligned":        # contiguous, but starting 4 / 12 bytes into a 16-byte quad, with set bytes around the tensor
        def shifted(x, k):
            buf = torch.full((x.numel() + 8,), 1.0, device=DEV)
            v = buf[k:k + x.numel()].view(x.shape)
            v.copy_(x)
            assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k
            return v
        Rr, Rs = shifted(Rr, 1), shifted(Rs, 3)
    return Rr, Rs


def assert_same_csr(got, want, what):
    assert got.B == want.B and got.N == want.N, what
    assert got.row_ptr.dtype == torch.int32 and got.edge_recv.dtype == torch.int32 and got.edge_send.dtype == torch.int32
    assert torch.equal(got.row_ptr, want.row_ptr), f"row_ptr {what}"
    total = int(want.row_ptr[-1])
    assert torch.equal(got.edge_recv[:total], want.edge_recv[:total]), f"edge_recv {what}"
    assert torch.equal(got.edge_send[:total], want.edge_send[:total]), f"edge_send {what}"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_from_dense_equals_the_host_function(kind):
    for n, (B, E, N) in enumerate(SIZES):
        Rr, Rs = dense_case(kind, B, E, N, seed=n)
        got = aggraph.csr_from_dense_device(Rr, Rs)
        assert got.e_cap == B * E and got.edge_recv.numel() >= B * E
        assert_same_csr(got, aggraph.csr_from_dense(Rr, Rs), f"{kind} B={B} E={E} N={N}")


@pytest.mark.gpu
def test_from_dense_behind_more_than_256_scan_blocks():
    """66 066 receivers are 259 scan blocks, the last one partial: the blocks behind the 256th take a second trip through the strided sum of the
    partial sums in front of them."""
    B, E, N = 66, 7, 1001
    Rr, Rs = dense_case("padded", B, E, N, seed=5)
    got = aggraph.csr_from_dense_device(Rr, Rs)
    want = aggraph.csr_from_dense(Rr, Rs)
    assert int(want.row_ptr[256 * 256]) > 0 and int(want.row_ptr[-1]) > int(want.row_ptr[256 * 256])      # edges on both sides of block 256
    assert_same_csr(got, want, f"B={B} E={E} N={N}")


def built_graphs():
    for material, n_obj, batch, kw in (("rope", 93, 5, dict(spacing=0.1, n_pad=7)), ("cloth", 256, 2, {}), ("granular", 300, 2, {}),
                                       ("rope", 5, 2, dict(spacing=10.0))):
        g = synth.make_graph_inputs(material, n_obj, batch, seed=4, **kw)
        mm = synth.MATERIALS[material]
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        csr = aggraph.build_edges(t(g["state"][:, -1]), mm["radius"], t(g["mask"]), t(g["tool_mask"]), mm["topk"], mm["connect_tools_all"],
                                  "batch", max_tools=g["n_tools"])
        yield f"{material}{n_obj}x{batch}", csr


@pytest.mark.gpu
def test_round_trip_build_edges_to_dense_from_dense():
    for name, csr in built_graphs():
        Rr, Rs = csr.to_dense()
        assert_same_csr(aggraph.csr_from_dense_device(Rr, Rs), csr, name)
        k = Rr.shape[1] + 11                                      # ... and through the padded form
        Rr, Rs = csr.to_dense(e_max=k)
        assert_same_csr(aggraph.csr_from_dense_device(Rr, Rs), csr, name + " padded")


@pytest.mark.gpu
def test_from_dense_other_inputs_take_the_host_function():
    Rr, Rs = dense_case("padded", 2, 9, 12, seed=1)
    want = aggraph.csr_from_dense(Rr, Rs)
    assert aggraph.as_csr(want, None) is want
    assert aggraph.as_csr(Rr, Rs).e_cap == 2 * 9                                   # the device path (its capacity is the bound B E)
    assert_same_csr(aggraph.as_csr(Rr.double(), Rs.double()), want, "float64")      # the host function: any dtype ...
    host = aggraph.as_csr(Rr.cpu(), Rs.cpu())                                       # ... and any device
    assert not host.row_ptr.is_cuda and torch.equal(host.row_ptr, want.row_ptr.cpu())
    with pytest.raises(TypeError):
        aggraph.csr_from_dense_device(Rr.double(), Rs.double())
    empty = aggraph.csr_from_dense_device(Rr[:, :0], Rs[:, :0])                     # no relation rows at all
    assert empty.e_cap == 0 and int(empty.row_ptr.abs().sum()) == 0 and empty.row_ptr.numel() == 2 * 12 + 1


# ------------------------------------------------------------------------------------------ CSR -> dense
def to_dense_torch(csr, dtype=torch.float32):
    """CSREdges.to_dense as it was before the kernel (graph.py:146-155 layout): the expected value."""
    n = csr.n_rel()
    e_max = int(n.max().item()) if csr.B else 0
    total = int(csr.row_ptr[-1].item())
    dev = csr.row_ptr.device
    Rr = torch.zeros((csr.B, e_max, csr.N), dtype=dtype, device=dev)
    Rs = torch.zeros((csr.B, e_max, csr.N), dtype=dtype, device=dev)
    if total:
        r = csr.edge_recv[:total].long()
        s = csr.edge_send[:total].long()
        b = r // csr.N
        start = csr.row_ptr.long()[b * csr.N]
        idx = torch.arange(total, device=dev) - start
        Rr[b, idx, r - b * csr.N] = 1
        Rs[b, idx, s - b * csr.N] = 1
    return Rr, Rs


def csr_cases():
    yield from built_graphs()
    for B, E, N in ((3, 65, 108), (2, 7, 1), (1, 1, 5), (3, 500, 257), (2, 40, 1001), (2, 9, 253)):
        yield f"random {B}x{E}x{N}", aggraph.csr_from_dense(*dense_case("padded", B, E, N, seed=E))


@pytest.fixture(scope="module")
def dense_expected():
    return [(name, csr, to_dense_torch(csr)) for name, csr in csr_cases()]


@pytest.mark.gpu
def test_to_dense_equals_the_torch_construction(dense_expected):
    for name, csr, (Rr0, Rs0) in dense_expected:
        Rr, Rs = csr.to_dense()
        assert Rr.dtype == torch.float32 and Rr.shape == Rr0.shape and Rs.shape == Rs0.shape, name
        assert torch.equal(Rr, Rr0) and torch.equal(Rs, Rs0), name
        assert int(csr.overflow) == 0, name
        Rh, _ = csr.to_dense(torch.float64)
        assert Rh.dtype == torch.float64 and torch.equal(Rh, Rr0.double()), name
    csr = aggraph.csr_from_dense(*dense_case("all_zero", 2, 5, 6, seed=0))          # no edge anywhere: (B, 0, N), as before
    Rr, Rs = csr.to_dense()
    assert Rr.shape == (2, 0, 6) and Rs.shape == (2, 0, 6) and int(csr.overflow) == 0


@pytest.mark.gpu
def test_to_dense_e_max_pads_like_pad_torch(dense_expected):
    for name, csr, (Rr0, Rs0) in dense_expected:
        for extra in (0, 1, 37):
            k = Rr0.shape[1] + extra
            if k == 0:
                continue
            Rr, Rs = csr.to_dense(e_max=k)
            pad = torch.zeros(csr.B, extra, csr.N, device=DEV)                  # pad_torch(x, max_nR): zero rows behind (utils.py:37-46)
            assert torch.equal(Rr, torch.cat([Rr0, pad], 1)) and torch.equal(Rs, torch.cat([Rs0, pad], 1)), (name, k)
            assert csr.overflow.is_cuda and csr.overflow.dtype == torch.int32 and int(csr.overflow) == 0, (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("guard", [256, 260, 268])       # outputs 16-byte aligned, and 4 / 12 bytes into a quad
def test_to_dense_overflow_drops_the_surplus_and_stays_inside_its_outputs(dense_expected, guard):
    L = _lib.lib()
    for name, csr, (Rr0, Rs0) in dense_expected:
        e_full = Rr0.shape[1]
        for k in sorted({1, e_full // 2, e_full - 1} - {0}):
            if k >= e_full:
                continue
            nbytes = csr.B * k * csr.N * 4
            bufs = [torch.full((guard + nbytes + guard,), 0xFF, dtype=torch.uint8, device=DEV) for _ in range(2)]
            ovf = torch.full((3,), -1, dtype=torch.int32, device=DEV)
            rc = L.ag_edges_to_dense(csr.row_ptr.data_ptr(), csr.edge_recv.data_ptr(), csr.edge_send.data_ptr(), csr.B, csr.N, k,
                                     bufs[0].data_ptr() + guard, bufs[1].data_ptr() + guard, ovf.data_ptr() + 4, None)
            assert rc == 0, L.ag_last_error()
            torch.cuda.synchronize()
            assert ovf.tolist() == [-1, 1, -1], (name, k)
            for buf, want in zip(bufs, (Rr0, Rs0)):
                assert bool((buf[:guard] == 0xFF).all()) and bool((buf[guard + nbytes:] == 0xFF).all()), f"guard touched: {name} k={k}"
                got = buf[guard:guard + nbytes].clone().view(torch.float32).view(csr.B, k, csr.N)
                assert torch.equal(got, want[:, :k]), (name, k)
    csr = dense_expected[0][1]
    csr.to_dense(e_max=1)
    assert int(csr.overflow) == 1


@pytest.mark.gpu
def test_to_dense_checks_the_node_ids_it_reads():
    """Ids outside their sample leave the row zero; nothing is written outside the outputs."""
    B, N = 2, 6
    row_ptr = torch.tensor([0, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 4], dtype=torch.int32, device=DEV)
    recv = torch.tensor([0, 0, 6, 11], dtype=torch.int32, device=DEV)
    send = torch.tensor([5, 6, -3, 2 ** 31 - 1], dtype=torch.int32, device=DEV)          # 6: next sample's node; -3, INT_MAX: nowhere
    csr = aggraph.CSREdges(row_ptr, recv, send, B, N, 4)
    Rr, Rs = csr.to_dense(e_max=3)
    want_r = torch.zeros(B, 3, N, device=DEV)
    want_s = torch.zeros(B, 3, N, device=DEV)
    want_r[0, 0, 0] = want_r[0, 1, 0] = want_r[1, 0, 0] = want_r[1, 1, 5] = 1
    want_s[0, 0, 5] = 1
    assert torch.equal(Rr, want_r) and torch.equal(Rs, want_s)


# ------------------------------------------------------------------------------------------ forward on dense inputs
PRECISIONS = {"fast": 2, "bf16x3": 1, "f32": 0}


def make_model(weights, prec):
    from adaptigraph_amd.model import DynamicsPredictor
    m = DynamicsPredictor(configs.model_config(), configs.material_config("rope"), configs.dataset_config("rope"), DEV)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in weights.items()})
    m = m.to(DEV).eval()
    m.set_option("precision", PRECISIONS[prec])
    return m


def rope_graph(n_obj, batch, seed, **kw):
    """(reference-format graph dict without Rr / Rs, its CSREdges)"""
    g = synth.make_graph_inputs("rope", n_obj, batch, seed=seed, spacing=0.1, **kw)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    csr = aggraph.build_edges(t(g["state"][:, -1]), 0.5, t(g["mask"]), t(g["tool_mask"]), 10, False, "batch", max_tools=1)
    graph = dict(state=t(g["state"]), attrs=t(g["attrs"]), p_instance=t(g["p_instance"]), action=t(g["action"]), rope_physics_param=t(g["phys"]),
                 obj_mask=None)
    return graph, csr, g


@pytest.mark.gpu
@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_forward_on_dense_inputs_is_bitwise_the_forward_on_their_csr(weights, prec, monkeypatch):
    m = make_model(weights, prec)
    for n_obj, batch, kw in ((93, 5, dict(n_pad=7)), (300, 2, {})):
        graph, csr, _ = rope_graph(n_obj, batch, 4, **kw)
        want = m(Rr=csr, Rs=None, **graph)
        for k in (None, int(csr.n_rel().max()) + 29):
            Rr, Rs = csr.to_dense(e_max=k)
            got = m(Rr=Rr, Rs=Rs, **graph)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (n_obj, k)
            with monkeypatch.context() as mp:                   # ... and the forward with the host conversion in its place
                mp.setattr(aggraph, "csr_from_dense_device", aggraph.csr_from_dense)
                host = m(Rr=Rr, Rs=Rs, **graph)
            assert torch.equal(got[0], host[0]) and torch.equal(got[1], host[1]), (n_obj, k)
    # an all-zero pair: no edge at all, the forward still runs
    graph, csr, _ = rope_graph(40, 2, 1)
    N = graph["attrs"].shape[1]
    empty = aggraph.CSREdges(torch.zeros(2 * N + 1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                             torch.zeros(1, dtype=torch.int32, device=DEV), 2, N, 0)
    want = m(Rr=empty, Rs=None, **graph)
    z = torch.zeros(2, 17, N, device=DEV)
    got = m(Rr=z, Rs=z.clone(), **graph)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert m.take_status() == 0


# ------------------------------------------------------------------------------------------ capture, no host synchronisation
@pytest.mark.gpu
def test_forward_on_dense_inputs_is_hip_graph_capturable(weights):
    """model(**graph) with the reference's dense Rr / Rs records into a HIP graph; replays follow the edges in the input buffers."""
    m = make_model(weights, "fast")
    graph, csr1, _ = rope_graph(93, 5, 4, n_pad=7)
    _, csr2, _ = rope_graph(93, 5, 9, n_pad=7)
    K = int(max(csr1.n_rel().max(), csr2.n_rel().max())) + 5
    dense = [c.to_dense(e_max=K) for c in (csr1, csr2)]
    assert not torch.equal(dense[0][0], dense[1][0])
    want = [tuple(x.clone() for x in m(Rr=c, Rs=None, **graph)) for c in (csr1, csr2)]
    Rr, Rs = dense[0][0].clone(), dense[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(Rr=Rr, Rs=Rs, **graph)
    torch.cuda.current_stream().wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        pos, mot = m(Rr=Rr, Rs=Rs, **graph)
    for which in (1, 0, 1):
        Rr.copy_(dense[which][0])
        Rs.copy_(dense[which][1])
        pos.zero_()
        mot.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(pos, want[which][0]) and torch.equal(mot, want[which][1]), which
    assert m.take_status() == 0


@pytest.mark.gpu
def test_construct_edges_batch_with_bounds_is_hip_graph_capturable():
    _, csr1, g1 = rope_graph(93, 5, 4, n_pad=7)
    _, csr2, g2 = rope_graph(93, 5, 9, n_pad=7)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    pos = [t(g["state"][:, -1]) for g in (g1, g2)]
    mask, tool = t(g1["mask"]), t(g1["tool_mask"])
    K = int(max(csr1.n_rel().max(), csr2.n_rel().max())) + 5
    call = lambda p: aggraph.construct_edges_from_states_batch(p, 0.5, mask, tool, topk=10, connect_tools_all=False, max_tools=1, max_nR=K)
    want = [tuple(x.clone() for x in call(p)) for p in pos]
    for (Rr, Rs), p in zip(want, pos):          # the bounded call is the default call, padded
        Rr0, Rs0 = aggraph.construct_edges_from_states_batch(p, 0.5, mask, tool, topk=10, connect_tools_all=False)
        assert Rr.shape == (5, K, Rr0.shape[2]) and torch.equal(Rr[:, :Rr0.shape[1]], Rr0) and torch.equal(Rs[:, :Rs0.shape[1]], Rs0)
        assert int(Rr[:, Rr0.shape[1]:].abs().sum()) == 0 and int(Rs[:, Rs0.shape[1]:].abs().sum()) == 0
    assert not torch.equal(want[0][0], want[1][0])
    cur = pos[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(cur)
    torch.cuda.current_stream().wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=side):
        Rr, Rs = call(cur)
    for which in (1, 0, 1):
        cur.copy_(pos[which])
        Rr.fill_(7.0)
        Rs.fill_(7.0)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(Rr, want[which][0]) and torch.equal(Rs, want[which][1]), which
    # the single-graph form with both bounds: the default call's rows, padded
    one = aggraph.construct_edges_from_states(pos[0][0], 0.5, mask[0], tool[0], topk=10, connect_tools_all=False)
    pad = aggraph.construct_edges_from_states(pos[0][0], 0.5, mask[0], tool[0], topk=10, connect_tools_all=False, max_tools=1, max_nR=K)
    n = one[0].shape[0]
    assert pad[0].shape == (K, one[0].shape[1]) and torch.equal(pad[0][:n], one[0]) and torch.equal(pad[1][:n], one[1]) and int(pad[0][n:].abs().sum()) == 0


@pytest.mark.gpu
def test_device_conversions_do_not_synchronise_the_host():
    Rr, Rs = dense_case("padded", 3, 65, 108, seed=2)
    want = aggraph.csr_from_dense(Rr, Rs)
    dense_want = to_dense_torch(want)
    aggraph.csr_from_dense_device(Rr, Rs)          # (first call: the scratch buffer is allocated)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = aggraph.csr_from_dense_device(Rr, Rs)
        dense = got.to_dense(e_max=70)
        one = aggraph.construct_edges_from_states_batch(torch.zeros(2, 6, 3, device=DEV), 0.5, torch.ones(2, 6, dtype=torch.bool, device=DEV),
                                                        torch.zeros(2, 6, dtype=torch.bool, device=DEV), max_tools=1, max_nR=40)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert_same_csr(got, want, "under sync-debug")
    assert torch.equal(dense[0][:, :dense_want[0].shape[1]], dense_want[0]) and torch.equal(dense[1][:, :dense_want[1].shape[1]], dense_want[1])
    assert int(got.overflow) == 0 and one[0].shape == (2, 40, 6)
