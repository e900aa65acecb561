"""Radius-graph / top-k adjacency on the HIP engine.

Drop-in for src/dynamics/dataset/graph.py: `construct_edges_from_states(...)` (:38-89) and
`construct_edges_from_states_batch(...)` (:91-156) keep the reference's signatures and dense
one-hot `(Rr, Rs)` return value; `build_edges(...)` is the native fast path returning the CSR
adjacency the kernels consume (no O(E*N) one-hots, no host sync).
"""
import numpy as np
import torch

from . import _lib
from ._lib import _WS, _require_gpu, _stream_ptr, _u8, workspace  # noqa: F401  (their home is _lib; tests and older callers reach them here)


class CSREdges:
    """Receiver-sorted adjacency of a batch of graphs, as produced by ag_build_edges.

    row_ptr (B*N+1,) int32 over global rows b*N+i; edge_recv / edge_send (e_cap,) int32 global node ids;
    only the first row_ptr[-1] entries are valid.  Edge order == the reference's nonzero() order.
    """

    def __init__(self, row_ptr, edge_recv, edge_send, B, N, e_cap):
        self.row_ptr, self.edge_recv, self.edge_send = row_ptr, edge_recv, edge_send
        self.B, self.N, self.e_cap = B, N, e_cap

    def n_rel(self):
        """(B,) int64 edge count per sample (device tensor)."""
        rp = self.row_ptr.long()
        return rp[self.N::self.N][:self.B] - rp[0:self.B * self.N:self.N]

    def to_lists(self):
        """[(recv_local, send_local) numpy int32 arrays] per sample (host sync; tests / debugging)."""
        rp = self.row_ptr.cpu().numpy()
        r = self.edge_recv.cpu().numpy()
        s = self.edge_send.cpu().numpy()
        out = []
        for b in range(self.B):
            lo, hi = rp[b * self.N], rp[(b + 1) * self.N]
            out.append((r[lo:hi] - b * self.N, s[lo:hi] - b * self.N))
        return out

    def to_dense(self, dtype=torch.float32, e_max=None):
        """(Rr, Rs) one-hot (B, e_max, N) exactly as graph.py:146-155 lays them out, written by ag_edges_to_dense.

        e_max=None: the batch maximum of n_rel, the reference's shape (one host read).  An integer e_max pads to that many rows — the
        reference's pad_torch(Rr, max_nR) in the same step — with no host synchronisation (safe to capture); a sample with more edges
        loses the surplus ones.  Either way `self.overflow` is then a device int32 word: 1 if some sample had more than e_max edges.
        (An adjacency in host memory — csr_from_dense of CPU tensors — gets the same tensors from torch indexing.)"""
        dev = self.row_ptr.device
        if e_max is None:
            e_max = int(self.n_rel().max().item()) if self.B else 0
        e_max = int(e_max)
        if not self.row_ptr.is_cuda:
            return self._to_dense_host(dtype, e_max)
        Rr = torch.empty((self.B, e_max, self.N), dtype=torch.float32, device=dev)
        Rs = torch.empty((self.B, e_max, self.N), dtype=torch.float32, device=dev)
        if Rr.numel() == 0:
            self.overflow = (self.row_ptr[-1:] > 0).to(torch.int32)
            return Rr.to(dtype), Rs.to(dtype)
        self.overflow = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.call("ag_edges_to_dense", dev, self.row_ptr, self.edge_recv, self.edge_send, self.B, self.N, e_max, Rr, Rs, self.overflow)
        return Rr.to(dtype), Rs.to(dtype)

    def _to_dense_host(self, dtype, e_max):
        """to_dense of an adjacency held in host memory (csr_from_dense of CPU tensors): the same tensors by torch indexing."""
        n = self.n_rel()
        self.overflow = (n > e_max).any().to(torch.int32).reshape(1)
        Rr = torch.zeros((self.B, e_max, self.N), dtype=dtype)
        Rs = torch.zeros((self.B, e_max, self.N), dtype=dtype)
        total = int(self.row_ptr[-1].item())
        if total and e_max:
            r = self.edge_recv[:total].long()
            s = self.edge_send[:total].long()
            b = r // self.N
            idx = torch.arange(total) - self.row_ptr.long()[b * self.N]
            keep = idx < e_max
            b, idx, r, s = b[keep], idx[keep], r[keep], s[keep]
            Rr[b, idx, r - b * self.N] = 1
            Rs[b, idx, s - b * self.N] = 1
        return Rr, Rs


def threshold_sq(adj_thresh, B, device, variant):
    """Squared radius per sample, rounded the way the chosen builder variant rounds it:
    single: Python double r*r, cast to fp32 by the tensor-scalar subtraction (graph.py:53,68);
    batch:  fp32 tensor r * r (graph.py:106-108)."""
    if torch.is_tensor(adj_thresh):
        t = adj_thresh.to(device=device, dtype=torch.float32).reshape(-1)
        if t.numel() == 1:
            t = t.repeat(B)
        return (t * t).contiguous()
    if isinstance(adj_thresh, (list, tuple, np.ndarray)):     # one host double per sample (e.g. radii drawn by a dataset)
        r = np.asarray(adj_thresh, np.float64).reshape(-1)
        assert r.size == B, f"{r.size} radii for {B} samples"
        v = (r * r).astype(np.float32) if variant == _lib.AG_VARIANT_SINGLE else r.astype(np.float32) * r.astype(np.float32)
        return torch.from_numpy(np.ascontiguousarray(v)).to(device)
    r = float(adj_thresh)
    if variant == _lib.AG_VARIANT_SINGLE:
        v = np.float32(r * r)
    else:
        v = np.float32(r) * np.float32(r)
    return torch.full((B,), float(v), dtype=torch.float32, device=device)


def build_edges(states, adj_thresh, mask, tool_mask, topk=10, connect_tools_all=False, variant="batch",
                max_tools=None):
    """states (B,N,3) fp32 cuda; mask, tool_mask (B,N) bool -> CSREdges.  No host synchronisation when
    `max_tools` is given (default: N, always sufficient)."""
    _require_gpu(states, "states")
    L = _lib.lib()
    B, N, _ = states.shape
    dev = states.device
    var = _lib.AG_VARIANT_SINGLE if variant == "single" else _lib.AG_VARIANT_BATCH
    states = states.contiguous().float()
    mask_u8, tool_u8 = _u8(mask, dev), _u8(tool_mask, dev)
    thr = threshold_sq(adj_thresh, B, dev, var)
    if max_tools is None:
        max_tools = N
    connect = 1 if connect_tools_all else 0
    e_cap = int(L.ag_edge_capacity(B, N, int(topk), connect, int(max_tools)))
    row_ptr = torch.empty(B * N + 1, dtype=torch.int32, device=dev)
    edge_recv = torch.empty(max(e_cap, 1), dtype=torch.int32, device=dev)
    edge_send = torch.empty(max(e_cap, 1), dtype=torch.int32, device=dev)
    nbytes = L.ag_edges_workspace_bytes(B, N, int(topk), connect, int(max_tools))
    ws = workspace(dev, nbytes)
    _lib.call("ag_build_edges", dev, states, mask_u8, tool_u8, thr, int(topk), connect, var, B, N, int(max_tools), row_ptr, edge_recv, edge_send,
              e_cap, ws, ws.numel())
    return CSREdges(row_ptr, edge_recv, edge_send, B, N, e_cap)


def construct_edges_from_states(states, adj_thresh, mask, tool_mask, topk=10, connect_tools_all=False, max_tools=None, max_nR=None):
    """Drop-in for graph.py:38-89: states (N,3) -> (Rr, Rs) of shape (n_rel, N).
    Two optional bounds make the call free of host reads (safe to capture): `max_tools` >= the number of tool slots (else counted, one
    read) and `max_nR`, the row count to pad to (else n_rel, one read) — see CSREdges.to_dense."""
    n_tools = int(tool_mask.sum().item()) if max_tools is None else int(max_tools)
    csr = build_edges(states[None], adj_thresh, mask[None], tool_mask[None], topk, connect_tools_all, "single",
                      max_tools=n_tools)
    Rr, Rs = csr.to_dense(states.dtype, e_max=max_nR)
    return Rr[0], Rs[0]


def construct_edges_from_states_batch(states, adj_thresh, mask, tool_mask, topk=10, connect_tools_all=False, max_tools=None, max_nR=None):
    """Drop-in for graph.py:91-156: states (B,N,3) -> (Rr, Rs) of shape (B, max n_rel, N); `max_tools` / `max_nR` as in
    construct_edges_from_states (with `max_nR` the shape is (B, max_nR, N): the reference's pad_torch(Rr, max_nR) included)."""
    n_tools = int(tool_mask.sum(1).max().item()) if max_tools is None else int(max_tools)
    csr = build_edges(states, adj_thresh, mask, tool_mask, topk, connect_tools_all, "batch", max_tools=n_tools)
    return csr.to_dense(states.dtype, e_max=max_nR)


def csr_from_dense(Rr, Rs):
    """One-hot (B,E,N) pair -> CSREdges (compat path of DynamicsPredictor.forward; host sync).
    All-zero (padded) rows are dropped, which is exact (truncate_graph / pad_torch vanish);
    edges are stably re-sorted by receiver because the kernels reduce over CSR rows."""
    B, E, N = Rr.shape
    dev = Rr.device
    valid = (Rr.sum(-1) > 0) & (Rs.sum(-1) > 0)
    b_idx = torch.arange(B, device=dev)[:, None].expand(B, E)
    recv = (Rr.argmax(-1) + b_idx * N)[valid]
    send = (Rs.argmax(-1) + b_idx * N)[valid]
    order = torch.sort(recv, stable=True).indices
    recv, send = recv[order], send[order]
    counts = torch.bincount(recv, minlength=B * N)
    row_ptr = torch.zeros(B * N + 1, dtype=torch.int32, device=dev)
    row_ptr[1:] = torch.cumsum(counts, 0).int()
    total = int(recv.numel())
    return CSREdges(row_ptr, recv.int().contiguous() if total else torch.zeros(1, dtype=torch.int32, device=dev),
                    send.int().contiguous() if total else torch.zeros(1, dtype=torch.int32, device=dev), B, N,
                    max(total, 1) if total else 0)


def csr_from_dense_device(Rr, Rs):
    """csr_from_dense for CUDA fp32 pairs as HIP kernels (ag_edges_from_dense, csrc/ag_dense.hip): the same row_ptr / edge_recv /
    edge_send in every bit, with no host read (safe to capture).  The edge count stays on the device, so e_cap is the bound B*E."""
    _require_gpu(Rr, "Rr")
    _require_gpu(Rs, "Rs")
    if Rr.dtype != torch.float32 or Rs.dtype != torch.float32:
        raise TypeError(f"csr_from_dense_device reads float32 (got {Rr.dtype}, {Rs.dtype}); csr_from_dense takes any dtype")
    assert Rr.shape == Rs.shape and Rr.dim() == 3, f"Rr {tuple(Rr.shape)} / Rs {tuple(Rs.shape)}"
    assert Rr.device == Rs.device, f"Rr on {Rr.device}, Rs on {Rs.device}"
    B, E, N = Rr.shape
    dev = Rr.device
    row_ptr = torch.empty(B * N + 1, dtype=torch.int32, device=dev)
    edge_recv = torch.empty(max(B * E, 1), dtype=torch.int32, device=dev)
    edge_send = torch.empty(max(B * E, 1), dtype=torch.int32, device=dev)
    if B * E * N == 0:
        return CSREdges(row_ptr.zero_(), edge_recv.zero_(), edge_send.zero_(), B, N, 0)
    Rr, Rs = Rr.contiguous(), Rs.contiguous()
    L = _lib.lib()
    ws = workspace(dev, L.ag_dense_edges_workspace_bytes(B, E, N))
    _lib.call("ag_edges_from_dense", dev, Rr, Rs, B, E, N, row_ptr, edge_recv, edge_send, ws, ws.numel())
    return CSREdges(row_ptr, edge_recv, edge_send, B, N, B * E)


def as_csr(Rr, Rs):
    """The adjacency of a forward call: a CSREdges as it is, a CUDA fp32 one-hot pair through the kernels, anything else through the host function."""
    if isinstance(Rr, CSREdges):
        return Rr
    if Rr.is_cuda and Rs.device == Rr.device and Rr.dtype == torch.float32 and Rs.dtype == torch.float32:
        return csr_from_dense_device(Rr, Rs)
    return csr_from_dense(Rr, Rs)
