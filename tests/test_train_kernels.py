"""The training kernels at real shapes and edges, exactly: the split-K weight / bias gradient kernels (csrc/ag_train.hip), the
fused dense chains (csrc/ag_chain.hip) and the graph operators of train_ops, each against plain float64 torch.

Method.  Every kernel here is sums of products, ReLU and masks.  With small-integer-valued fp32 inputs every product and every
partial sum is an integer below 2^24, so the fp32 result equals the float64 reference BIT FOR BIT in any summation order: the
backbone is `torch.equal(got.double(), ref)`, no tolerance — one dropped or doubled row of a 10^5-row contraction, or a wrong
clamp in the last partial slab, changes an integer.  For the split-bf16 chains (x = hi + lo, lo * lo dropped) the weights must
have a zero lo half (integers in -2..2, sparse rows) and the activations must be integers below 2^16, for which hi + lo is exact.
Each exact case asserts these bounds on the reference side, so a case that outgrows exactness fails loudly.  Integer data also
sits on the ReLU kink (pre == 0) and the |g_r - g_s| == 0 kink all the time: relu'(0) = 0 and sign(0) = 0, as in torch.
Beside each exact family one or two random-float cases run under the gates the suite already has (chains 2e-5 / 1e-4, graph
adjoints 1e-5); the bare weight-gradient kernel has no gate in the project, so its float case uses the derived bound of an
fp32 dot product of length K in any order, |err| <= K 2^-24 (|dz|^T |prev|) with K = rows + slabs.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from adaptigraph_amd import _lib

DEV = "cuda:0"
EXACT_F32 = 2 ** 24          # integers below this are exact in fp32, and so is any sum of them that stays below it
EXACT_SPLIT = 2 ** 16        # integers up to this are exactly hi + lo in two bf16 halves (first inexact integer: 131 329)
FP = 160


def make_gen(seed, dev):
    return torch.Generator(device=dev).manual_seed(seed)


def ints(gen, shape, lo, hi, dev):
    """Integer-valued fp32 in [lo, hi]."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen, device=dev).float()


def floats(gen, shape, dev):
    return torch.randn(tuple(shape), generator=gen, device=dev)


# =====================================================================================================================
# 1. Weight and bias gradients: dw_partial_kernel / dw_reduce_kernel
# =====================================================================================================================
# layer = (n_out, n_in, dz_ld, prev layout).  prev layouts: "tight" (ld = n_in), "160" (ld = 160, columns >= n_in poisoned),
# "slice" (a column slice of a wider table, ld = n_in + 37).  n_in + 1 <= 32 takes the one-tile row loop, above it the five-tile one.
SPECS = {
    "A": [(150, 1, 160, "tight"), (150, 31, 150, "160"), (3, 150, 3, "slice"), (150, 33, 160, "tight")],
    "B": [(150, 6, 160, "160"), (150, 32, 160, "slice"), (150, 149, 150, "tight"), (150, 30, 160, "160")],
    "C": [(150, 17, 160, "tight"), (150, 150, 160, "160"), (3, 150, 3, "160")],
    "D": [(150, 150, 150, "slice"), (150, 31, 160, "tight")],
    "E": [(150, 150, 160, "160")],
    "F": [(150, 32, 160, "tight")],
}
SMALL_ROWS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129]
# rows chosen by slab count (1 / 2 slabs are among the small rows): (rows, spec) -> slabs, slab size class
SLAB_CASES = [(512, "E"), (513, "F"), (1037, "D"), (7000, "C"), (30011, "D"), (20000, "A"), (210001, "B")]
DW_CASES = [(r, s) for r in SMALL_ROWS for s in ("A", "B")] + SLAB_CASES
DW_MAX_ABS = 3               # |dz|, |prev| <= 3: every partial sum of a case is below rows * 9 (+ rows * 3 for the bias column)
SLAB_COUNT_CLASSES = {"1": lambda s: s == 1, "2": lambda s: s == 2, "8": lambda s: s == 8, "9": lambda s: s == 9,
                      "17": lambda s: s == 17, ">=100": lambda s: s >= 100}


def slab_count(rows, n_layers):
    """Slabs of one weight-gradient call, through the public workspace query (one 160 x 160 fp32 partial per slab and layer)."""
    nbytes = _lib.lib().ag_train_weight_grads_workspace_bytes(rows, n_layers)
    assert nbytes % (n_layers * FP * FP * 4) == 0
    return nbytes // (n_layers * FP * FP * 4)


def slab_size_class(rows, n_layers):
    """Where the slab size sits, from the slab count alone: the documented floor is 64 rows per slab and the cap 2048."""
    s = slab_count(rows, n_layers)
    if s == -(-rows // 64):
        return "floor"
    if s == -(-rows // 2048):
        return "cap"
    assert -(-rows // 2048) < s < -(-rows // 64)
    return "between"


def test_weight_grad_case_table_covers_every_slab_class():
    """If the slab heuristic of ag_train.hip changes, this says which coverage moved (the GPU cases take rows from this table)."""
    counts = [slab_count(r, len(SPECS[s])) for r, s in DW_CASES if r > 0]
    for name, hit in SLAB_COUNT_CLASSES.items():
        assert any(hit(c) for c in counts), f"no case with {name} slabs: {sorted(set(counts))}"
    assert slab_count(0, 4) == 1 and slab_count(64, 4) == 1 and slab_count(65, 4) == 2 and slab_count(129, 4) == 3
    sizes = {slab_size_class(r, len(SPECS[s])) for r, s in SLAB_CASES}
    assert sizes == {"floor", "between", "cap"}, sizes
    assert slab_size_class(210001, 4) == "cap" and slab_count(210001, 4) > 100      # the 2048-row cap, partial last slab
    assert 210001 % 2048 not in (0, 2047) and 513 % 64 == 1 and 512 % 64 == 0          # last slab: partial, one row, full
    assert {len(v) for v in SPECS.values()} == {1, 2, 3, 4}
    assert {l[1] for v in SPECS.values() for l in v} == {1, 6, 17, 30, 31, 32, 33, 149, 150}
    assert {l[2] for v in SPECS.values() for l in v} == {3, 150, 160}
    assert {l[3] for v in SPECS.values() for l in v} == {"tight", "160", "slice"}
    for v in SPECS.values():
        assert all(n_out <= dz_ld <= FP and n_in <= 150 for n_out, n_in, dz_ld, _ in v)
    for r, s in DW_CASES:      # the integer bound on the reference side, for any data the builder can draw
        assert r * DW_MAX_ABS * DW_MAX_ABS < EXACT_F32


def dw_tables(rows, spec, gen, dev, real=False):
    """Tables of one call.  What must not be read is NaN: rows >= `rows` of every table, prev columns >= n_in where ld > n_in
    (and the wider table around a slice); dz columns >= n_out hold finite junk, which lands outside the documented block."""
    dzs, prevs, n_ins = [], [], []
    draw = (lambda shape: floats(gen, shape, dev)) if real else (lambda shape: ints(gen, shape, -DW_MAX_ABS, DW_MAX_ABS, dev))
    for n_out, n_in, dz_ld, layout in SPECS[spec]:
        dz = torch.full((rows + 3, dz_ld), float("nan"), device=dev)
        dz[:rows, :n_out] = draw((rows, n_out))
        if dz_ld > n_out:
            dz[:rows, n_out:] = torch.rand((rows, dz_ld - n_out), generator=gen, device=dev) * 2e3 - 1e3
        ld, off = {"tight": (n_in, 0), "160": (FP, 0), "slice": (n_in + 37, 5)}[layout]
        tab = torch.full((rows + 3, ld), float("nan"), device=dev)
        tab[:rows, off:off + n_in] = draw((rows, n_in))
        prev = tab[:, off:off + n_in]
        assert prev.stride(1) == 1 and prev.stride(0) == ld and dz.stride(0) == dz_ld
        dzs.append(dz); prevs.append(prev); n_ins.append(n_in)
    return dzs, prevs, n_ins


def dw_reference(dzs, prevs, rows, spec):
    """float64 dz^T prev and column sums, and the magnitude sums |dz|^T |prev| that bound every partial sum."""
    out = []
    for dz, prev, (n_out, n_in, _, _) in zip(dzs, prevs, SPECS[spec]):
        z, p = dz[:rows, :n_out].double(), prev[:rows].double()
        out.append((z.T @ p, z.sum(0), z.abs().T @ p.abs(), z.abs().sum(0)))
    return out


def dw_id(case):
    return f"{case[0]}-{case[1]}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", DW_CASES, ids=dw_id)
def test_weight_grads_exact_vs_float64(case):
    """out[l, :n_out, :n_in] = dz^T prev and out[l, :n_out, n_in] = column sums of dz, bit for bit, with poisoned surroundings;
    two calls give the same bits."""
    from adaptigraph_amd import train_ops
    rows, spec = case
    dzs, prevs, n_ins = dw_tables(rows, spec, make_gen(rows + 1, DEV), DEV)
    out = train_ops.weight_grads(dzs, prevs, n_ins, rows)
    again = train_ops.weight_grads(dzs, prevs, n_ins, rows)
    assert out.shape == (len(dzs), FP, FP)
    for l, (rw, rb, mw, mb) in enumerate(dw_reference(dzs, prevs, rows, spec)):
        n_out, n_in = SPECS[spec][l][:2]
        assert max(mw.max().item(), mb.max().item()) < EXACT_F32          # exactness precondition, reference side
        assert torch.equal(out[l, :n_out, :n_in].double(), rw), (l, (out[l, :n_out, :n_in].double() - rw).abs().max().item())
        assert torch.equal(out[l, :n_out, n_in].double(), rb), (l, (out[l, :n_out, n_in].double() - rb).abs().max().item())
        assert torch.equal(out[l, :n_out, :n_in + 1], again[l, :n_out, :n_in + 1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(7000, "C"), (210001, "B")], ids=dw_id)
def test_weight_grads_random_floats_within_derived_bound(case):
    """Random floats: |err| <= K 2^-24 (|dz|^T |prev|) elementwise, K = rows + slabs (an fp32 dot product of length K in any
    order; the slab sums add one more term per slab).  Prints the observed ratio to that bound."""
    from adaptigraph_amd import train_ops
    rows, spec = case
    dzs, prevs, n_ins = dw_tables(rows, spec, make_gen(5, DEV), DEV, real=True)
    out = train_ops.weight_grads(dzs, prevs, n_ins, rows)
    K = rows + slab_count(rows, len(dzs))
    worst = 0.0
    for l, (rw, rb, mw, mb) in enumerate(dw_reference(dzs, prevs, rows, spec)):
        n_out, n_in = SPECS[spec][l][:2]
        got = torch.cat([out[l, :n_out, :n_in], out[l, :n_out, n_in:n_in + 1]], 1).double()
        ref, mag = torch.cat([rw, rb[:, None]], 1), torch.cat([mw, mb[:, None]], 1)
        assert torch.isfinite(got).all()
        ratio = ((got - ref).abs() / (K * 2.0 ** -24 * mag)).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (l, ratio)
    print(f"weight_grads float case rows={rows} spec={spec}: worst |err| / bound = {worst:.3e}")


def call_into(dzs, prevs, n_ins, rows, w_dsts, b_dsts, n_outs):
    """ag_train_weight_grads_into, called directly: accumulate into w_dsts (views: row stride = stride(0)) and b_dsts (None = null)."""
    from adaptigraph_amd import graph, train_ops
    L, n, dev = _lib.lib(), len(dzs), dzs[0].device
    ws = graph.workspace(dev, L.ag_train_weight_grads_workspace_bytes(rows, n))
    i32 = lambda v: (ctypes.c_int32 * 4)(*(list(v) + [0] * (4 - n)))
    pv = lambda v: (ctypes.c_void_p * 4)(*(list(v) + [None] * (4 - n)))
    with torch.cuda.device(dev):
        rc = L.ag_train_weight_grads_into(n, train_ops._ptr_array(dzs), i32(t.stride(0) for t in dzs), train_ops._ptr_array(prevs),
                                          i32(t.stride(0) for t in prevs), i32(n_ins), rows, None, pv(w.data_ptr() for w in w_dsts),
                                          i32(w.stride(0) for w in w_dsts), pv(b.data_ptr() if b is not None else None for b in b_dsts),
                                          i32(n_outs), ws.data_ptr(), ws.numel(), graph._stream_ptr(dev))
    _lib.check(rc, "ag_train_weight_grads_into")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(129, "A"), (7000, "C"), (30011, "D")], ids=dw_id)
def test_weight_grads_into_accumulates_only_inside_the_block(case):
    """The accumulating entry point: destinations pre-filled with random values, weight blocks that are strided slices of wider
    tables (one tight), one null bias.  Result = pre + (the `out` mode result), one fp32 add per element, bit for bit; every
    element outside the n_out x n_in block and every bias guard element is untouched."""
    from adaptigraph_amd import train_ops
    rows, spec = case
    gen = make_gen(11, DEV)
    dzs, prevs, n_ins = dw_tables(rows, spec, gen, DEV)
    out = train_ops.weight_grads(dzs, prevs, n_ins, rows)
    n = len(dzs)
    wides, w_dsts, biases, b_dsts = [], [], [], []
    for l, (n_out, n_in, _, _) in enumerate(SPECS[spec]):
        tight = l == n - 1                                      # the last layer: a plain contiguous parameter
        wide = floats(gen, (n_out, n_in) if tight else (n_out + 2, n_in + 9), DEV)
        wides.append(wide)
        w_dsts.append(wide if tight else wide[1:1 + n_out, 4:4 + n_in])
        bias = floats(gen, (n_out + 2,), DEV)
        biases.append(bias)
        b_dsts.append(None if l == 0 else bias[1:1 + n_out])   # layer 0 has no bias destination
    before_w, before_b = [w.clone() for w in wides], [b.clone() for b in biases]
    call_into(dzs, prevs, n_ins, rows, w_dsts, b_dsts, [s[0] for s in SPECS[spec]])
    for l, (n_out, n_in, _, _) in enumerate(SPECS[spec]):
        want_w, want_b = before_w[l].clone(), before_b[l].clone()
        blk = want_w if l == n - 1 else want_w[1:1 + n_out, 4:4 + n_in]
        blk += out[l, :n_out, :n_in]
        if b_dsts[l] is not None:
            want_b[1:1 + n_out] += out[l, :n_out, n_in]
        assert torch.equal(wides[l], want_w), l
        assert torch.equal(biases[l], want_b), l


@pytest.mark.gpu
def test_weight_grads_skip_frozen_layers_and_frozen_biases():
    """The Python `keep` path: a frozen weight drops its layer (and its bias) from the launch, a frozen bias alone gets a null
    destination; the layers that remain get exactly their float64 gradient."""
    from adaptigraph_amd import train_ops
    rows, spec = 1037, "C"
    dzs, prevs, n_ins = dw_tables(rows, spec, make_gen(2, DEV), DEV)
    ref = dw_reference(dzs, prevs, rows, spec)
    Ws = [torch.zeros(s[0], s[1], device=DEV, requires_grad=(l != 1)) for l, s in enumerate(SPECS[spec])]
    bs = [torch.zeros(s[0], device=DEV, requires_grad=(l == 0)) for l, s in enumerate(SPECS[spec])]
    assert train_ops.weight_grads(dzs, prevs, n_ins, rows, list(zip(Ws, bs))) is None
    assert Ws[1].grad is None and bs[1].grad is None and bs[2].grad is None
    assert torch.equal(Ws[0].grad.double(), ref[0][0]) and torch.equal(bs[0].grad.double(), ref[0][1])
    assert torch.equal(Ws[2].grad.double(), ref[2][0])
    for w in Ws:
        w.requires_grad_(False)
    first = [None if w.grad is None else w.grad.clone() for w in Ws]
    assert train_ops.weight_grads(dzs, prevs, n_ins, rows, list(zip(Ws, bs))) is None          # every layer frozen: nothing runs
    assert all((a is None and w.grad is None) or torch.equal(a, w.grad) for a, w in zip(first, Ws))


def shared_linear_graph(lin, x, W, b, V, probe):
    """One weight applied ten times and a second one three times, interleaved; signed-permutation weights keep integers small."""
    h = x
    for i in range(13):
        h = torch.relu(lin(h, V, None) if i in (2, 6, 11) else lin(h, W, b))
    return (h * probe).sum()


def shared_linear_inputs(dev):
    gen = make_gen(4, dev)
    rows, D = 300, 150
    perm = lambda: torch.eye(D, device=dev)[torch.randperm(D, generator=gen, device=dev)] * (ints(gen, (D, 1), 0, 1, dev) * 2 - 1)
    return ints(gen, (rows, D), -3, 3, dev), perm(), ints(gen, (D,), -1, 2, dev), perm(), ints(gen, (rows, D), -2, 2, dev)


def shared_linear_reference(x, W, b, V, probe):
    Wd, bd, Vd = (t.double().requires_grad_() for t in (W, b, V))
    acts = []

    def lin(h, w, bias):
        acts.append(h)
        return F.linear(h, w, bias)

    loss = shared_linear_graph(lin, x.double(), Wd, bd, Vd, probe.double())
    grads = torch.autograd.grad(loss, (Wd, bd, Vd))
    # every dW partial sum is bounded by rows * max|g| * max|h|, and the 10 (3) uses add up in the same destination
    bound = 10 * x.shape[0] * probe.abs().max().item() * max(a.abs().max().item() for a in acts)
    return grads, bound


def test_shared_destination_case_stays_inside_integer_bounds():
    grads, bound = shared_linear_reference(*shared_linear_inputs("cpu"))
    assert bound < EXACT_F32 and all(g.abs().max().item() > 0 for g in grads)


@pytest.mark.gpu
def test_direct_grads_of_a_weight_used_ten_times_equal_float64_autograd():
    """train_ops.linear under direct_grads(): ten uses of one weight and three of another queue 13 layers with two destinations;
    that takes the early flush at >= 8 queued, the final flush, and the rule that two layers of one launch never share a
    destination.  .grad equals float64 autograd of the same graph bit for bit, twice over (accumulation)."""
    from adaptigraph_amd import train_ops
    x, W, b, V, probe = shared_linear_inputs(DEV)
    (rW, rb, rV), bound = shared_linear_reference(x, W, b, V, probe)
    assert 2 * bound < EXACT_F32
    Wp, bp, Vp = (t.clone().requires_grad_() for t in (W, b, V))
    for k in (1, 2):
        with train_ops.direct_grads():
            shared_linear_graph(train_ops.linear, x, Wp, bp, Vp, probe).backward()
        assert not train_ops._PENDING and not train_ops._PENDING_ARMED[0]
        assert torch.equal(Wp.grad.double(), k * rW) and torch.equal(bp.grad.double(), k * rb) and torch.equal(Vp.grad.double(), k * rV)
    got = torch.autograd.grad(shared_linear_graph(train_ops.linear, x, Wp, bp, Vp, probe), (Wp, bp, Vp))      # and through autograd's own sums
    assert all(torch.equal(a.double(), r) for a, r in zip(got, (rW, rb, rV)))


# =====================================================================================================================
# 2. Fused chains: chain_forward_kernel / chain_backward_kernel
# =====================================================================================================================
CHAIN_LAYERS = {"edge": 4, "node": 3, "decoder": 3}
CHAIN_D_IN = {"edge": 17, "node": 6, "decoder": 150}


def sparse_int_weight(gen, n_out, n_in, nnz, dev):
    """`nnz` entries of {-2, -1, 1, 2} per row, on shifted diagonals: every column holds about nnz * n_out / n_in of them, so
    magnitudes grow by a bounded factor per layer in both directions."""
    W = torch.zeros(n_out, n_in, device=dev)
    o = torch.arange(n_out, device=dev)
    vals = torch.tensor([-2.0, -1.0, 1.0, 2.0], device=dev)
    for c in torch.randperm(n_in, generator=gen, device=dev)[:min(nnz, n_in)].tolist():
        W[o, (o + c) % n_in] = vals[torch.randint(0, 4, (n_out,), generator=gen, device=dev)]
    return W


def chain_case(kind, d_in, rows, seed, dev, real=False, x_max=2, dy_max=1):
    """x, weights, biases and the probe (dy) of one chain case.  The edge chain's last weight is the first 150 columns of a
    (150, 450) parameter, as in the model."""
    gen = make_gen(seed, dev)
    n = CHAIN_LAYERS[kind]
    dims = [d_in] + [150] * (n - 1) + [3 if kind == "decoder" else 150]
    if real:
        Ws = [floats(gen, (dims[l + 1], dims[l]), dev) / np.sqrt(dims[l]) for l in range(n)]
        bs = [floats(gen, (dims[l + 1],), dev) * 0.1 for l in range(n)]
        x, probe = floats(gen, (rows, d_in), dev), floats(gen, (rows, dims[-1]), dev)
    else:
        Ws = [sparse_int_weight(gen, dims[l + 1], dims[l], 40 if dims[l + 1] == 3 else 3, dev) for l in range(n)]
        bs = [ints(gen, (dims[l + 1],), -2, 2, dev) for l in range(n)]
        x, probe = ints(gen, (rows, d_in), -x_max, x_max, dev), ints(gen, (rows, dims[-1]), -dy_max, dy_max, dev)
    if kind == "edge":
        Ws[-1] = torch.cat([Ws[-1], floats(gen, (150, 300), dev) if real else ints(gen, (150, 300), -2, 2, dev)], 1)
    return x, Ws, bs, probe


def chain_reference(kind, x, Ws, bs, probe):
    """The same stack in float64 torch (F.linear / relu / autograd): output, [dx] + weight + bias gradients, and the largest
    magnitudes the exactness argument depends on."""
    n = len(Ws)
    relu = [True] * (n - 1) + [kind == "node"]
    xd = x.double().requires_grad_()
    Wd, bd = [w.double().requires_grad_() for w in Ws], [b.double().requires_grad_() for b in bs]
    h, acts, pres = xd, [xd], []
    for l in range(n):
        pre = F.linear(h, Wd[l][:, :150] if (kind == "edge" and l == n - 1) else Wd[l], bd[l])
        h = torch.relu(pre) if relu[l] else pre
        pres.append(pre); acts.append(h)
    grads = torch.autograd.grad((h * probe.double()).sum(), [xd] + Wd + bd + pres)
    dzs = grads[1 + 2 * n:]
    ones = torch.ones((x.shape[0], 1), dtype=torch.float64, device=x.device)
    mags = {"act": max(a.abs().max().item() for a in acts), "pre": max(p.abs().max().item() for p in pres),
            "dz": max(z.abs().max().item() for z in dzs), "dx": grads[0].abs().max().item(),
            "dw": max((dzs[l].abs().T @ torch.cat([acts[l].detach().abs(), ones], 1)).max().item() for l in range(n))}
    return h.detach(), grads[:1 + 2 * n], mags


def rows_near_a_relu_kink(kind, x, Ws, bs, margin):
    """Rows of the float64 forward with a ReLU input closer than `margin` to 0."""
    n = len(Ws)
    h, near = x.double(), torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    for l in range(n):
        h = F.linear(h, (Ws[l][:, :150] if (kind == "edge" and l == n - 1) else Ws[l]).double(), bs[l].double())
        if l < n - 1 or kind == "node":
            near |= (h.abs() < margin).any(1)
            h = torch.relu(h)
    return near


def assert_chain_exactness_bounds(mags):
    """Activations and pre-activation gradients enter a split-bf16 layer: integers below 2^16.  Everything else is an fp32 sum
    of integers: below 2^24, |dz|^T |y| included (it bounds every partial sum of the weight gradient in any order)."""
    assert mags["act"] < EXACT_SPLIT and mags["dz"] < EXACT_SPLIT, mags
    assert mags["pre"] < EXACT_F32 and mags["dx"] < EXACT_F32 and mags["dw"] < EXACT_F32, mags


def run_chain(kind, x, Ws, bs, probe):
    from adaptigraph_amd import train_ops
    n = len(Ws)
    xs, Wp, bp = x.clone().requires_grad_(), [w.clone().requires_grad_() for w in Ws], [b.clone().requires_grad_() for b in bs]
    layers = [((Wp[l][:, :150] if (kind == "edge" and l == n - 1) else Wp[l]), bp[l]) for l in range(n)]
    y = train_ops.fused_chain(kind, xs, layers)
    return y.detach(), torch.autograd.grad((y * probe).sum(), [xs] + Wp + bp)


def multi_tile_rows(cus):
    # ag_train_chain caps the grid at AG_MLP_WG_PER_CU x CUs workgroups, AG_MLP_WG_PER_CU = 512 / AG_MLP_THREADS = 2, and a tile
    # is 128 rows: 2 tiles x 128 rows x 2 workgroups per CU x CUs rows give every workgroup two tiles, 77 more rows a third
    # (partial) tile to workgroup 0 — each workgroup walks several tiles and re-streams the weight ring, on any part.
    return 2 * 128 * 2 * cus + 77


SMALL_CHAIN_CASES = [(k, CHAIN_D_IN[k], r) for k in ("edge", "node", "decoder") for r in (1, 127, 128, 129)] + \
                    [("node", d, 129) for d in (1, 2, 3, 4, 5, 7)]


def test_split_bf16_is_exact_for_the_integers_the_exact_cases_use():
    """hi = bf16(v), lo = bf16(v - hi), round to nearest even: hi + lo == v for every integer |v| <= 65 536, and the weights
    and biases of the exact cases (-2..2) have a zero lo half, so lo * lo — the product the kernels drop — is zero."""
    v = torch.arange(-65536, 65537, dtype=torch.float32)
    hi = v.bfloat16().float()
    lo = (v - hi).bfloat16().float()
    assert torch.equal(hi + lo, v)
    w = torch.arange(-2, 3, dtype=torch.float32)
    assert torch.equal(w.bfloat16().float(), w)
    bad = torch.tensor([131329.0])
    h2 = bad.bfloat16().float()
    assert not torch.equal(h2 + (bad - h2).bfloat16().float(), bad)


@pytest.mark.parametrize("kind,d_in,rows", SMALL_CHAIN_CASES + [("edge", 17, multi_tile_rows(256))])
def test_chain_exact_cases_stay_inside_integer_bounds(kind, d_in, rows):
    """The builders of the exact chain cases, on the CPU: the float64 reference stays inside the bounds that make fp32 and
    split-bf16 arithmetic exact (the GPU tests assert the same on their own data)."""
    x, Ws, bs, probe = chain_case(kind, d_in, rows, 7, "cpu")
    y, grads, mags = chain_reference(kind, x, Ws, bs, probe)
    assert_chain_exactness_bounds(mags)
    assert all(torch.equal(g, g.round()) for g in grads) and y.abs().max().item() > 0
    if rows > 1:
        assert all(g.abs().max().item() > 0 for g in grads)          # no gradient path of the case is dead


def assert_chain_equal(got_y, got_grads, ref_y, ref_grads):
    assert got_y.shape == ref_y.shape and torch.equal(got_y.double(), ref_y), (got_y.double() - ref_y).abs().max().item()
    for i, (a, b) in enumerate(zip(got_grads, ref_grads)):
        assert a.shape == b.shape and torch.equal(a.double(), b), (i, (a.double() - b).abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("kind,d_in,rows", SMALL_CHAIN_CASES)
def test_chain_small_shapes_exact_vs_float64(kind, d_in, rows, precision, monkeypatch):
    """Output, dx and every weight / bias gradient, bit for bit, at rows around one tile and node d_in 1..7, both arithmetics."""
    from adaptigraph_amd import train_ops
    monkeypatch.setattr(train_ops, "CHAIN_PRECISION", precision)
    x, Ws, bs, probe = chain_case(kind, d_in, rows, 7, DEV)
    ref_y, ref_grads, mags = chain_reference(kind, x, Ws, bs, probe)
    assert_chain_exactness_bounds(mags)
    assert_chain_equal(*run_chain(kind, x, Ws, bs, probe), ref_y, ref_grads)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("kind", ["edge", "node", "decoder"])
def test_chain_many_tiles_per_workgroup_exact_vs_float64(kind, precision, monkeypatch):
    """More row tiles than the grid has workgroups: every workgroup walks at least two tiles, the last tile is partial
    (the shape bench_train.py times).  Bit for bit against float64; two runs give the same bits."""
    from adaptigraph_amd import train_ops
    monkeypatch.setattr(train_ops, "CHAIN_PRECISION", precision)
    rows = multi_tile_rows(torch.cuda.get_device_properties(DEV).multi_processor_count)
    x, Ws, bs, probe = chain_case(kind, CHAIN_D_IN[kind], rows, 7, DEV)
    ref_y, ref_grads, mags = chain_reference(kind, x, Ws, bs, probe)
    assert_chain_exactness_bounds(mags)
    y, grads = run_chain(kind, x, Ws, bs, probe)
    assert_chain_equal(y, grads, ref_y, ref_grads)
    y2, grads2 = run_chain(kind, x, Ws, bs, probe)
    assert torch.equal(y, y2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("kind", ["edge", "decoder"])
def test_chain_many_tiles_per_workgroup_random_floats(kind, precision, monkeypatch):
    """The same shape with random floats, under the gates of test_fused_dense_chain_forward_and_backward_vs_torch.
    With 6 x 10^7 ReLU inputs some lie within rounding of 0, where an fp32 and a float64 forward pick different masks and the
    gradient, which is discontinuous there, has no reference value (first run of this test: dx off by 7e-2 of its maximum in
    both arithmetics, while the integer case of the same shape was bit-exact).  Rows whose float64 pre-activation comes within
    1e-3 of a kink (ten times the forward gate) therefore get a zero upstream gradient; the rest is gated as usual."""
    from adaptigraph_amd import train_ops
    monkeypatch.setattr(train_ops, "CHAIN_PRECISION", precision)
    tol = 2e-5 if precision == 0 else 1e-4
    rows = multi_tile_rows(torch.cuda.get_device_properties(DEV).multi_processor_count)
    x, Ws, bs, probe = chain_case(kind, CHAIN_D_IN[kind], rows, 9, DEV, real=True)
    near = rows_near_a_relu_kink(kind, x, Ws, bs, 1e-3)
    assert near.float().mean().item() < 0.6 and not near[-77:].all() and not near[:128].all()
    probe[near] = 0.0
    ref_y, ref_grads, _ = chain_reference(kind, x, Ws, bs, probe)
    y, grads = run_chain(kind, x, Ws, bs, probe)
    err = (y.double() - ref_y).abs().max().item() / max(1.0, ref_y.abs().max().item())
    errs = [(a.double() - b).abs().max().item() / max(1e-3, b.abs().max().item()) for a, b in zip(grads, ref_grads)]
    print(f"chain float case {kind} precision={precision} rows={rows}: output {err:.2e}, gradients {max(errs):.2e} (gate {tol:.0e})")
    assert y.shape == ref_y.shape and err <= tol
    assert all(a.shape == b.shape for a, b in zip(grads, ref_grads)) and max(errs) <= tol, errs


@pytest.mark.gpu
@pytest.mark.parametrize("precision", [1, 0])
@pytest.mark.parametrize("kind", ["edge", "node", "decoder"])
def test_chain_with_no_rows(kind, precision, monkeypatch):
    """rows = 0: the output is (0, n_out), every parameter gradient is exactly zero (the tables are torch.empty: nothing of
    them may leak into a gradient), dx is (0, d_in)."""
    from adaptigraph_amd import train_ops
    monkeypatch.setattr(train_ops, "CHAIN_PRECISION", precision)
    x, Ws, bs, probe = chain_case(kind, CHAIN_D_IN[kind], 0, 7, DEV)
    poison = [torch.full((128, FP), float("nan"), device=DEV) for _ in range(12)]      # what torch.empty hands out next
    del poison
    y, grads = run_chain(kind, x, Ws, bs, probe)
    assert y.shape == (0, 3 if kind == "decoder" else 150) and grads[0].shape == x.shape
    for g, p in zip(grads[1:], Ws + bs):
        assert g.shape == p.shape and torch.equal(g, torch.zeros_like(p))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["edge", "node", "decoder"])
def test_chain_backward_ignores_stale_rows_of_the_shared_dy_buffer(kind):
    """_zero_padded keeps one dy buffer per padded size: after a call with more rows, a call with fewer rows at the same padded
    size finds stale non-zero rows past its own.  They must not reach any result: same bits as after dropping the buffers."""
    from adaptigraph_amd import train_ops
    big = chain_case(kind, CHAIN_D_IN[kind], 250, 7, DEV, dy_max=2)
    small = chain_case(kind, CHAIN_D_IN[kind], 131, 8, DEV)
    train_ops._ZEROS.clear()
    run_chain(kind, *big)
    dy = train_ops._ZEROS[("dy_" + kind, 256, torch.device(DEV).index)]
    assert dy[131:250].abs().max().item() > 0                  # the stale rows are really there
    y1, g1 = run_chain(kind, *small)
    train_ops._ZEROS.clear()
    y2, g2 = run_chain(kind, *small)
    assert torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    ref_y, ref_grads, mags = chain_reference(kind, *small)
    assert_chain_exactness_bounds(mags)
    assert_chain_equal(y1, g1, ref_y, ref_grads)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["edge", "node", "decoder"])
def test_pack_cache_serves_alternating_parameter_sets(kind):
    """The pack cache has one slot per kind: parameter sets A, B, A of one kind give A the same bits both times, B its own."""
    from adaptigraph_amd import train_ops
    x, Wa, ba, probe = chain_case(kind, CHAIN_D_IN[kind], 300, 7, DEV)
    _, Wb, bb, _ = chain_case(kind, CHAIN_D_IN[kind], 300, 8, DEV)
    n = len(Wa)

    def run(Ws, bs):      # the SAME parameter objects every time: only the cache slot changes hands
        layers = [((Ws[l][:, :150] if (kind == "edge" and l == n - 1) else Ws[l]), bs[l]) for l in range(n)]
        y = train_ops.fused_chain(kind, x, layers)
        return [y.detach()] + list(torch.autograd.grad((y * probe).sum(), Ws + bs))

    A = [w.requires_grad_() for w in Wa], [b.requires_grad_() for b in ba]
    B = [w.requires_grad_() for w in Wb], [b.requires_grad_() for b in bb]
    a1, b1, a2, b2 = run(*A), run(*B), run(*A), run(*B)
    assert all(torch.equal(p, q) for p, q in zip(a1, a2)) and all(torch.equal(p, q) for p, q in zip(b1, b2))
    assert not torch.equal(a1[0], b1[0])
    ref_y, ref_grads, mags = chain_reference(kind, x, [w.detach() for w in Wb], [b.detach() for b in bb], probe)
    assert_chain_exactness_bounds(mags)
    assert torch.equal(b2[0].double(), ref_y) and all(torch.equal(p.double(), q) for p, q in zip(b2[1:], ref_grads[1:]))


# =====================================================================================================================
# 3. Graph operators
# =====================================================================================================================
def graph_lists(name):
    """(N, recv, send) of one hand-built graph, receiver-sorted (the order ag_build_edges produces)."""
    if name == "degrees":        # degrees 0, 1, 64 and 1000 in one graph; nodes 1004.. neither send nor receive
        N, edges = 1100, [(1, 7)] + [(2, 10 + i) for i in range(64)] + [(3, 4 + i) for i in range(1000)] + [(5, 3), (9, 9)]
    elif name == "hub":          # node 0 receives from everyone and is everyone's sender
        N = 300
        edges = [(0, i) for i in range(1, N)] + [(i, 0) for i in range(1, N)]
    elif name == "dups_loops":   # duplicate edges, self loops, a duplicated self loop, trailing isolated nodes
        N, edges = 20, [(0, 0), (1, 2), (1, 2), (1, 2), (2, 1), (2, 2), (2, 2), (4, 1), (4, 4), (7, 0), (7, 0), (7, 7)]
    else:
        assert name == "empty"
        N, edges = 5, []
    edges = sorted(edges, key=lambda e: e[0])                    # stable: keeps the order within a receiver
    recv = np.array([e[0] for e in edges], np.int32).reshape(1, -1)
    send = np.array([e[1] for e in edges], np.int32).reshape(1, -1)
    return N, recv, send


GRAPHS = ["degrees", "hub", "dups_loops", "empty"]
WIDTHS = [1, 3, 15, 150, 160, 257]


def test_graph_case_table_covers_the_degrees_and_edges_asked_for():
    N, recv, send = graph_lists("degrees")
    deg = np.bincount(recv[0], minlength=N)
    assert {0, 1, 64, 1000} <= set(deg.tolist()) and deg[1004:].sum() == 0 and np.bincount(send[0], minlength=N)[1004:].sum() == 0
    N, recv, send = graph_lists("hub")
    assert np.bincount(recv[0], minlength=N)[0] == N - 1 and np.bincount(send[0], minlength=N)[0] == N - 1
    N, recv, send = graph_lists("dups_loops")
    pairs = list(zip(recv[0].tolist(), send[0].tolist()))
    assert len(set(pairs)) < len(pairs) and any(r == s for r, s in pairs) and max(max(p) for p in pairs) < N - 1
    assert graph_lists("empty")[1].shape == (1, 0)
    for g in GRAPHS:
        assert np.all(np.diff(graph_lists(g)[1][0]) >= 0)


def edge_views(name):
    from adaptigraph_amd import train_ops
    from test_gpu_parity import csr_from_lists
    N, recv, send = graph_lists(name)
    v = train_ops.EdgeViews(csr_from_lists([recv.shape[1]], recv, send, N))
    assert v.E == recv.shape[1] and v.M == N
    return v, torch.from_numpy(recv[0]).long().to(DEV), torch.from_numpy(send[0]).long().to(DEV)


def grads_or_zeros(out, inputs):
    got = torch.autograd.grad(out, inputs, allow_unused=True)      # an operand that an empty graph never touches has a zero gradient
    return [torch.zeros_like(t) if g is None else g for g, t in zip(got, inputs)]


def message_case(v, recv, send, D, real):
    from adaptigraph_amd import train_ops
    gen = make_gen(D, DEV)
    draw = (lambda shape, m: floats(gen, shape, DEV)) if real else (lambda shape, m: ints(gen, shape, -m, m, DEV))
    x, e, hr = (draw(s, 3).requires_grad_() for s in ((v.M, D), (v.E, D), (v.M, D)))
    w1, w2, w3 = draw((v.E, D), 2), draw((v.M, D), 2), draw((v.E, D), 2)
    gr, gs, agg = train_ops.gather_receivers(x, v), train_ops.gather_senders(x, v), train_ops.message_sum(e, hr, x, v)
    got = grads_or_zeros((gr * w1).sum() + (gs * w3).sum() + (agg * w2).sum(), (x, e, hr))
    xd, ed, hrd = (t.detach().double().requires_grad_() for t in (x, e, hr))
    rr, rs = xd[recv], xd[send]
    ragg = torch.zeros(v.M, D, dtype=torch.float64, device=DEV).index_add(0, recv, torch.relu(ed + hrd[recv] + xd[send]))
    ref = torch.autograd.grad((rr * w1.double()).sum() + (rs * w3.double()).sum() + (ragg * w2.double()).sum(), (xd, ed, hrd))
    return (gr, gs, agg), got, (rr.detach(), rs.detach(), ragg.detach()), ref


@pytest.mark.gpu
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("graph", GRAPHS)
def test_message_and_gather_ops_exact_vs_float64(graph, D):
    """gather_receivers / gather_senders / message_sum forward and backward (gather_rows, segment_sum, message_fwd / bwd) on
    hand-built graphs, integer data: bit for bit against float64 indexing / index_add / autograd, relu'(0) = 0 included."""
    v, recv, send = edge_views(graph)
    fwd, got, rfwd, ref = message_case(v, recv, send, D, real=False)
    assert max(t.abs().max().item() if t.numel() else 0 for t in list(rfwd) + list(ref)) < EXACT_F32
    for a, b in zip(list(fwd) + list(got), list(rfwd) + list(ref)):
        assert a.shape == b.shape and torch.equal(a.double(), b), (a.double() - b).abs().max().item()
    if v.E > 100 and D >= 15:
        assert (ref[1] == 0).any() and (ref[1] != 0).any()          # some messages are masked (pre <= 0), some pass


@pytest.mark.gpu
@pytest.mark.parametrize("graph,D", [("degrees", 150), ("hub", 15)])
def test_message_and_gather_ops_random_floats(graph, D):
    """The same operators on random floats, under the gate of test_graph_ops_forward_and_adjoint_vs_torch (1e-5 relative)."""
    v, recv, send = edge_views(graph)
    fwd, got, rfwd, ref = message_case(v, recv, send, D, real=True)
    assert torch.equal(fwd[0].double(), rfwd[0]) and torch.equal(fwd[1].double(), rfwd[1])
    for a, b in zip([fwd[2]] + list(got), [rfwd[2]] + list(ref)):
        err = (a.double() - b).abs().max().item() / b.abs().max().item()
        print(f"graph float case {graph} D={D}: {err:.2e} (gate 1e-5)")
        assert err <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("A,G,S", [(2, 2, 12), (0, 2, 3), (2, 0, 12), (1, 1, 1), (3, 5, 249)])
@pytest.mark.parametrize("graph", GRAPHS)
def test_edge_inputs_exact_vs_float64(graph, A, G, S):
    """edge_inputs forward and backward, integer data (group columns 0 / 1, so |g_r - g_s| sits on its kink for about half the
    edges and on every self loop): bit for bit against the float64 composition; A = 0 and G = 0 included."""
    from adaptigraph_amd import train_ops
    v, recv, send = edge_views(graph)
    gen = make_gen(A + 10 * G, DEV)
    tab = ints(gen, (v.M, A + G + S), -3, 3, DEV)
    tab[:, A:A + G] = ints(gen, (v.M, G), 0, 1, DEV)
    tab.requires_grad_()
    probe = ints(gen, (v.E, 2 * A + 1 + S), -2, 2, DEV)
    out = train_ops.edge_inputs(tab, v, A, G)
    (got,) = torch.autograd.grad((out * probe).sum(), tab)
    td = tab.detach().double().requires_grad_()
    ref_out = torch.cat([td[recv, :A], td[send, :A], (td[recv, A:A + G] - td[send, A:A + G]).abs().sum(1, keepdim=True),
                         td[recv, A + G:] - td[send, A + G:]], 1)
    (ref,) = torch.autograd.grad((ref_out * probe.double()).sum(), td)
    assert ref.abs().max().item() < EXACT_F32
    assert out.shape == ref_out.shape and torch.equal(out.double(), ref_out.detach())
    assert got.shape == ref.shape and torch.equal(got.double(), ref), (got.double() - ref).abs().max().item()
    (again,) = torch.autograd.grad((train_ops.edge_inputs(tab, v, A, G) * probe).sum(), tab)
    assert torch.equal(got, again)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [4, 8, 4 * (256 * 1000 + 3)])
def test_add3_relu_and_its_mask_exact(count):
    """relu(a + b + c) and g * [y > 0] with integer data: about one sum in seven is exactly 0, where the gradient is 0."""
    from adaptigraph_amd import train_ops
    gen = make_gen(count, DEV)
    a, b, c = (ints(gen, (count,), -3, 3, DEV).requires_grad_() for _ in range(3))
    with torch.no_grad():
        a[0], b[0], c[0] = 2.0, -3.0, 1.0                          # a sum of exactly zero, whatever the draw
        a[count - 1], b[count - 1], c[count - 1] = 1.0, 1.0, 1.0
    w = ints(gen, (count,), -2, 2, DEV)
    y = train_ops.add3_relu(a, b, c)
    got = torch.autograd.grad((y * w).sum(), (a, b, c))
    ad, bd, cd = (t.detach().double().requires_grad_() for t in (a, b, c))
    ry = torch.relu(ad + bd + cd)
    ref = torch.autograd.grad((ry * w.double()).sum(), (ad, bd, cd))
    assert torch.equal(y.double(), ry.detach()) and y[0].item() == 0 and y[count - 1].item() == 3
    assert all(torch.equal(g.double(), r) for g, r in zip(got, ref)) and got[0][0].item() == 0


def model_batch(g, B):
    from test_train import KEYS, tg
    from test_gpu_parity import csr_from_lists
    data = {k: tg(g["b_" + k][:B]) for k in KEYS}
    data.update(Rr=csr_from_lists(g["n_rel"][:B], g["recv"][:B], g["send"][:B], g["b_attrs"].shape[1]), Rs=None)
    return data


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 2])
def test_fused_model_equals_plain_torch_model_at_odd_and_even_node_counts(B, weights):
    """TrainableDynamicsPredictor with fused_dense = True against fused_dense = False (plain torch GEMMs, torch graph ops for the
    edge inputs): the 3-step loss and all 22 parameter gradients, under the gradient gate of
    test_unrolled_loss_and_gradients_match_reference (2e-4 relative).  B = 3 gives B * N = 123 nodes: (B N nf) % 4 != 0, the
    branch of forward without linear2 / add3_relu; B = 2 (82 nodes) is the control through them."""
    from adaptigraph_amd.train_model import unrolled_loss
    from test_train import trainable
    g = load_golden("train_rope")
    N = g["b_attrs"].shape[1]
    assert (B * N) % 2 == B % 2 and N % 2 == 1
    res = {}
    for fused in (True, False):
        model = trainable(weights).train()
        model.fused_dense = fused
        assert ((B * N * model.nf_effect) % 4 != 0) == (B == 3)
        loss = unrolled_loss(model, model_batch(g, B), 3)
        loss.backward()
        res[fused] = (loss.item(), {n: p.grad.clone() for n, p in model.named_parameters()})
    assert len(res[True][1]) == 22
    assert abs(res[True][0] - res[False][0]) <= 2e-4 * abs(res[False][0])
    for name, ref in res[False][1].items():
        err = (res[True][1][name] - ref).abs().max().item()
        assert err <= 2e-4 * ref.abs().max().item() + 1e-9, (name, err, ref.abs().max().item())
