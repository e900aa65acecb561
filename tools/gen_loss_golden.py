#!/usr/bin/env python
"""Generate tests/golden/gnn_loss_cases.npz: inputs and expected results of the matching losses (adaptigraph_amd.losses.emd / hausdorff,
adaptigraph_amd.gnn_loss), on the build machine only (needs scipy and the imported reference, as tools/gen_golden.py does).

    python tools/gen_loss_golden.py          # gnn_loss_cases.npz
    python tools/gen_loss_golden.py large    # gnn_loss_large.npz: the same recording at 300 ... 1024 points (scipy only, its own seed)

Per case `<name>` the file holds
    <name>_x (B,N,3), <name>_y (By,M,3) fp32, and for the masked cases <name>_xm (B,N), <name>_ym (By,M) u8;
    <name>_col (B,N) int32: scipy.optimize.linear_sum_assignment on the cost matrix of the valid points,
        c[n,m] = sqrt((dx dx + dy dy) + dz dz) in numpy fp32, widened to fp64; -1 for a masked or unmatched point;
    <name>_total (B) fp64: the sum of the matched costs, accumulated in ascending n (NaN for an empty side);
    <name>_colb / <name>_totalb: the same with y[0] as the one cloud of every sample (the broadcast form), where recorded;
    <name>_ref (3) fp32: ChamferLoss, EarthMoverLoss, HausdorffLoss of the reference's dynamics/gnn/loss.py on (x, y), for unmasked cases
        with one y per sample;
    <name>_unique: 1 when the optimum is unique as far as three scipy solves can tell (on C, on C.T and on a row-permuted C: all three return
        the same pairs); the generator refuses to write a case it expects to be unique and is not.
`cases` lists the names.  gnn_loss_large.npz holds the keys above (no `_ref`) for the cases of `LARGE_SHAPES`, `masked1024` and the two long chains:
every register slot of the 8 and 16 columns-per-lane kernels, valid counts far below and across a size class.  No test imports scipy or the reference: the small cases are re-proved by brute force in tests/test_gnn_loss_cpu.py.
"""
import os
import sys

import numpy as np
import scipy.optimize
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from ref_import import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gnn_loss_cases.npz")
OUT_LARGE = os.path.join(ROOT, "tests", "golden", "gnn_loss_large.npz")
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (63, 64), (64, 65), (65, 64), (100, 100), (129, 257), (257, 129)]
LARGE_SHAPES = [(512, 512), (513, 300), (300, 513), (640, 1024), (1000, 1000), (1024, 1024)]
MASKED1024_COUNTS = [(700, 900), (0, 500), (3, 1024), (1024, 1), (513, 512)]
LARGE_CHAINS = [(1024, 1024), (513, 1024)]


def cost_matrix(x, y):
    """(N,3), (M,3) fp32 -> (N,M) fp32, products rounded separately."""
    d = x[:, None, :].astype(np.float32) - y[None, :, :].astype(np.float32)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)


def gauss(rng, shape, scale=np.float32(1.0)):
    """Normal coordinates on a grid of 2^-12: exact in fp32 with twelve zero mantissa bits, which keeps the compressed fixture small."""
    return (np.round(rng.standard_normal(shape) * float(scale) * 4096.0) / 4096.0).astype(np.float32)


def pairs_of(C):
    r, c = scipy.optimize.linear_sum_assignment(C)
    return sorted(zip(r.tolist(), c.tolist()))


def solve(C, rng, need_unique):
    """-> (pairs, unique) on an fp64 cost matrix."""
    base = pairs_of(C)
    via_t = sorted((r, c) for c, r in pairs_of(C.T.copy()))
    perm = rng.permutation(C.shape[0])
    via_p = sorted((int(perm[r]), c) for r, c in pairs_of(C[perm]))
    unique = base == via_t == via_p
    if need_unique and not unique:
        raise SystemExit("a case meant to have a unique optimum has several: change its seed")
    return base, unique


def assign(x, y, xm, ym, rng, need_unique=True):
    """One sample -> (col (N) int32, total fp64, unique)."""
    vx = np.arange(x.shape[0]) if xm is None else np.flatnonzero(xm)
    vy = np.arange(y.shape[0]) if ym is None else np.flatnonzero(ym)
    col = np.full(x.shape[0], -1, np.int32)
    if len(vx) == 0 or len(vy) == 0:
        return col, float("nan"), True
    C = cost_matrix(x[vx], y[vy]).astype(np.float64)
    pairs, unique = solve(C, rng, need_unique)
    total = 0.0
    for r, c in pairs:                      # ascending n
        col[vx[r]] = vy[c]
        total += float(C[r, c])
    return col, total, unique


def record(out, name, x, y, rng, xm=None, ym=None, need_unique=True, broadcast=False, ref=None):
    B = x.shape[0]
    cols, totals, uniq = [], [], True
    for b in range(B):
        yb = y[b if y.shape[0] == B else 0]
        ymb = None if ym is None else ym[b if ym.shape[0] == B else 0]
        c, t, u = assign(x[b], yb, None if xm is None else xm[b], ymb, rng, need_unique)
        cols.append(c); totals.append(t); uniq = uniq and u
    out[name + "_x"], out[name + "_y"] = x.astype(np.float32), y.astype(np.float32)
    if xm is not None:
        out[name + "_xm"], out[name + "_ym"] = xm.astype(np.uint8), ym.astype(np.uint8)
    out[name + "_col"], out[name + "_total"] = np.stack(cols), np.array(totals, np.float64)
    out[name + "_unique"] = np.array(int(uniq), np.int32)
    if broadcast:
        cb = [assign(x[b], y[0], None if xm is None else xm[b], None if ym is None else ym[0], rng, need_unique) for b in range(B)]
        out[name + "_colb"], out[name + "_totalb"] = np.stack([c[0] for c in cb]), np.array([c[1] for c in cb], np.float64)
    if ref is not None:
        tx, ty = torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.float32))
        out[name + "_ref"] = np.array([float(m()(tx, ty)) for m in (ref.ChamferLoss, ref.EarthMoverLoss, ref.HausdorffLoss)], np.float32)
    out.setdefault("cases", []).append(name)


def chain(N, M):
    x, y = np.zeros((1, N, 3), np.float32), np.zeros((1, M, 3), np.float32)
    x[0, :, 0] = np.arange(N, dtype=np.float32)[::-1]
    y[0, :, 0] = np.arange(M, dtype=np.float32) + np.float32(0.4)
    return x, y


def main_large():
    """The size classes the small file does not reach: 8 columns per lane with every slot occupied, 16 columns per lane from its first size to
    the limit.  Its own rng stream, so gnn_loss_cases.npz does not depend on it."""
    out = {}
    rng = np.random.default_rng(20250611)
    for N, M in LARGE_SHAPES:                                             # Gaussian clouds, two different samples each
        x, y = gauss(rng, (2, N, 3)), gauss(rng, (2, M, 3))
        record(out, f"s{N}x{M}", x, y, rng, broadcast=True)
    # 1024 slots a side, the valid points scattered: few valid in many slots, the rows on either side, counts across the 512 boundary
    N = M = 1024
    B = len(MASKED1024_COUNTS)
    x, y = gauss(rng, (B, N, 3)), gauss(rng, (B, M, 3))
    xm, ym = np.zeros((B, N), np.uint8), np.zeros((B, M), np.uint8)
    for b, (nx, my) in enumerate(MASKED1024_COUNTS):
        xm[b, rng.permutation(N)[:nx]] = 1
        ym[b, rng.permutation(M)[:my]] = 1
    record(out, "masked1024", x, y, rng, xm, ym, broadcast=True)
    for N, M in LARGE_CHAINS:                                             # augmenting paths through every register slot
        record(out, f"chain{N}x{M}", *chain(N, M), rng)
    for name in out["cases"]:
        assert int(out[name + "_unique"]) == 1, name
    out["cases"] = np.array(out["cases"])
    np.savez_compressed(OUT_LARGE, **out)
    print(f"{OUT_LARGE}: {len(out['cases'])} cases, {os.path.getsize(OUT_LARGE) / 1024:.1f} KiB")


def main():
    import_reference()
    from dynamics.gnn import loss as ref
    out = {}
    rng = np.random.default_rng(20240607)
    for N, M in SHAPES:                                                   # Gaussian clouds, three different samples each
        x, y = gauss(rng, (3, N, 3)), gauss(rng, (3, M, 3))
        record(out, f"s{N}x{M}", x, y, rng, broadcast=True, ref=ref)
    # padded clouds: the valid counts differ per sample and per side; sample 1 has an empty side, sample 3 every point valid
    N, M = 70, 80
    x, y = gauss(rng, (4, N, 3)), gauss(rng, (4, M, 3))
    xm, ym = np.zeros((4, N), np.uint8), np.zeros((4, M), np.uint8)
    for b, (nx, my) in enumerate([(50, 66), (0, 40), (65, 31), (N, M)]):
        xm[b, rng.permutation(N)[:nx]] = 1
        ym[b, rng.permutation(M)[:my]] = 1
    record(out, "masked", x, y, rng, xm, ym, broadcast=True)
    # a small masked case the brute-force proof reaches (K <= 6)
    x, y = gauss(rng, (3, 9, 3)), gauss(rng, (3, 7, 3))
    xm, ym = np.zeros((3, 9), np.uint8), np.zeros((3, 7), np.uint8)
    for b, (nx, my) in enumerate([(4, 6), (6, 3), (5, 5)]):
        xm[b, rng.permutation(9)[:nx]] = 1
        ym[b, rng.permutation(7)[:my]] = 1
    record(out, "masked_small", x, y, rng, xm, ym)
    # the chain: x_n = (n, 0, 0), y_m = (m + 0.4, 0, 0), the rows in descending order (every augmentation walks the whole chain)
    for N, M in ((64, 64), (65, 130)):
        record(out, f"chain{N}x{M}", *chain(N, M), rng)
    # near-rigid: y = a permutation of x + 0.01 noise; the assignment recovers the permutation
    x = gauss(rng, (3, 100, 3))
    perm = np.stack([rng.permutation(100) for _ in range(3)])
    y = np.stack([x[b][perm[b]] for b in range(3)]) + gauss(rng, (3, 100, 3), np.float32(0.01))
    record(out, "rigid", x, y.astype(np.float32), rng)
    out["rigid_perm"] = perm.astype(np.int32)                              # y[b, m] ~ x[b, perm[b, m]]
    for b in range(3):
        assert np.array_equal(perm[b][out["rigid_col"][b]], np.arange(100)), "near-rigid: the optimum is not the permutation"
    # ties: two integer grids, many optimal assignments (only the total is the fixture)
    g = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(27, 3).astype(np.float32)
    x = np.stack([g, g[::-1], g[rng.permutation(27)]])
    y = np.stack([g + np.float32([1, 0, 0]), g + np.float32([1, 1, 0]), g[rng.permutation(27)] + np.float32([0, 2, 1])])
    record(out, "ties", x, y, rng, need_unique=False)
    # the module values: (100,100), B = 4
    x, y = gauss(rng, (4, 100, 3)), gauss(rng, (4, 100, 3))
    record(out, "modules", x, y, rng, ref=ref)
    out["cases"] = np.array(out["cases"])
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out['cases'])} cases, {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    if sys.argv[1:] == ["large"]:
        main_large()
    elif sys.argv[1:]:
        raise SystemExit("usage: gen_loss_golden.py [large]")
    else:
        main()
