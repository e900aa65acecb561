"""What the matching losses can show without a GPU: the fixture proves its own small cases by brute force, the loss-spec parser, and the three
new entry points in the header, the export map, the build and the binding table."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from adaptigraph_amd import _lib, gnn_loss
from test_abi import declared_prototypes, signature_mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ag_emd", "ag_emd_backward", "ag_hausdorff")


def cost_matrix(x, y):
    d = x[:, None, :].astype(np.float32) - y[None, :, :].astype(np.float32)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)


def brute_force(C):
    """All injections of the smaller side of an fp64 cost matrix into the larger -> (minimum total, the (n, m) pair sets that attain it)."""
    N, M = C.shape
    best, argbest = np.inf, []
    if N <= M:
        candidates = ([(n, p[n]) for n in range(N)] for p in itertools.permutations(range(M), N))
    else:
        candidates = (sorted((p[m], m) for m in range(M)) for p in itertools.permutations(range(N), M))
    for pairs in candidates:
        total = 0.0
        for n, m in pairs:                      # ascending n, as the fixture accumulates
            total += float(C[n, m])
        if total < best:
            best, argbest = total, [pairs]
        elif total == best:
            argbest.append(pairs)
    return best, argbest


def test_fixture_small_cases_are_optimal_by_brute_force():
    g = load_golden("gnn_loss_cases")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "gnn_loss_cases.npz")) < 256 * 1024
    proved = 0
    for name in [str(c) for c in g["cases"]]:
        x, y = g[name + "_x"], g[name + "_y"]
        xm, ym = (g[name + "_xm"], g[name + "_ym"]) if name + "_xm" in g else (None, None)
        forms = [(y, ym, g[name + "_col"], g[name + "_total"])]
        if name + "_colb" in g:
            forms.append((y[:1], None if ym is None else ym[:1], g[name + "_colb"], g[name + "_totalb"]))
        for yy, yym, col, total in forms:
            for b in range(x.shape[0]):
                by = b if yy.shape[0] == x.shape[0] else 0
                vx = np.arange(x.shape[1]) if xm is None else np.flatnonzero(xm[b])
                vy = np.arange(yy.shape[1]) if yym is None else np.flatnonzero(yym[by])
                K = min(len(vx), len(vy))
                if K == 0:
                    assert np.isnan(total[b]) and (col[b] == -1).all()
                    continue
                if K > 6 or max(len(vx), len(vy)) > 7:
                    continue
                best, pairs = brute_force(cost_matrix(x[b][vx], yy[by][vy]).astype(np.float64))
                recorded = sorted((int(np.searchsorted(vx, n)), int(np.searchsorted(vy, col[b, n]))) for n in vx if col[b, n] >= 0)
                assert len(recorded) == K and (col[b][np.setdiff1d(np.arange(x.shape[1]), vx)] == -1).all()
                assert total[b] == best, (name, b)
                assert len(pairs) == 1 and sorted(pairs[0]) == recorded, (name, b)
                proved += 1
    assert proved >= 4 * 3 * 2 + 3


LARGE_CASES = ["s512x512", "s513x300", "s300x513", "s640x1024", "s1000x1000", "s1024x1024", "masked1024", "chain1024x1024", "chain513x1024"]


def test_large_fixture_is_self_consistent():
    """tests/golden/gnn_loss_large.npz (too large for brute force): every recorded assignment is an injection of the valid smaller side into
    valid points of the other, its total is the ascending-n fp64 sum of the fp32 costs, and the optimum was unique for the generator."""
    g = load_golden("gnn_loss_large")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "gnn_loss_large.npz")) < 512 * 1024
    assert [str(c) for c in g["cases"]] == LARGE_CASES
    checked = 0
    for name in LARGE_CASES:
        x, y = g[name + "_x"], g[name + "_y"]
        assert x.dtype == np.float32 and y.dtype == np.float32 and int(g[name + "_unique"]) == 1
        if not name.startswith("chain"):                                  # Gaussian coordinates on the 2^-12 grid
            assert np.array_equal(x * 4096, np.round(x * 4096)) and np.array_equal(y * 4096, np.round(y * 4096))
        xm, ym = (g[name + "_xm"], g[name + "_ym"]) if name + "_xm" in g else (None, None)
        forms = [(y, ym, g[name + "_col"], g[name + "_total"])]
        if name.startswith("chain"):
            assert x.shape[0] == 1 and name + "_colb" not in g
        else:
            forms.append((y[:1], None if ym is None else ym[:1], g[name + "_colb"], g[name + "_totalb"]))
        for yy, yym, col, total in forms:
            assert col.shape == x.shape[:2] and col.dtype == np.int32 and total.shape == x.shape[:1] and total.dtype == np.float64
            for b in range(x.shape[0]):
                by = b if yy.shape[0] == x.shape[0] else 0
                vx = np.arange(x.shape[1]) if xm is None else np.flatnonzero(xm[b])
                vy = np.arange(yy.shape[1]) if yym is None else np.flatnonzero(yym[by])
                K = min(len(vx), len(vy))
                if K == 0:
                    assert np.isnan(total[b]) and (col[b] == -1).all()
                    continue
                n = np.flatnonzero(col[b] >= 0)
                assert len(n) == K and np.isin(n, vx).all() and np.isin(col[b, n], vy).all() and len(set(col[b, n].tolist())) == K
                assert col[b].max() < yy.shape[1] and (col[b][col[b] < 0] == -1).all()
                C = cost_matrix(x[b], yy[by])
                S = 0.0
                for i in n:                                               # ascending n
                    S += float(C[i, col[b, i]])
                assert total[b] == S, (name, b)
                checked += 1
    assert checked == 6 * 2 * 2 + 4 + 4 + 2


def test_block_wise_hausdorff_reference_equals_the_whole_matrix_one():
    """The reference of the GPU tests evaluates the cost matrix in row blocks; block sizes that divide the cloud, do not, and exceed it give the
    bits and the indices of the whole-matrix form, also where every minimum and maximum is attained many times."""
    from test_gnn_loss import hausdorff_numpy, hausdorff_numpy_whole
    g = load_golden("gnn_loss_cases")
    x, y = g["s257x129_x"], g["s257x129_y"]
    rng = np.random.default_rng(9)
    gx, gy = rng.integers(0, 3, (2, 300, 3)).astype(np.float32), rng.integers(0, 3, (2, 280, 3)).astype(np.float32) + np.float32(0.5)
    gx[:, 150:] = gx[:, :150]
    gy[:, 140:] = gy[:, :140]
    gxm, gym = (rng.random((2, 300)) < 0.6).astype(np.uint8), (rng.random((2, 280)) < 0.6).astype(np.uint8)
    mx, my = g["masked_xm"], g["masked_ym"]
    cases = [(x, y, None, None), (x, y[:1], None, None), (gx, gy, None, None), (gx, gy, gxm, gym), (gx, gy[:1], gxm, gym[:1]),
             (g["masked_x"], g["masked_y"], mx, my)]
    for cx, cy, cxm, cym in cases:
        want_val, want_arg = hausdorff_numpy_whole(cx, cy, cxm, cym)
        for rows in (1, 7, 50, 64, 257, 512):
            val, arg = hausdorff_numpy(cx, cy, cxm, cym, rows=rows)
            assert val.dtype == np.float32 and arg.dtype == np.int32
            assert np.array_equal(val.view(np.int32), want_val.view(np.int32)) and np.array_equal(arg, want_arg), rows
    tied_val, tied_arg = hausdorff_numpy_whole(gx, gy, None, None)
    assert (tied_arg[:, [0, 3]] < 150).all() and (tied_arg[:, [1, 2]] < 140).all()      # (the grid does have its ties: duplicates never win)


def test_loss_spec_parser():
    assert gnn_loss.parse_loss_spec([["mse", 1], ["emd", 0.5]]) == [("mse", 1.0), ("emd", 0.5)]
    assert gnn_loss.parse_loss_spec([("chamfer", 2), ("hausdorff", 0.25)]) == [("chamfer", 2.0), ("hausdorff", 0.25)]
    with pytest.raises(ValueError, match="unknown loss 'sinkhorn'"):
        gnn_loss.parse_loss_spec([["mse", 1], ["sinkhorn", 1]])
    for bad in ("one", None, True, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight"):
            gnn_loss.parse_loss_spec([["emd", bad]])
    for bad in ([], "emd", [["emd"]], [["emd", 1, 2]], ["emd", 1]):
        with pytest.raises(ValueError):
            gnn_loss.parse_loss_spec(bad)
    funcs = gnn_loss.build_loss_funcs(gnn_loss.parse_loss_spec([["mse", 1], ["emd", 0.5]]))
    assert [w for _, w in funcs] == [1.0, 0.5] and all(callable(f) for f, _ in funcs)


def test_new_entry_points_agree_in_header_map_build_and_table():
    protos = declared_prototypes()
    for name in NEW:
        assert name in protos and name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
        assert protos[name][0] == "int" and protos[name][1][-1] == "ag_stream_t"
    assert signature_mismatches({n: _lib.SIGNATURES[n] for n in protos}) == []
    csrc = os.path.join(ROOT, "adaptigraph_amd", "csrc")
    assert re.search(r"global:\s*ag_\*;", open(os.path.join(csrc, "exports.map")).read())
    assert "ag_match.hip" in open(os.path.join(csrc, "Makefile")).read().split("SRCS    :=")[1].splitlines()[0]
    header = open(os.path.join(ROOT, "include", "adaptigraph_hip.h")).read()
    limit = int(re.search(r"#define AG_EMD_MAX_POINTS (\d+)", header).group(1))
    assert limit == _lib.AG_EMD_MAX_POINTS and limit & (limit - 1) == 0 and limit <= 1024
    assert "loss.py:29-55" in header and "loss.py:70-75" in header              # the reference lines they replace


def test_argument_checks_need_no_gpu():
    """Sizes, the limit and the mask pair are refused with AG_ERR_ARG before any HIP call."""
    L = _lib.lib()
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    limit = _lib.AG_EMD_MAX_POINTS
    assert L.ag_emd(p, None, p, None, 1, 0, 1, 1, p, p, p, None) == -1
    assert L.ag_emd(p, None, p, None, 1, 1, 0, 1, p, p, p, None) == -1
    assert L.ag_emd(p, None, p, None, 1, limit + 1, 1, 1, p, p, p, None) == -1 and b"AG_EMD_MAX_POINTS" in L.ag_last_error()
    assert L.ag_emd(p, None, p, None, 1, 1, limit + 1, 1, p, p, p, None) == -1
    assert L.ag_emd(p, p, p, None, 1, 1, 1, 1, p, p, p, None) == -1 and b"both masks" in L.ag_last_error()
    assert L.ag_emd(p, None, p, None, 1, 1, 1, 1, p, None, p, None) == -1 and b"null" in L.ag_last_error()
    assert L.ag_emd_backward(p, p, p, p, p, 1, 1, limit + 1, 1, p, None, None) == -1
    assert L.ag_emd_backward(p, p, None, p, p, 1, 1, 1, 1, p, None, None) == -1
    assert L.ag_hausdorff(p, None, p, None, 1, 0, 1, 1, p, p, None) == -1
    assert L.ag_hausdorff(p, None, p, p, 1, 1, 1, 1, p, p, None) == -1
    assert L.ag_hausdorff(p, None, p, None, 1, 12800, 1, 1, p, p, None) == -1 and b"12800" in L.ag_last_error()
