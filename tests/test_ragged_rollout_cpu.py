"""Ragged rollout without a GPU: the argument checks of `ag_rollout_order` / `ag_rollout_ragged` (codes and messages, before any HIP call) and
the CPU-tensor form of the ordering (`forward_dynamics.rollout_order`) against numpy."""
import ctypes

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib
from adaptigraph_amd.forward_dynamics import rollout_order

S = _lib.AG_RAGGED_MAX_STEPS


def test_rollout_order_rejects_bad_arguments_without_a_gpu():
    L = _lib.lib()
    buf = (ctypes.c_int32 * (S + 1))()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for args in ((None, 4, p, p), (p, 4, None, p), (p, 4, p, None)):
        assert L.ag_rollout_order(*args, None) == -1 and b"ag_rollout_order: null argument" in L.ag_last_error(), args
    for B in (0, -3):
        assert L.ag_rollout_order(p, B, p, p, None) == -1 and b"(>= 1)" in L.ag_last_error(), B


def test_rollout_ragged_rejects_bad_arguments_without_a_gpu():
    """Every check below runs before the model is read and before any HIP call: the handle and the device pointers are dummies that are never
    dereferenced; the parameters and active_per_step are real host memory."""
    L = _lib.lib()
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    B = 6

    def call(n_steps=3, active=(6, 4, 4), model=p, prm=True, height=_lib.AG_HEIGHT_MIN, sizes=None, **null):
        prm_ = _lib.RolloutParams(*(sizes or (B, 9, 8, 1, 10, 0, 1)), n_steps, height, 0.0)
        act = None if active is None else (ctypes.c_int32 * max(len(active), 1))(*active)
        names = ("state0", "delta", "attrs", "p_instance", "phys", "mask", "tool_mask", "obj_mask", "thr_sq", "repeat")
        ptrs = [None if null.get(n) else p for n in names]
        return L.ag_rollout_ragged(model, ctypes.byref(prm_) if prm else None, *ptrs, act, None if null.get("out_index", True) else p,
                                   None if null.get("out_seq") else p, None, None if null.get("workspace") else p, 1 << 20, None)

    assert call(model=None) == -1 and b"ag_rollout_ragged: null argument" in L.ag_last_error()
    assert call(prm=False) == -1 and b"null argument" in L.ag_last_error()
    for name in ("state0", "delta", "attrs", "p_instance", "mask", "tool_mask", "thr_sq", "repeat", "out_seq", "workspace"):
        assert call(**{name: True}) == -1 and b"ag_rollout_ragged: null argument" in L.ag_last_error(), name
    assert call(active=None) == -1 and b"null argument (active_per_step)" in L.ag_last_error()
    assert call(height=_lib.AG_HEIGHT_MASKED_MEAN, obj_mask=True) == -1 and b"obj_mask is null" in L.ag_last_error()
    assert call(sizes=(0, 9, 8, 1, 10, 0, 1)) == -1 and b"bad sizes" in L.ag_last_error()
    assert call(n_steps=S + 1, active=(1,) * (S + 1)) == -1 and b"n_steps=1025 (<= 1024)" in L.ag_last_error()
    for active, where in (((6, 4, 5), b"active_per_step[2]=5"),      # not non-increasing
                          ((7, 4, 4), b"active_per_step[0]=7"),      # above B
                          ((6, 4, -1), b"active_per_step[2]=-1"),    # below 0
                          ((0, 1, 0), b"active_per_step[1]=1")):
        assert call(active=active) == -1 and where in L.ag_last_error() and b"non-increasing, 0..B=6" in L.ag_last_error(), active


def numpy_order(rep):
    r = np.maximum(rep.astype(np.int64), 0)
    order = np.argsort(-r, kind="stable").astype(np.int32)
    active = np.array([(r >= s + 1).sum() for s in range(S + 1)], np.int32)      # the last word: repeat >= S + 1, i.e. above S
    return order, active


@pytest.mark.parametrize("B", [1, 2, 65])
@pytest.mark.parametrize("case", ["equal", "zeros_and_negatives", "above_1024", "mixed"])
def test_cpu_ordering_agrees_with_numpy(B, case):
    rng = np.random.default_rng(B * 7 + len(case))
    rep = {"equal": np.full(B, 7), "zeros_and_negatives": rng.integers(-3, 2, B), "above_1024": rng.integers(1020, 1030, B),
           "mixed": np.where(rng.uniform(size=B) < 0.1, 2000, rng.integers(-1, 16, B))}[case].astype(np.int32)
    order, active = rollout_order(torch.from_numpy(rep))
    want_order, want_active = numpy_order(rep)
    assert order.dtype == torch.int32 and active.dtype == torch.int32 and active.shape == (S + 1,)
    assert np.array_equal(order.numpy(), want_order) and np.array_equal(active.numpy(), want_active)
    assert int(active[-1]) == int((rep > S).sum()) and int(active[0]) == int((rep >= 1).sum())
    steps = int(np.count_nonzero(active.numpy()[:-1]))
    assert steps == min(max(int(rep.max()), 0), S)
