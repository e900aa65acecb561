"""The set-up pieces the rollout drivers of forward_dynamics.py share, on the CPU: each against the statements it replaced, bit for bit, and the
public signatures against tests/golden/driver_digests.json."""
import inspect
import json
import os

import pytest
import torch

from conftest import GOLDEN
from adaptigraph_amd import forward_dynamics as fd


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def masks(name, bsz, n_obj):
    g = torch.Generator().manual_seed(3)
    if name == "all_true":
        return torch.ones((bsz, n_obj), dtype=torch.bool)
    if name == "single_particle":
        m = torch.zeros((bsz, n_obj), dtype=torch.bool)
        m[torch.arange(bsz), torch.randint(0, n_obj, (bsz,), generator=g)] = True
        return m
    if name == "scattered":
        m = torch.rand((bsz, n_obj), generator=g) < 0.6
    else:                                                  # "counts": a different number of valid slots per sample, anywhere in the row
        m = torch.stack([torch.randperm(n_obj, generator=g) < n_obj - 1 - 2 * b for b in range(bsz)])
        assert len(set(m.sum(1).tolist())) == bsz
    m[:, 0] = True
    return m


def masked_setup_as_it_was(state, state_mask, n_t, max_n, device="cpu"):
    """The lines dynamics_masked and dynamics_masked_differentiable each carried before they shared fd._masked_inputs / fd._masked_height."""
    bsz, n_obj = state.shape[0], state.shape[1]
    N = n_obj + n_t
    cnt = state_mask.sum(dim=1)
    y = (state[:, :, 1] * state_mask).sum(dim=1) / cnt
    attrs = torch.zeros((bsz, N, 2), device=device)
    attrs[:, :n_obj, 0] = state_mask.float()
    attrs[:, n_obj:, 1] = 1.0
    p_instance = torch.zeros((bsz, n_obj, max_n), device=device)
    p_instance[:, :, 0] = (torch.arange(n_obj, device=device)[None] < cnt[:, None]).float()
    mask = torch.ones((bsz, N), dtype=torch.bool, device=device)
    mask[:, :n_obj] = state_mask.bool()
    tool_mask = torch.zeros((bsz, N), dtype=torch.bool, device=device)
    tool_mask[:, n_obj:] = True
    return (attrs, p_instance, mask, tool_mask, state_mask.bool(), cnt), y


@pytest.mark.parametrize("as_float", [False, True], ids=["bool", "float"])
@pytest.mark.parametrize("n_t", [1, 5])
@pytest.mark.parametrize("name", ["all_true", "scattered", "single_particle", "counts"])
def test_masked_inputs_are_the_statements_they_replace(name, n_t, as_float):
    bsz, n_obj, max_n = 5, 23, 2
    state_mask = masks(name, bsz, n_obj)
    state_mask = state_mask.float() if as_float else state_mask
    state = torch.randn((bsz, n_obj, 3), generator=torch.Generator().manual_seed(4))
    want, want_y = masked_setup_as_it_was(state, state_mask, n_t, max_n)
    got = fd._masked_inputs(state_mask, n_t, max_n)
    assert len(got) == len(want) == 6
    for field, a, b in zip(("attrs", "p_instance", "mask", "tool_mask", "obj_mask", "cnt"), got, want):
        assert same(a, b), field
    assert [t.dtype for t in got[:5]] == [torch.float32, torch.float32, torch.bool, torch.bool, torch.bool]
    assert same(fd._masked_height(state, state_mask, got[5]), want_y)


@pytest.mark.parametrize("n_t", [1, 5])
@pytest.mark.parametrize("n_his", [1, 4])
def test_frames_are_the_slice_assignment_form(n_his, n_t):
    bsz, n_obj = 4, 11
    g = torch.Generator().manual_seed(n_his + n_t)
    obj, eef, dlt = torch.randn((bsz, n_obj, 3), generator=g), torch.randn((bsz, n_t, 3), generator=g), torch.randn((bsz, 1, 3), generator=g)
    obj[0, 0, 0], eef[1, 0, 2], dlt[2, 0, 1], dlt[3, 0, 0] = -0.0, -0.0, -0.0, float("nan")
    dlt = dlt.expand(bsz, n_t, 3)                           # _place_tool_lean hands the per-step motion over as an expanded view
    N = n_obj + n_t
    state0 = torch.empty((bsz, n_his, N, 3))
    state0[:, :, :n_obj] = obj[:, None]
    state0[:, :, n_obj:] = eef[:, None]
    delta = torch.zeros((bsz, N, 3))
    delta[:, n_obj:] = dlt
    got0, got_delta = fd._frames(obj, eef, dlt, n_his, torch.zeros((bsz, n_obj, 3)))
    assert same(got0, state0) and same(got_delta, delta)
    assert got0.is_contiguous() and got_delta.is_contiguous()
    assert bool((bits(got0)[0, :, 0, 0] == -2 ** 31).all()) and int(bits(got_delta)[2, n_obj, 1]) == -2 ** 31      # the sign of zero survives


def test_public_signatures_are_the_recorded_ones():
    with open(os.path.join(GOLDEN, "driver_digests.json")) as f:
        want = json.load(f)["signatures"]
    assert len(want) == 10
    for name, sig in want.items():
        assert str(inspect.signature(getattr(fd, name))) == sig, name
