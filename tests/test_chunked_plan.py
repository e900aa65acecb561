"""A planning step of all chunks in one pass (`ag_plan_cost_chunked`, `ag_mppi_update`, `mpc.running_cost_chunked`,
`plan_utils.optimize_action_mppi_chunks`, `plan_utils.sample_action_seq_chunks`, `mpc.ChunkedPlanner`): argument checks and the tensor-op routes on
the CPU; on the GPU the chunked reward bit for bit against the call on each slice, the update's arg-max and copies exactly and its values against
the float64 mirror next to the float32 tensor ops, the planner against the per-chunk loop of `mpc.Planner` + `merge_res`, and HIP-graph capture."""
import ctypes
from functools import partial

import numpy as np
import pytest
import torch

from adaptigraph_amd import _lib, configs, losses, mpc, synth
from adaptigraph_amd import plan_utils as pu
from test_plan_cost import PEN_T, T_ERR, T_FAR, VALUE_BBOX, VALUE_BOX, chamfer64, make_value_inputs, value_target

CLOTH = configs.task_config("cloth")
LO, HI = np.array(CLOTH["action_lower_lim"], np.float32), np.array(CLOTH["action_upper_lim"], np.float32)
PUSH, WEIGHT = float(CLOTH["push_length"]), 500.0


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_entry_points_reject_bad_arguments_without_a_gpu():
    """Every check runs before any HIP call: AG_ERR_ARG and a message, no crash (the pointers are never dereferenced)."""
    L = _lib.lib()
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    cost = lambda prm, n_chunk, st=p, rw=p: L.ag_plan_cost_chunked(ctypes.byref(prm) if prm is not None else None, n_chunk, st, p, p, p, rw, None, p,
                                                                   1 << 20, None)
    prm = _lib.PlanCostParams(6, 2, 10, 1, 1, 10.0)
    assert cost(None, 2) == -1 and b"null parameters" in L.ag_last_error()
    for n_chunk in (0, -2, 4, 7):                             # no chunk, and 6 samples in 4 or 7 chunks
        assert cost(prm, n_chunk) == -1 and b"chunks of S >= 1" in L.ag_last_error(), n_chunk
    assert cost(_lib.PlanCostParams(0, 2, 10, 1, 1, 10.0), 1) == -1 and b"at least 1" in L.ag_last_error()
    assert cost(_lib.PlanCostParams(6, 2, 10, 7, 1, 10.0), 2) == -1 and b"unknown penalty" in L.ag_last_error()
    assert cost(prm, 3, st=None) == -1 and b"null argument" in L.ag_last_error()
    assert cost(prm, 3, rw=None) == -1 and b"null argument" in L.ag_last_error()

    def update(C=2, S=3, L_=1, ac=p, rw=p, null=False):
        prm = _lib.MppiParams(C, S, L_, 500.0, 0.1)
        return L.ag_mppi_update(None if null else ctypes.byref(prm), ac, rw, p, p, p, p, None)
    assert update(null=True) == -1 and b"null parameters" in L.ag_last_error()
    assert update(ac=None) == -1 and b"null argument" in L.ag_last_error()
    assert update(rw=None) == -1 and b"null argument" in L.ag_last_error()
    for kw in (dict(C=0), dict(S=0), dict(L_=0), dict(S=-5)):
        assert update(**kw) == -1 and b"at least 1" in L.ag_last_error(), kw
    for kw in (dict(C=1 << 15, S=1 << 15, L_=2), dict(C=1 << 20, S=1 << 20, L_=1), dict(C=1, S=1 << 30, L_=2)):
        assert update(**kw) == -1 and b"exceeds 2^30" in L.ag_last_error(), kw


@pytest.mark.parametrize("penalty", ["rope", "cloth", "granular", None])
def test_chunked_cost_on_cpu_tensors_is_running_cost_per_slice(penalty):
    C, S = 3, 5
    state, action, init = (torch.from_numpy(a) for a in make_value_inputs(penalty or "rope", C * S, 2, 20, seed=4))
    state = state * torch.linspace(0.5, 1.5, C).repeat_interleave(S)[:, None, None, None]      # every chunk its own largest error
    pf = partial(PEN_T[penalty], sim_real_ratio=1.0) if penalty else mpc._no_penalty
    cham = partial(chamfer64, y=torch.from_numpy(value_target(20)))
    for kw, ef in ((dict(box_target=VALUE_BOX), partial(losses.box_loss, target=torch.from_numpy(VALUE_BOX))), (dict(error_func=cham), cham)):
        got = mpc.running_cost_chunked(state, action, init, C, VALUE_BBOX, penalty, sim_real_ratio=1.0, **kw)["reward_seqs"]
        want = torch.cat([mpc.running_cost(state[c * S:(c + 1) * S], action[c * S:(c + 1) * S], init, ef, pf, VALUE_BBOX)["reward_seqs"]
                          for c in range(C)])
        whole = mpc.running_cost(state, action, init, ef, pf, VALUE_BBOX)["reward_seqs"]
        assert got.shape == (C * S,) and torch.equal(got, want) and not torch.equal(got, whole)
    with pytest.raises(ValueError, match="chunks of equal size"):
        mpc.running_cost_chunked(state, action, init, 4, VALUE_BBOX, penalty, sim_real_ratio=1.0, box_target=VALUE_BOX)


def update_inputs(C, S, L, seed=7):
    """The value recipe: a base sequence per chunk inside the middle half of the limits (|theta| <= 2), uniform jitter of +-(0.3, 0.3, 0.25, 1.0)
    per sample, rewards uniform in [-0.02, 0] ([-0.01, 0] for S <= 63)."""
    rng = np.random.default_rng(seed)
    mid, half = (LO + HI) / 2, (HI - LO) / 4
    base = rng.uniform(mid - half, mid + half, (C, 1, L, 4))
    base[..., 2] = rng.uniform(-2.0, 2.0, (C, 1, L))
    acts = (base + rng.uniform(-1, 1, (C, S, L, 4)) * np.array([0.3, 0.3, 0.25, 1.0])).astype(np.float32)
    reward = rng.uniform(-0.01 if S <= 63 else -0.02, 0.0, (C, S)).astype(np.float32)
    return acts, reward


def mirror64(acts, reward, clip=True):
    """plan_utils.optimize_action_mppi per chunk in float64 on the float32 inputs; clip=False: the values before the clamp (theta wrapped), and
    the softmax weights."""
    a, r = torch.from_numpy(acts).double(), torch.from_numpy(reward).double()
    if clip:
        lo, hi = torch.from_numpy(LO).double(), torch.from_numpy(HI).double()
        return torch.stack([pu.optimize_action_mppi(a[c], r[c], WEIGHT, lo, hi, PUSH) for c in range(a.shape[0])])
    w = torch.softmax(r * WEIGHT, dim=1)
    ends = [(w[:, :, None] * v).sum(dim=1) for v in pu._push_ends(a, PUSH)]
    raw = pu._from_ends(*ends, PUSH)
    raw[..., 2] = pu.angle_normalize(raw[..., 2])
    return raw, w


UPDATE_SHAPES = [(1, 1, 1), (3, 2, 1), (2, 63, 2), (3, 64, 1), (2, 65, 3), (1, 1030, 2), (40, 500, 1)]


@pytest.mark.parametrize("C,S,L", UPDATE_SHAPES)
def test_update_on_cpu_tensors_is_the_per_chunk_functions(C, S, L):
    acts, reward = update_inputs(C, S, L)
    reward[C - 1, S // 2] = reward[C - 1].max()                # a tie: the first index wins
    a, r, lo, hi = (torch.from_numpy(x) for x in (acts, reward, LO, HI))
    new_seq, idx, seq, rew = pu.optimize_action_mppi_chunks(a, r, WEIGHT, lo, hi, PUSH)
    assert new_seq.shape == (C, L, 4) and idx.shape == (C,) and idx.dtype == torch.int32 and seq.shape == (C, L, 4) and rew.shape == (C,)
    for c in range(C):
        assert torch.equal(new_seq[c], pu.optimize_action_mppi(a[c], r[c], WEIGHT, lo, hi, PUSH))
        k = int(torch.argmax(r[c]))
        assert int(idx[c]) == k == int(np.argmax(reward[c])) and torch.equal(seq[c], a[c, k]) and rew[c] == r[c, k]


def test_value_inputs_exercise_the_mean():
    """The recipe's own conditions on the float64 mirror, without a GPU: effective sample size >= 8 for S >= 63, |theta'| <= 2.2, length'
    strictly inside (2.5, 9.5), and the float32 tensor ops within 1e-5 of float64."""
    for C, S, L in UPDATE_SHAPES:
        acts, reward = update_inputs(C, S, L)
        check_mirror(acts, reward)
        f32 = torch.stack([pu.optimize_action_mppi(torch.from_numpy(acts[c]), torch.from_numpy(reward[c]), WEIGHT, torch.from_numpy(LO),
                                                   torch.from_numpy(HI), PUSH) for c in range(C)])
        assert float((f32.double() - mirror64(acts, reward)).abs().max()) <= 1e-5


def check_mirror(acts, reward):
    raw, w = mirror64(acts, reward, clip=False)
    ess = 1.0 / (w * w).sum(dim=1)
    assert acts.shape[1] < 63 or float(ess.min()) >= 8, ess
    assert float(raw[..., 2].abs().max()) <= 2.2 and 2.5 < float(raw[..., 3].min()) and float(raw[..., 3].max()) < 9.5
    return float(ess.min()), float(ess.max())


def test_chunk_sampler_iteration_0_is_the_loop_under_one_seed():
    C, S, L = 3, 5, 2
    lo, hi = torch.from_numpy(LO), torch.from_numpy(HI)
    seq = torch.from_numpy(update_inputs(C, 1, L)[0][:, 0])
    torch.manual_seed(11)
    want = torch.stack([pu.sample_action_seq(seq[c], lo, hi, S, "cpu", iter_index=0, noise_level=0.3, push_length=PUSH) for c in range(C)])
    torch.manual_seed(11)
    got = pu.sample_action_seq_chunks(seq, lo, hi, S, "cpu", iter_index=0, noise_level=0.3, push_length=PUSH)
    assert got.shape == (C, S, L, 4) and torch.equal(got, want)


def test_chunk_sampler_later_iterations_with_injected_noise_are_the_loop():
    C, S, L, level = 3, 6, 2, 0.3
    lo, hi = torch.from_numpy(LO), torch.from_numpy(HI)
    seq = torch.from_numpy(update_inputs(C, 1, L)[0][:, 0])
    want, draws = [], []
    for c in range(C):                                         # the loop's draws for chunk c: one normal(S, 4) per look-ahead index
        torch.manual_seed(100 + c)
        draws.append([torch.normal(0, level, (S, 4)) for _ in range(L)])
        torch.manual_seed(100 + c)
        want.append(pu.sample_action_seq(seq[c], lo, hi, S, "cpu", iter_index=1, noise_level=level, push_length=PUSH))
    noise = [torch.stack([draws[c][i] for c in range(C)]) for i in range(L)]
    got = pu.sample_action_seq_chunks(seq, lo, hi, S, "cpu", iter_index=1, noise_level=level, push_length=PUSH, noise=noise)
    assert got.shape == (C, S, L, 4) and torch.equal(got, torch.stack(want))
    assert torch.equal(got[:, 0], seq) and not torch.equal(got[:, 1], seq)      # sample 0 of every chunk is the unperturbed sequence
    torch.manual_seed(5)                                       # without `noise`: one draw of (C, S, 4) per look-ahead index
    drawn = pu.sample_action_seq_chunks(seq, lo, hi, S, "cpu", iter_index=1, noise_level=level, push_length=PUSH)
    torch.manual_seed(5)
    noise = [torch.normal(0, level, (C, S, 4)) for _ in range(L)]
    assert torch.equal(drawn, pu.sample_action_seq_chunks(seq, lo, hi, S, "cpu", iter_index=1, noise_level=level, push_length=PUSH, noise=noise))


# ---------------------------------------------------------------------------------------------------------------- GPU
DEV = "cuda:0"
COST_SHAPES = [(1, 1, 1, 1), (3, 1, 2, 63), (2, 63, 1, 64), (3, 64, 2, 65), (40, 500, 1, 200)]


def tg(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def cost_inputs(C, S, L, n, seed):
    """Clouds in a 4 x 4 square, scaled per chunk (so that every chunk has its own largest error), pushes that start inside it."""
    rng = np.random.default_rng(seed)
    B = C * S
    state = rng.uniform(0, 4, (B, L, n, 3)).astype(np.float32) * np.repeat(rng.uniform(0.5, 1.5, C), S).astype(np.float32)[:, None, None, None]
    init = rng.uniform(0, 4, (n, 3)).astype(np.float32)
    action = rng.uniform(0, 4, (B, L, 4)).astype(np.float32)
    action[..., 2] = rng.uniform(-3.14, 3.14, (B, L))
    return state, action, init


def chunked_and_slices(st, ac, si, C, penalty, criterion, given=None, ratio=1.0):
    """The chunked call's rewards and terms, and the fused call on every chunk's slice."""
    S, L = st.shape[0] // C, st.shape[1]
    kw = dict(box_target=VALUE_BOX) if criterion == "box" else dict(error_func=lambda s: given)
    out = mpc.running_cost_chunked(st, ac, si, C, VALUE_BBOX, penalty, sim_real_ratio=ratio, return_terms=True, **kw)
    parts = []
    for c in range(C):
        rows = slice(c * S, (c + 1) * S)
        if criterion != "box":
            kw = dict(error_func=lambda s, c=c: given[c * S * L:(c + 1) * S * L])
        parts.append(mpc.running_cost_fused(st[rows], ac[rows], si, VALUE_BBOX, penalty, sim_real_ratio=ratio, return_terms=True, **kw))
    return out, parts


@pytest.mark.gpu
@pytest.mark.parametrize("C,S,L,n", COST_SHAPES)
def test_chunked_reward_is_the_fused_call_on_every_slice(C, S, L, n):
    st, ac, si = (tg(a) for a in cost_inputs(C, S, L, n, seed=C + S + n))
    given = losses.chamfer(st.reshape(C * S * L, n, 3), tg(value_target(n)))
    differs = 0
    for penalty in ("rope", "cloth", "granular", None):
        for criterion in ("box", "given"):
            out, parts = chunked_and_slices(st, ac, si, C, penalty, criterion, given)
            assert out["reward_seqs"].shape == (C * S,) and bool(torch.isfinite(out["reward_seqs"]).all())
            assert torch.equal(out["reward_seqs"], torch.cat([p["reward_seqs"] for p in parts])), (penalty, criterion)
            assert torch.equal(out["terms"], torch.cat([p["terms"] for p in parts])), (penalty, criterion)
            kw = dict(box_target=VALUE_BOX) if criterion == "box" else dict(error_func=lambda s: given)
            whole = mpc.running_cost_fused(st, ac, si, VALUE_BBOX, penalty, sim_real_ratio=1.0, **kw)["reward_seqs"]
            one = mpc.running_cost_chunked(st, ac, si, 1, VALUE_BBOX, penalty, sim_real_ratio=1.0, **kw)["reward_seqs"]
            assert torch.equal(one, whole)                     # n_chunk = 1 is ag_plan_cost
            differs += int(not torch.equal(out["reward_seqs"], whole))
    assert differs == (8 if C > 1 else 0)                      # (the chunks' normalisers are not the whole call's)


@pytest.mark.gpu
def test_chunk_maxima_in_the_last_sample_of_a_chunk():
    """A small cloth (sim_real_ratio 1: the cap on the farthest distance is 0.4).  The LAST sample of every chunk has the chunk's largest error
    and the largest farthest distance: beyond the cap in chunk 0 (the cap binds), below it in chunk 1; the FIRST sample of chunk 2 has a larger
    error than all of chunk 1.  A chunk border one sample off changes a normaliser."""
    C, S, L, n = 3, 64, 2, 65
    rng = np.random.default_rng(21)
    state = rng.uniform(0, 0.2, (C * S, L, n, 3)).astype(np.float32)
    init = rng.uniform(0, 0.2, (n, 3)).astype(np.float32)
    action = rng.uniform(0, 0.2, (C * S, L, 4)).astype(np.float32)      # grasp points inside the cloth: no particle farther than its diagonal, 0.283
    for c, reach in ((0, 0.7), (1, 0.38), (2, 0.33)):
        last = c * S + S - 1
        state[last, :, :, 2] -= 3.0 + c                        # far from the target box: the chunk's largest box_loss
        action[last, :, 0], action[last, :, 1] = reach, 0.1
    state[2 * S, :, :, 2] -= 9.0
    st, ac, si = tg(state), tg(action), tg(init)
    given = tg(rng.uniform(0.1, 1.0, C * S * L).astype(np.float32))
    for c in range(C):
        given[(c * S + S - 1) * L + L - 1] = 2.0 + c
    given[2 * S * L] = 7.0
    for criterion in ("box", "given"):
        out, parts = chunked_and_slices(st, ac, si, C, "cloth", criterion, given)
        terms = out["terms"].reshape(C, S * L, -1)
        assert (terms[..., T_ERR].argmax(dim=1) // L).tolist() == [S - 1, S - 1, 0] and terms[2, 0, T_ERR] > terms[1, :, T_ERR].max()
        assert (terms[..., T_FAR].argmax(dim=1) // L).tolist() == [S - 1] * C
        cap = float(np.float32(0.4))
        far = terms[..., T_FAR].max(dim=1).values
        assert float(far[0]) > cap > float(far[1]) > 0.3 and int((terms[0, :, T_FAR] > cap).sum()) == L
        assert torch.equal(out["reward_seqs"], torch.cat([p["reward_seqs"] for p in parts])), criterion
        assert torch.equal(out["terms"], torch.cat([p["terms"] for p in parts])), criterion


@pytest.mark.gpu
@pytest.mark.parametrize("criterion", ["box", "given"])
def test_nan_stays_inside_its_chunk(criterion):
    C, S, L, n = 3, 9, 2, 70
    state, action, init = cost_inputs(C, S, L, n, seed=5)
    state[S + 4, 0, n - 1, 2] = np.nan                         # chunk 1, sample 4
    st, ac, si = tg(state), tg(action), tg(init)
    given = torch.linspace(0.5, 1.5, C * S * L, device=DEV)
    for penalty in ("rope", "cloth", "granular"):
        out, parts = chunked_and_slices(st, ac, si, C, penalty, criterion, given)
        got, want = out["reward_seqs"].reshape(C, S), torch.stack([p["reward_seqs"] for p in parts])
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (penalty, got, want)
        assert bool(torch.isnan(got[1, 4])) and bool(torch.isnan(got[1]).all()) == (criterion == "box")
        assert not bool(torch.isnan(got[[0, 2]]).any()) and torch.equal(got[[0, 2]], want[[0, 2]])
        ok = ~torch.isnan(want)
        assert torch.equal(got[ok], want[ok])


def update_on_gpu(acts, reward):
    return pu.optimize_action_mppi_chunks(tg(acts), tg(reward), WEIGHT, LO, HI, PUSH)


def exact_inputs(C, S, L, seed):
    """Sequences around a base per chunk that lies inside, below or above the limits by turns (the means of most chunks get clamped)."""
    rng = np.random.default_rng(seed)
    span = HI - LO
    base = np.stack([(LO + span * f) for f in ([0.5, 0.5, 0.5, 0.5], [-0.2, 1.3, 0.4, -0.3], [1.2, -0.1, 0.6, 1.4])])[np.arange(C) % 3]
    acts = (base[:, None, None, :] + rng.uniform(-1, 1, (C, S, L, 4)) * np.array([0.3, 0.3, 0.25, 1.0])).astype(np.float32)
    acts[..., 3] = np.maximum(acts[..., 3], 0.05)
    return acts, rng.uniform(-0.02, 0.0, (C, S)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("C,S,L", UPDATE_SHAPES)
def test_update_exact_parts(C, S, L):
    acts, reward = exact_inputs(C, S, L, seed=C + S + L)
    variants = {"random": reward}
    if S >= 2:
        variants["tie_first_last"] = reward.copy()
        variants["tie_first_last"][:, [0, S - 1]] = 1.0
        variants["tie_last_two"] = reward.copy()
        variants["tie_last_two"][:, [S - 2, S - 1]] = 1.0
    if S >= 65:
        variants["tie_63_64"] = reward.copy()
        variants["tie_63_64"][:, [63, 64]] = 1.0
    variants["all_equal"] = np.full_like(reward, -0.5)
    variants["nan"] = reward.copy()
    variants["nan"][C - 1, S // 2] = np.nan
    variants["nan"][C - 1, S - 1] = np.nan                     # (the first NaN wins)
    results = {}
    for name, r in variants.items():
        new_seq, idx, seq, rew = results[name] = update_on_gpu(acts, r)
        want = np.argmax(r, axis=1)
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want), (name, idx, want)
        assert np.array_equal(seq.cpu().numpy(), acts[np.arange(C), want]), name
        assert np.array_equal(rew.cpu().numpy().view(np.int32), r[np.arange(C), want].view(np.int32)), name
        again = update_on_gpu(acts, r)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(results[name], again)), name
    if S >= 2:
        assert results["tie_first_last"][1].tolist() == [0] * C and results["tie_last_two"][1].tolist() == [S - 2] * C
    if S >= 65:
        assert results["tie_63_64"][1].tolist() == [63] * C
    assert results["all_equal"][1].tolist() == [0] * C and results["nan"][1][C - 1].item() == S // 2
    # a NaN reward: its chunk's new sequence is NaN, every other chunk keeps the bits it has without it
    assert bool(torch.isnan(results["nan"][0][C - 1]).all()) and torch.equal(results["nan"][0][:C - 1], results["random"][0][:C - 1])
    assert bool(torch.isfinite(results["random"][0]).all())
    # action rows that start 4 bytes off a 16-byte boundary (a view into a larger buffer): the same bits
    shifted = torch.empty(acts.size + 1, device=DEV)[1:].view(acts.shape).copy_(tg(acts))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    off = pu.optimize_action_mppi_chunks(shifted, tg(reward), WEIGHT, LO, HI, PUSH)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(results["random"], off))
    # beyond a limit by more than 1e-3 in the float64 mirror: the output IS the limit
    new_seq = results["random"][0].cpu().numpy()
    raw = mirror64(acts, reward, clip=False)[0].numpy()
    below, above = raw < LO.astype(np.float64) - 1e-3, raw > HI.astype(np.float64) + 1e-3
    assert np.array_equal(new_seq[below], np.broadcast_to(LO, raw.shape)[below]) and np.array_equal(new_seq[above], np.broadcast_to(HI, raw.shape)[above])
    assert C < 3 or (below.any() and above.any())
    inside = ~below & ~above
    assert np.abs(new_seq[inside] - np.clip(raw, LO, HI)[inside]).max() <= 1e-3
    if S == 1:                                                 # weight exactly 1: x and z are the clamped inputs bit for bit
        want = np.ascontiguousarray(np.clip(acts[:, 0, :, :2], LO[:2], HI[:2]))
        assert np.array_equal(np.ascontiguousarray(new_seq[..., :2]).view(np.int32), want.view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("C,S,L", UPDATE_SHAPES)
def test_update_values_against_float64_next_to_the_tensor_ops(C, S, L):
    """Both float32 evaluations on the GPU against the float64 mirror on the same inputs: e_kernel <= 2 e_tensor_ops + 1e-6."""
    acts, reward = update_inputs(C, S, L)
    ess = check_mirror(acts, reward)
    ref = mirror64(acts, reward)
    a, r, lo, hi = tg(acts), tg(reward), tg(LO), tg(HI)
    ops = torch.stack([pu.optimize_action_mppi(a[c], r[c], WEIGHT, lo, hi, PUSH) for c in range(C)])
    got = update_on_gpu(acts, reward)[0]
    e_ops, e_kernel = float((ops.double().cpu() - ref).abs().max()), float((got.double().cpu() - ref).abs().max())
    print(f"mppi update values {C}x{S}x{L}: ess {ess[0]:.1f}..{ess[1]:.1f} e_tensor_ops {e_ops:.3e} e_kernel {e_kernel:.3e}")
    assert e_kernel <= 2 * e_ops + 1e-6, (e_kernel, e_ops)


def planner_setup(weights, shared_state):
    from adaptigraph_amd.forward_dynamics import dynamics
    from adaptigraph_amd.model import DynamicsPredictor
    mat = "rope"
    task = configs.task_config(mat)
    C, S = 3, 8
    state, act0 = synth.make_mpc_inputs(mat, 60, C * S, seed=17, len_lo=1, len_hi=2.9, spacing=0.1)
    _, act1 = synth.make_mpc_inputs(mat, 60, C * S, seed=18, len_lo=1, len_hi=2.9, spacing=0.1)
    target = (state[::3] + np.array([0.3, 0.0, 0.2], np.float32)).astype(np.float32)
    bbox = np.array([[state[:, 0].min() - 1, state[:, 0].max() + 1], [state[:, 2].min() - 1, state[:, 2].max() + 1]])
    lo, hi = np.array(task["action_lower_lim"], np.float32), np.array(task["action_upper_lim"], np.float32)
    lo[3], hi[3] = 1.0, 3.0
    model = DynamicsPredictor(configs.model_config(), configs.material_config(mat), configs.dataset_config(mat), DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()})
    model = model.to(DEV).eval().set_option("precision", 0).set_option("shared_state", shared_state)
    ppm = configs.ppm_optimizer_stub(mat)
    ppm.physics_param = {mat: torch.tensor([0.5], device=DEV)}
    cost = dict(bbox=bbox, penalty="rope", sim_real_ratio=task["sim_real_ratio"], error_func=partial(losses.chamfer, y=tg(target)[None]))
    cfg = dict(action_dim=4, model_rollout_fn=partial(dynamics, model=model, device=DEV, ppm_optimizer=ppm), n_sample=S, n_look_ahead=1,
               reward_weight=WEIGHT, action_lower_lim=tg(lo), action_upper_lim=tg(hi), planner_type="MPPI", device=DEV, noise_level=1.0)
    return cfg, cost, tg(state), [tg(act0), tg(act1)], C, S, float(task["push_length"]), target


@pytest.mark.gpu
@pytest.mark.parametrize("shared_state", [0, 1])
def test_chunked_planner_is_the_loop_of_planners(weights, shared_state):
    """Seed-0 weights, a 60-particle rope, 3 chunks of 8 injected samples, L = 1, length limits [1, 3]: `ChunkedPlanner` against one `mpc.Planner`
    per chunk (scored by `running_cost_fused`, fed the same sample slices) + `merge_res`."""
    cfg, cost, state, samples, C, S, push, target = planner_setup(weights, shared_state)
    lo, hi = cfg["action_lower_lim"], cfg["action_upper_lim"]
    for n_iter in (1, 2):
        res_list = []
        for c in range(C):
            loop = mpc.Planner(dict(cfg, n_update_iter=n_iter, evaluate_traj_fn=partial(mpc.running_cost_fused, **cost),
                                    sampling_action_seq_fn=lambda act_seq, iter_index=0, c=c: samples[iter_index][c * S:(c + 1) * S].clone(),
                                    optimize_action_mppi_fn=partial(pu.optimize_action_mppi, reward_weight=WEIGHT, action_lower_lim=lo,
                                                                    action_upper_lim=hi, push_length=push)))
            res = loop.trajectory_optimization(state, samples[0][0])
            res_list.append({k: ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in res.items()})
        want = loop.merge_res(res_list)
        planner = mpc.ChunkedPlanner(dict(cfg, n_update_iter=n_iter, n_chunk=C, cost=cost, push_length=push))
        got = planner.trajectory_optimization(state, samples[0][0], samples=samples[:n_iter])
        assert set(got) == set(want) | {"chunks"}
        assert got["act_seq"].shape == (1, 4) and torch.equal(got["act_seq"], want["act_seq"])
        assert torch.equal(got["best_model_output"]["state_seqs"], want["best_model_output"]["state_seqs"])
        assert got["best_eval_output"]["reward_seqs"].shape == (1,)
        assert torch.equal(got["best_eval_output"]["reward_seqs"], want["best_eval_output"]["reward_seqs"])
        chunks = got["chunks"]
        assert torch.equal(chunks["act_seq"], torch.stack([r["act_seq"] for r in res_list]))
        assert torch.equal(chunks["best_reward_seqs"], torch.cat([r["best_eval_output"]["reward_seqs"] for r in res_list]))
        assert len(chunks["new_seqs"]) == n_iter              # (scored alone, a sequence's error term is -2 e / (e + 1e-6): chunks do tie, and
                                                               # both merges break the tie with the same device arg-max)
    # every chunk's MPPI mean after iteration 0 against the loop's optimize_action_mppi, by the value bound
    acts = samples[0]
    reward = mpc.running_cost_chunked(cfg["model_rollout_fn"](state, acts)["state_seqs"], acts, state, C, **cost)["reward_seqs"]
    ops = torch.stack([pu.optimize_action_mppi(acts[c * S:(c + 1) * S], reward[c * S:(c + 1) * S], WEIGHT, lo, hi, push) for c in range(C)])
    ref = torch.stack([pu.optimize_action_mppi(acts[c * S:(c + 1) * S].double().cpu(), reward[c * S:(c + 1) * S].double().cpu(), WEIGHT,
                                               lo.double().cpu(), hi.double().cpu(), push) for c in range(C)])
    e_ops, e_kernel = float((ops.double().cpu() - ref).abs().max()), float((chunks["new_seqs"][0].double().cpu() - ref).abs().max())
    print(f"chunked planner new_seq after iteration 0 (shared_state {shared_state}): e_tensor_ops {e_ops:.3e} e_kernel {e_kernel:.3e}")
    assert e_kernel <= 2 * e_ops + 1e-6, (e_kernel, e_ops)


@pytest.mark.gpu
def test_cost_and_update_are_captured_in_one_graph_and_replay_on_new_inputs():
    C, S, L, n = 5, 33, 2, 130
    sets = [tuple(tg(a) for a in make_value_inputs("granular", C * S, L, n, seed=s)) for s in range(4)]
    given = [torch.rand(C * S * L, device=DEV) + 0.1 * s for s in range(4)]
    st, ac, si, er = (t.clone() for t in (*sets[0], given[0]))

    def run():
        reward = mpc.running_cost_chunked(st, ac, si, C, VALUE_BBOX, "granular", sim_real_ratio=1.0, error_func=lambda s: er)["reward_seqs"]
        return (reward,) + pu.optimize_action_mppi_chunks(ac.reshape(C, S, L, 4), reward.reshape(C, S), 50.0, [-5, -5, -3.14, 2], [9, 9, 3.14, 14], 0.1)
    run()                                                      # (the grow-only workspace exists before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for s in (1, 2, 3):
        for dst, src in zip((st, ac, si, er), (*sets[s], given[s])):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out]
        eager = run()
        assert all(torch.equal(g, e) for g, e in zip(got, eager)), s
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
        assert len({float(v) for v in got[1][:, 0, 0]}) == C    # (every chunk has a mean of its own)
