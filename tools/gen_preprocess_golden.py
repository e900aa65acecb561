#!/usr/bin/env python3
"""Goldens for adaptigraph_amd/preprocess.py: the REFERENCE's own process_eef and extract_push (src/dynamics/preprocess/preprocess.py) run on
small made-up tool paths, inputs and results stored side by side.

    python tools/gen_preprocess_golden.py          # seconds of CPU

Output (data only): tests/golden/preprocess_pairs.npz
  push_<i>_eef (T, N, 3), push_<i>_args = [dist_thresh, n_his, n_future, n_frames], push_<i>_pairs, push_<i>_cnt
  eef_<i>_states (T, N, 14) or (T, 14), eef_<i>_pos (max_neef, 3), eef_<i>_out (T, max_neef, 3)
Nothing of the reference's text is copied.
"""
import contextlib
import importlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_import import import_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "preprocess_pairs.npz")


def walk(rng, T, step, dtype=np.float64, n_eef=1):
    """A tool path of T frames: a random walk in x, z with steps around `step`, every key point at its own fixed offset."""
    a = rng.uniform(0, 2 * np.pi, T)
    d = rng.uniform(0.3, 1.7, T) * step
    p = np.cumsum(np.stack([d * np.cos(a), np.zeros(T), d * np.sin(a)], 1), 0)
    off = rng.uniform(-0.05, 0.05, (n_eef, 3))
    return (p[:, None] + off[None]).astype(dtype)


def push_cases(rng):
    line = lambda T, step: np.stack([np.arange(T) * step, np.full(T, 0.03), np.zeros(T)], 1)[:, None]
    cases = [(walk(rng, T, 0.1), (0.1, 4, 3, 0)) for T in (1, 2, 7, 25, 60)]
    cases.append((walk(rng, 30, 0.04, np.float32), (0.1, 4, 3, 17)))                       # several frames per threshold, float32, an offset
    cases.append((np.tile(np.array([[[0.3, 0.03, -0.2]]]), (10, 1, 1)), (0.1, 4, 3, 5)))   # a stationary tool: every row pads
    cases.append((walk(rng, 3, 0.2), (0.1, 4, 3, 0)))                                      # shorter than n_his
    cases.append((line(12, 0.25), (0.25, 4, 3, 0)))                                        # steps exactly equal to the threshold (exact in binary)
    cases.append((line(12, 0.25).astype(np.float32), (0.25, 3, 2, 40)))
    cases.append((line(16, 0.1).astype(np.float32), (0.1, 4, 3, 0)))                       # 0.1 k in float32 against the double 0.1
    cases.append((line(16, 0.1), (0.1, 4, 3, 0)))
    cases.append((walk(rng, 20, 0.1, n_eef=5), (0.1, 1, 1, 3)))                            # granular: five key points, the first decides
    cases.append((walk(rng, 20, 0.15, np.float32), (0.1, 2, 5, 0)))
    return cases


def eef_cases(rng):
    def states(T, n, dtype):
        s = rng.normal(0, 1, (T, n, 14))
        q = rng.normal(0, 1, (T, n, 4))
        s[:, :, 6:10] = q / np.linalg.norm(q, axis=2, keepdims=True)      # unit quaternions, none the identity
        return s.astype(dtype)
    rope, gran = [[0.0, 0.0, 1.0]], [[0.0, 0.0, 0.1], [0.0, 0.05, 0.1], [0.0, 0.025, 0.1], [0.0, -0.025, 0.1], [0.0, -0.05, 0.1]]
    return [(states(6, 1, np.float64), rope), (states(6, 1, np.float32), rope), (states(5, 1, np.float64)[:, 0], rope),
            (states(4, 1, np.float64), gran),                                     # fewer states than key points
            (states(4, 5, np.float32), gran), (states(1, 1, np.float64), [[0.3, -0.2, 0.12]])]


def main():
    import_reference()
    ref = importlib.import_module("dynamics.preprocess.preprocess")
    rng = np.random.default_rng(0)
    out = {}
    for i, (eef, args) in enumerate(push_cases(rng)):
        with contextlib.redirect_stdout(io.StringIO()):
            pairs, cnt = ref.extract_push(eef.copy(), args[0], int(args[1]), int(args[2]), int(args[3]))
        out.update({f"push_{i}_eef": eef, f"push_{i}_args": np.array(args, np.float64), f"push_{i}_pairs": np.asarray(pairs),
                    f"push_{i}_cnt": np.int64(cnt)})
    for i, (states, pos) in enumerate(eef_cases(rng)):
        res = ref.process_eef(states.copy(), {"pos": pos, "max_neef": len(pos)})
        out.update({f"eef_{i}_states": states, f"eef_{i}_pos": np.array(pos, np.float64), f"eef_{i}_out": res})
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
