"""From raw trajectories to the preprocessed layout `load.py` reads: the tool key points of every frame and the frame tuples of a push
(src/dynamics/preprocess/preprocess.py:22-49, 71-133).  Host code with the reference's signatures and return values, pinned to results of the
reference's own functions (tests/golden/preprocess_pairs.npz, made by tools/gen_preprocess_golden.py).
"""
import numpy as np


def _rotations(quat):
    """(T, 4) quaternions (x, y, z, w) -> (T, 3, 3) rotation matrices, in the quaternions' dtype."""
    q1, q2, q3, w = quat[:, 0], quat[:, 1], quat[:, 2], quat[:, 3]
    rows = [[1 - 2 * (q2 ** 2 + q3 ** 2), 2 * (q1 * q2 - q3 * w), 2 * (q1 * q3 + q2 * w)],
            [2 * (q1 * q2 + q3 * w), 1 - 2 * (q1 ** 2 + q3 ** 2), 2 * (q2 * q3 - q1 * w)],
            [2 * (q1 * q3 - q2 * w), 2 * (q2 * q3 + q1 * w), 1 - 2 * (q1 ** 2 + q2 ** 2)]]
    return np.stack([np.stack(r, axis=1) for r in rows], axis=1)


def process_eef(eef_states, eef_dataset):
    """eef_states (T, N, 14) — or (T, 14) for one tool body — rows of position (0:3), ..., quaternion x, y, z, w (6:10); eef_dataset = the
    dataset_config['eef'] dict: 'pos' the key points in the tool's frame, 'max_neef' their number.  -> (T, max_neef, 3) float64: key point j =
    position + R(quaternion) pos[j] of body j, of the LAST body when there are fewer bodies than key points (the granular tool)."""
    T = eef_states.shape[0]
    if eef_states.ndim == 2:
        eef_states = eef_states.reshape(T, 1, 14)
    pos = eef_dataset["pos"]
    assert len(pos) == eef_dataset["max_neef"], "Number of eef not match."
    out = np.zeros((T, eef_dataset["max_neef"], 3))
    for j in range(len(pos)):
        body = eef_states[:, min(j, eef_states.shape[1] - 1)]
        rot = _rotations(body[:, 6:10])
        for i in range(T):      # np.dot per frame: the matrix-vector product of the reference, whatever order its BLAS sums in
            out[i, j] = body[i, 0:3] + np.dot(rot[i], pos[j])
    return out


def extract_push(eef, dist_thresh, n_his, n_future, n_frames):
    """eef (T, N, 3) tool key points of one push (key point 0 is used, its x and z).  -> (frame_idxs (T, n_his + n_future) int, T): row f holds
    n_his history frames ending in f and n_future future frames, each chosen greedily: walking away from f, the next frame at least dist_thresh
    from the last chosen one; a side that runs out of frames repeats its last frame.  n_frames (the episode's frames before this push) is
    added to every index."""
    T = eef.shape[0]
    xz = eef[:, 0][:, [0, 2]]
    dist = np.sqrt((xz[:, None, 0] - xz[None, :, 0]) ** 2 + (xz[:, None, 1] - xz[None, :, 1]) ** 2)      # (T, T), in eef's dtype
    rows = np.zeros((T, n_his + n_future), np.int64)
    for f in range(T):
        for lo, length, order in ((0, n_his, range(f, -1, -1)), (n_his, n_his + n_future, range(f, T))):
            picked = [f] if lo == 0 else list(rows[f, :n_his])      # (the history in its final order: it ends in f)
            cur = f
            for fi in order:
                if dist[cur, fi] >= dist_thresh:
                    picked.append(fi)
                    cur = fi
                if len(picked) == length:
                    break
            picked = picked + [picked[-1]] * (length - len(picked))
            if lo == 0:
                rows[f, :n_his] = picked[::-1]
            else:
                rows[f, n_his:] = picked[n_his:]
    return rows + n_frames, T
