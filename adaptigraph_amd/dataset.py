"""Training / validation samples from the reference's preprocessed dataset layout — SURVEY.md §8f row n4 data side
(src/dynamics/dataset/dataset.py:10-252).

`DynDataset[idx]` yields the same tensors as the reference for the same numpy RNG state (FPS start indices, FPS radius,
physics noise, state noise, rotation, adjacency radius — drawn in that order), except that it does NOT build dense
`Rr`/`Rs` on the host: it returns the masks and the drawn radius, and `attach_edges` builds the whole batch's adjacency on
the GPU (`ag_build_edges`, single-graph rule variant, per-sample radius) after collation.

`DeviceBatcher(dataset, device).batch(indices)` yields `default_collate([dataset[i] for i in indices])` on the device with the same values under the
same `np.random.seed`: the positions stay in HBM, the host only draws the random numbers of the batch (in the order successive `__getitem__` calls
draw them) and uploads them in one pinned copy; the sampling (`ag_fps`, one launch per pass for the whole batch), the gathers, the noise and the
rotation run on the GPU (`ag_gather_clouds`, `ag_assemble_batch`, csrc/ag_batch.hip) without a host synchronisation.
"""
import ctypes

import numpy as np
import torch
from torch.utils.data import Dataset

from .graph import build_edges
from .load import load_dataset, load_positions
from .sampling import _draw_radius, fps, radius_as_compared, two_pass_tensors
from .train_ops import EdgeViews


class DynDataset(Dataset):
    def __init__(self, dataset_config, material_config, phase="train", fps_device=None):
        """`fps_device` (e.g. "cuda:0"): the key-point sampling of every item runs on that GPU (`sampling.fps(..., device=)`: the same indices and
        RNG draws as the host code).  Meant for `DataLoader(num_workers=0)`: a worker process must not inherit an initialised GPU."""
        assert phase in ["train", "valid"]
        self.phase = phase
        self.fps_device = fps_device
        self.dataset_config, self.material_config = dataset_config, material_config
        self.verbose = dataset_config.get("verbose", False)
        self.n_his, self.n_future = dataset_config["n_his"], dataset_config["n_future"]
        rnd = dataset_config["randomness"]
        self.add_randomness = rnd["use"]
        self.state_noise, self.phys_noise = rnd["state_noise"][phase], rnd["phys_noise"][phase]
        assert len(dataset_config["datasets"]) == 1, "Only one object type is supported."
        d = self.dataset = dataset_config["datasets"][0]
        self.max_nobj, self.fps_radius_range = d["max_nobj"], d["fps_radius_range"]
        self.max_nR, self.adj_radius_range = d["max_nR"], d["adj_radius_range"]
        self.topk, self.connect_tool_all = d["topk"], d["connect_tool_all"]
        self.pair_lists, self.physics_params = load_dataset(dataset_config, material_config, phase)
        self.pair_lists = np.array(self.pair_lists)
        self.materials = {k: v.shape[0] for k, v in self.physics_params[0].items()}
        self.eef_pos, self.obj_pos = load_positions(dataset_config)
        self.pos_dim = self.obj_pos[0].shape[-1]
        self.obj_dim, self.eef_dim = self.max_nobj, self.eef_pos[0].shape[1]
        self.state_dim = self.obj_dim + self.eef_dim

    def __len__(self):
        return len(self.pair_lists)

    def __getitem__(self, idx):
        H, Fu, no, ns = self.n_his, self.n_future, self.obj_dim, self.state_dim
        epi = int(self.pair_lists[idx][0])
        pair = self.pair_lists[idx][1:].astype(int)
        assert len(pair) == H + Fu
        obj_kps = np.asarray(self.obj_pos[epi])[pair]            # (H+Fu, N_all, 3)
        eef_kps = np.asarray(self.eef_pos[epi])[pair]            # (H+Fu, N_eef, 3)
        fps_idx = fps(obj_kps[H - 1], self.max_nobj, self.fps_radius_range, verbose=self.verbose, device=self.fps_device)
        n_kp, n_eef = len(fps_idx), eef_kps.shape[1]

        kp = np.zeros((H + Fu, no, self.pos_dim), np.float32)    # sampled key-points of every frame, zero-padded
        kp[:, :n_kp] = obj_kps[:, fps_idx]
        state_history = np.zeros((H, ns, self.pos_dim), np.float32)
        state_history[:, :no], state_history[:, no:] = kp[:H], eef_kps[:H]
        states_delta = np.zeros((ns, self.pos_dim), np.float32)
        states_delta[no:] = eef_kps[H] - eef_kps[H - 1]
        obj_kp_future = kp[H:].copy()
        eef_future = np.zeros((Fu - 1, ns, self.pos_dim), np.float32)
        states_delta_future = np.zeros((Fu - 1, ns, self.pos_dim), np.float32)
        eef_future[:, no:] = eef_kps[H:H + Fu - 1]
        states_delta_future[:, no:] = eef_kps[H + 1:H + Fu] - eef_kps[H:H + Fu - 1]

        state_mask = np.zeros(ns, bool)
        state_mask[:n_kp] = True
        state_mask[no:] = True
        eef_mask = np.zeros(ns, bool)
        eef_mask[no:] = True
        attrs = np.zeros((ns, 2), np.float32)
        attrs[:n_kp, 0] = 1.0
        attrs[no:, 1] = 1.0
        p_instance = np.zeros((no, 1), np.float32)
        p_instance[:n_kp, 0] = 1

        physics_param = self.physics_params[epi]                 # noise accumulates in place, as in the reference (:175-179)
        for m in self.dataset_config["materials"]:
            if m not in physics_param.keys():
                raise ValueError(f"Physics parameter {m} not found in {self.dataset_config['data_dir']}")
            physics_param[m] += np.random.uniform(-self.phys_noise, self.phys_noise, size=physics_param[m].shape)
        assert len(self.dataset_config["materials"]) == 1, "only support single material"
        material_idx = np.zeros((no, len(self.material_config["material_index"])), np.int64)
        material_idx[:n_kp, self.material_config["material_index"][self.dataset_config["materials"][0]]] = 1

        if self.add_randomness:                                   # position noise, then one rotation about the last axis
            state_history += np.random.uniform(-self.state_noise, self.state_noise, size=state_history.shape)   # stays fp32
            ang = np.random.uniform(-np.pi, np.pi)
            rot = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], dtype=state_history.dtype)
            state_history, states_delta = state_history @ rot[None], states_delta @ rot
            eef_future, states_delta_future, obj_kp_future = eef_future @ rot[None], states_delta_future @ rot[None], obj_kp_future @ rot[None]
        adj_thresh = np.random.uniform(*self.adj_radius_range)

        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
        graph = {"state": f32(state_history), "action": f32(states_delta), "eef_future": f32(eef_future),
                 "action_future": f32(states_delta_future), "state_future": f32(obj_kp_future), "attrs": f32(attrs),
                 "p_rigid": torch.zeros(1), "p_instance": f32(p_instance), "obj_mask": torch.from_numpy(np.arange(no) < n_kp),
                 "state_mask": torch.from_numpy(state_mask), "eef_mask": torch.from_numpy(eef_mask),
                 "material_index": torch.from_numpy(material_idx), "adj_thresh": torch.tensor(adj_thresh, dtype=torch.float64)}
        for m, dim in self.materials.items():
            graph[m + "_physics_param"] = f32(physics_param[m]) if m in physics_param else torch.zeros(dim)
        return graph


def attach_edges(data, dataset_config, device):
    """Collated batch (CPU or GPU tensors) -> the same dict on `device` with the adjacency of every sample built there:
    data['Rr'] = CSREdges (and data['Rs'] = None, data['edge_views'] for the training ops)."""
    d = dataset_config["datasets"][0]
    data = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in data.items()}
    radii = data.pop("adj_thresh").double().cpu().numpy().reshape(-1)
    csr = build_edges(data["state"][:, -1].contiguous(), radii, data["state_mask"], data["eef_mask"], d["topk"], d["connect_tool_all"],
                      "single", max_tools=int(data["eef_mask"].shape[1] - d["max_nobj"]))
    data["Rr"], data["Rs"], data["edge_views"] = csr, None, EdgeViews(csr)
    return data


def draw_batch_tables(dataset, indices):
    """Everything the host contributes to the items `indices` of a DynDataset, as numpy tables with one row per item: the episode and frames, and
    every random number, drawn item after item in the order `__getitem__` draws them (start of sampling pass 1, radius if a range, start of pass 2,
    physics noise, state noise, angle, adjacency radius), so np.random ends up exactly where `[dataset[i] for i in indices]` leaves it.  The
    physics noise accumulates in `dataset.physics_params[epi]` in place, as there; `phys_<m>[b]` is the episode's value after the last item of
    the batch, which is what the collated host items hold (their tensors are views of the dataset's arrays).  Needs no GPU."""
    cfg = dataset.dataset_config
    H, Fu, ns, B = dataset.n_his, dataset.n_future, dataset.state_dim, len(indices)
    assert B >= 1
    assert len(cfg["materials"]) == 1, "only support single material"
    t = {"epi": np.zeros(B, np.int32), "frames": np.zeros((B, H + Fu), np.int32), "fps_frame": np.zeros(B, np.int32),
         "k1": np.zeros(B, np.int32), "start1": np.zeros(B, np.int32), "start2": np.zeros(B, np.int32), "radius": np.zeros(B, np.float64),
         "adj_thresh": np.zeros(B, np.float64), "n": np.zeros(B, np.int32)}
    if dataset.add_randomness:
        t["noise"], t["rot"] = np.zeros((B, H, ns, dataset.pos_dim), np.float64), np.zeros((B, 3, 3), np.float32)
    for m, dim in dataset.materials.items():
        t["phys_" + m] = np.zeros((B, dim), np.float32)
    for b, idx in enumerate(indices):
        row = dataset.pair_lists[int(idx)]
        epi = int(row[0])
        assert len(row) == 1 + H + Fu
        n = int(np.shape(dataset.obj_pos[epi])[1])
        t["epi"][b], t["frames"][b], t["fps_frame"][b], t["n"][b], t["k1"][b] = epi, row[1:], row[H], n, min(dataset.max_nobj, n)
        t["start1"][b] = np.random.randint(0, n)
        t["radius"][b] = radius_as_compared(_draw_radius(dataset.fps_radius_range))
        t["start2"][b] = np.random.randint(min(dataset.max_nobj, n))
        physics_param = dataset.physics_params[epi]
        for m in cfg["materials"]:
            if m not in physics_param.keys():
                raise ValueError(f"Physics parameter {m} not found in {cfg['data_dir']}")
            physics_param[m] += np.random.uniform(-dataset.phys_noise, dataset.phys_noise, size=physics_param[m].shape)
        if dataset.add_randomness:
            t["noise"][b] = np.random.uniform(-dataset.state_noise, dataset.state_noise, size=(H, ns, dataset.pos_dim))
            ang = np.random.uniform(-np.pi, np.pi)
            t["rot"][b] = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], dtype=np.float32)
        t["adj_thresh"][b] = np.random.uniform(*dataset.adj_radius_range)
    for b, epi in enumerate(t["epi"]):
        for m in dataset.materials:
            if m in dataset.physics_params[epi]:
                t["phys_" + m][b] = dataset.physics_params[epi][m]
    return t


class DeviceBatcher:
    """Batches of a DynDataset assembled on `device` (see the module docstring).  The dataset's pair lists, physics parameters and config are used
    as they are; its positions are uploaded once: the object positions as fp32 (where the host path casts them too), the tool positions in their
    own dtype (the actions are differences taken in that dtype, rounded afterwards).  Episodes may differ in frames and points.
    `max_bytes`: the most the resident stores may take; default FREE_FRACTION of the device memory free at construction.  Larger stores raise
    ValueError: there is no fall-back to the host path."""
    FREE_FRACTION = 0.5
    _TABLES = ("epi", "frames", "fps_frame", "k1", "start1", "start2", "radius", "noise", "rot")

    def __init__(self, dataset, device, max_bytes=None):
        self.dataset, self.device = dataset, torch.device(device)
        assert dataset.pos_dim == 3
        obj = [np.asarray(a) for a in dataset.obj_pos]
        eef = [np.asarray(a) for a in dataset.eef_pos]
        tool_dtype = eef[0].dtype
        if tool_dtype not in (np.float32, np.float64) or any(a.dtype != tool_dtype for a in eef):
            raise TypeError(f"DeviceBatcher: tool positions must be all float32 or all float64, got {sorted({str(a.dtype) for a in eef})}")
        table, obj_off, tool_off = np.zeros((len(obj), 4), np.int64), 0, 0
        for e, (o, t) in enumerate(zip(obj, eef)):
            if o.ndim != 3 or t.shape != (o.shape[0], dataset.eef_dim, 3) or o.shape[2] != 3 or o.shape[1] < 1:
                raise ValueError(f"DeviceBatcher: episode {e} has object positions {o.shape} and tool positions {t.shape}")
            table[e] = obj_off, tool_off, o.shape[0], o.shape[1]
            obj_off, tool_off = obj_off + o.shape[0] * o.shape[1], tool_off + t.shape[0] * t.shape[1]
        pairs = dataset.pair_lists
        if len(pairs) and not ((pairs[:, 1:] >= 0).all() and (pairs[:, 1:] < table[pairs[:, 0], 2][:, None]).all()):
            raise ValueError("DeviceBatcher: a frame pair names a frame its episode does not have")
        self.store_bytes = obj_off * 3 * 4 + tool_off * 3 * tool_dtype.itemsize + table.nbytes
        if max_bytes is None:
            max_bytes = int(self.FREE_FRACTION * torch.cuda.mem_get_info(self.device)[0])
        if self.store_bytes > max_bytes:
            raise ValueError(f"DeviceBatcher: the resident position stores need {self.store_bytes} bytes, more than the {max_bytes} allowed "
                             f"(max_bytes); use the host loader for this dataset")
        if self.device.type != "cuda":
            raise RuntimeError(f"adaptigraph_amd: DeviceBatcher needs an MI355X (got {self.device}); the engine has no CPU path")
        up = lambda arrays, dt: torch.from_numpy(np.concatenate([a.astype(dt, copy=False).reshape(-1) for a in arrays])).to(self.device)
        self.obj_store, self.tool_store, self.episodes = up(obj, np.float32), up(eef, tool_dtype), torch.from_numpy(table).to(self.device)
        mats = dataset.material_config["material_index"]
        self.n_mat, self.mat_col = len(mats), int(mats[dataset.dataset_config["materials"][0]])
        self.tool_f64 = int(tool_dtype == np.float64)

    def draw(self, indices):
        return draw_batch_tables(self.dataset, [int(i) for i in indices])

    def upload(self, tables):
        """The host tables of one batch -> device tensors, through ONE pinned buffer and one asynchronous copy."""
        items = [(k, np.ascontiguousarray(v)) for k, v in tables.items() if k in self._TABLES or k.startswith("phys_")]
        offs, total = [], 0
        for _k, v in items:
            offs.append(total)
            total += (v.nbytes + 15) // 16 * 16
        pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        host = pinned.numpy()
        for (_k, v), off in zip(items, offs):
            host[off:off + v.nbytes] = v.reshape(-1).view(np.uint8)
        buf = pinned.to(self.device, non_blocking=True)
        return {k: buf[off:off + v.nbytes].view(getattr(torch, v.dtype.name)).view(v.shape) for (k, v), off in zip(items, offs)}

    def assemble(self, dev, n_max, K):
        """Device tables (`upload`) -> the batch, enqueued on the current stream: ag_gather_clouds, both sampling passes, ag_assemble_batch.
        n_max / K: the largest cloud and the largest min(max_nobj, cloud size) of the batch.  No host synchronisation (safe under capture)."""
        from . import _lib
        d = self.dataset
        H, Fu, no, ns, B = d.n_his, d.n_future, d.obj_dim, d.state_dim, int(dev["epi"].shape[0])
        device = self.device
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        mask = lambda *shape: torch.empty(shape, dtype=torch.bool, device=device)
        pts, count = f32(B, n_max, 3), torch.empty(B, dtype=torch.int32, device=device)
        _lib.call("ag_gather_clouds", device, self.obj_store, self.episodes, int(self.episodes.shape[0]), dev["epi"], dev["fps_frame"], B, int(n_max),
                  pts, count)
        with torch.cuda.device(device):
            picks = two_pass_tensors(pts, count, dev["k1"], dev["start1"], dev["start2"], dev["radius"], int(K)).contiguous()
            out = {"state": f32(B, H, ns, 3), "action": f32(B, ns, 3), "eef_future": f32(B, Fu - 1, ns, 3), "action_future": f32(B, Fu - 1, ns, 3),
                   "state_future": f32(B, Fu, no, 3), "attrs": f32(B, ns, 2), "p_rigid": torch.zeros((B, 1), dtype=torch.float32, device=device),
                   "p_instance": f32(B, no, 1), "obj_mask": mask(B, no), "state_mask": mask(B, ns), "eef_mask": mask(B, ns),
                   "material_index": torch.empty((B, no, self.n_mat), dtype=torch.int64, device=device)}
        dims = _lib.BatchDims(B, H, Fu, no, ns - no, int(K), self.n_mat, self.mat_col, int(self.episodes.shape[0]), self.tool_f64)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        outs = _lib.BatchOut(*[ptr(out[k]) for k, _ in _lib.BatchOut._fields_])
        _lib.call("ag_assemble_batch", device, ctypes.byref(dims), self.obj_store, self.tool_store, self.episodes, dev["epi"], dev["frames"], picks,
                  ptr(dev.get("noise")), ptr(dev.get("rot")), ctypes.byref(outs))
        for m in d.materials:
            out[m + "_physics_param"] = dev["phys_" + m]
        return out

    def batch(self, indices):
        """-> what `default_collate([dataset[i] for i in indices])` holds, on the device; `adj_thresh` stays on the host (float64), where
        `attach_edges` reads it."""
        t = self.draw(indices)
        out = self.assemble(self.upload(t), int(t["n"].max()), int(t["k1"].max()))
        out["adj_thresh"] = torch.from_numpy(t["adj_thresh"])
        keys = list(out)                                   # the host item's key order: adj_thresh in front of the physics parameters
        keys.insert(keys.index("material_index") + 1, keys.pop())
        return {k: out[k] for k in keys}
