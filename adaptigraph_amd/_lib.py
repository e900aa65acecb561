"""ctypes binding of libadaptigraph_hip.so (C ABI in include/adaptigraph_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or fails to load, importing
anything that computes raises immediately.
"""
import ctypes
import os
import subprocess

# torch (and with it torch's bundled libamdhip64.so.7) is loaded BEFORE the library: device pointers, streams and events are
# shared with torch, so both must sit on ONE HIP runtime instance; the loader then binds our DT_NEEDED
# libamdhip64.so.7 to the already-loaded copy.  (Loaded the other way round, torch finds no device.)
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AG_LIB_PATH") or os.path.join(_HERE, "libadaptigraph_hip.so")   # override: kernel A/B builds
CSRC = os.path.join(_HERE, "csrc")

KERNEL_CLASSES = ("build_edges", "node_encode", "edge_encode", "aggregate", "node_update", "rollout_step")

AG_VARIANT_SINGLE, AG_VARIANT_BATCH = 0, 1
AG_HEIGHT_MIN, AG_HEIGHT_MASKED_MEAN = 0, 1
AG_RAGGED_MAX_STEPS = 1024
AG_STATUS_NONFINITE, AG_STATUS_ORDER = 1, 4
AG_PENALTIES = {None: 0, "rope": 1, "cloth": 2, "granular": 3}      # AG_PENALTY_*
AG_ERROR_GIVEN, AG_ERROR_BOX = 0, 1
AG_PLAN_TERMS = 9
AG_EMD_MAX_POINTS = 1024

c_void_p, c_char_p, c_int, c_int32, c_int64, c_size_t, c_float, c_double, P = (
    ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float, ctypes.c_double,
    ctypes.POINTER)


class ModelConfig(ctypes.Structure):
    _fields_ = [("nf", ctypes.c_int32), ("n_his", ctypes.c_int32), ("attr_dim", ctypes.c_int32),
                ("phys_dim", ctypes.c_int32), ("action_dim", ctypes.c_int32), ("pstep", ctypes.c_int32),
                ("motion_clamp", ctypes.c_float)]


class BatchDims(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "H", "Fu", "no", "n_eef", "K", "n_mat", "mat_col", "n_episodes", "tool_f64")]


class BatchOut(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("state", "action", "eef_future", "action_future", "state_future", "attrs", "p_instance", "obj_mask",
                                               "state_mask", "eef_mask", "material_index")]


class RolloutParams(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("N", ctypes.c_int32), ("n_p", ctypes.c_int32), ("n_instance", ctypes.c_int32),
                ("topk", ctypes.c_int32), ("connect_tools_all", ctypes.c_int32), ("max_tools", ctypes.c_int32),
                ("n_steps", ctypes.c_int32), ("height_mode", ctypes.c_int32), ("gripper_raise", ctypes.c_float)]


class ScriptedParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "N", "n_p", "n_instance", "topk", "connect_tools_all", "max_tools", "variant", "n_steps")]


class PlanCostParams(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("L", ctypes.c_int32), ("n", ctypes.c_int32), ("penalty", ctypes.c_int32), ("criterion", ctypes.c_int32),
                ("sim_real_ratio", ctypes.c_float), ("bbox", ctypes.c_float * 4), ("box", ctypes.c_float * 4)]


class MppiParams(ctypes.Structure):
    _fields_ = [("n_chunk", ctypes.c_int32), ("S", ctypes.c_int32), ("L", ctypes.c_int32), ("reward_weight", ctypes.c_float),
                ("push_length", ctypes.c_float), ("lo", ctypes.c_float * 4), ("hi", ctypes.c_float * 4)]


# The C ABI, one row per export in the order and the groups of include/adaptigraph_hip.h: name -> (restype, [argtypes]).
# Device pointers, model handles and streams are c_void_p; HOST arrays and structs are typed pointers.
# tests/test_abi.py holds every row to the header's prototype, position by position.
SIGNATURES = {
    "ag_last_error": (c_char_p, []),
    "ag_version": (c_int, []),
    # model
    "ag_model_create": (c_int, [P(ModelConfig), P(c_void_p), P(c_void_p)]),
    "ag_model_update_weights": (c_int, [c_void_p, P(c_void_p)]),
    "ag_model_destroy": (c_int, [c_void_p]),
    "ag_set_option": (c_int, [c_void_p, c_char_p, c_int]),
    "ag_get_option": (c_int, [c_void_p, c_char_p, P(c_int)]),
    "ag_model_status": (c_int, [c_void_p, P(c_int), c_void_p]),
    # edges
    "ag_edge_capacity": (c_int64, [c_int] * 5),
    "ag_edges_workspace_bytes": (c_size_t, [c_int] * 5),
    "ag_build_edges": (c_int, [c_void_p] * 4 + [c_int] * 6 + [c_void_p] * 3 + [c_int64, c_void_p, c_size_t, c_void_p]),
    # dense Rr / Rs <-> CSR
    "ag_dense_edges_workspace_bytes": (c_size_t, [c_int] * 3),
    "ag_edges_from_dense": (c_int, [c_void_p] * 2 + [c_int] * 3 + [c_void_p] * 4 + [c_size_t, c_void_p]),
    "ag_edges_to_dense": (c_int, [c_void_p] * 3 + [c_int] * 3 + [c_void_p] * 4),
    # forward
    "ag_forward_workspace_bytes": (c_size_t, [c_int, c_int, c_int64]),
    "ag_forward_workspace_bytes_for": (c_size_t, [c_void_p, c_int, c_int, c_int64]),
    "ag_forward": (c_int, [c_void_p] * 5 + [c_int] + [c_void_p] * 4 + [c_int64] + [c_int] * 3 + [c_void_p] * 3 + [c_size_t, c_void_p]),
    # rollout
    "ag_rollout_workspace_bytes": (c_size_t, [P(RolloutParams)]),
    "ag_rollout_workspace_bytes_for": (c_size_t, [c_void_p, P(RolloutParams)]),
    "ag_rollout_streams_for": (c_int, [c_void_p, P(RolloutParams)]),
    "ag_rollout": (c_int, [c_void_p, P(RolloutParams)] + [c_void_p] * 13 + [c_size_t, c_void_p]),
    # scripted rollout
    "ag_rollout_scripted_workspace_bytes_for": (c_size_t, [c_void_p, P(ScriptedParams)]),
    "ag_rollout_scripted": (c_int, [c_void_p, P(ScriptedParams)] + [c_void_p] * 16 + [c_size_t, c_void_p]),
    # ragged rollout
    "ag_rollout_order": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "ag_rollout_ragged": (c_int, [c_void_p, P(RolloutParams)] + [c_void_p] * 10 + [P(c_int32)] + [c_void_p] * 4 + [c_size_t, c_void_p]),
    # chamfer, both clouds resident in LDS
    "ag_chamfer": (c_int, [c_void_p] * 2 + [c_int] * 4 + [c_void_p] * 2),
    "ag_chamfer_masked": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 2),
    "ag_chamfer_fwd_idx": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 4),
    "ag_chamfer_backward": (c_int, [c_void_p] * 7 + [c_int] * 4 + [c_void_p] * 3),
    # chamfer, tiled: clouds of any size
    "ag_chamfer_tile_sizes": (None, [P(c_int), P(c_int)]),
    "ag_chamfer_tiled_workspace_bytes": (c_size_t, [c_int] * 3),
    "ag_chamfer_tiled": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 4 + [c_size_t, c_void_p]),
    "ag_chamfer_tiled_backward": (c_int, [c_void_p] * 7 + [c_int] * 4 + [c_void_p] * 3),
    # matching losses: earth-mover assignment, its backward, directed Hausdorff maxima
    "ag_emd": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 4),
    "ag_emd_backward": (c_int, [c_void_p] * 5 + [c_int] * 4 + [c_void_p] * 3),
    "ag_hausdorff": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 3),
    # the planner's trajectory cost
    "ag_plan_cost_workspace_bytes": (c_size_t, [P(PlanCostParams)]),
    "ag_plan_cost": (c_int, [P(PlanCostParams)] + [c_void_p] * 7 + [c_size_t, c_void_p]),
    # a planning step's chunks in one pass
    "ag_plan_cost_chunked": (c_int, [P(PlanCostParams), c_int] + [c_void_p] * 7 + [c_size_t, c_void_p]),
    "ag_mppi_update": (c_int, [P(MppiParams)] + [c_void_p] * 7),
    # farthest-point sampling
    "ag_fps_workspace_bytes": (c_size_t, [c_int] * 2),
    "ag_fps": (c_int, [c_void_p] * 3 + [c_int] * 4 + [c_void_p] * 4 + [c_size_t, c_void_p]),
    # the tabletop cloud from depth images
    "ag_tabletop_workspace_bytes": (c_size_t, [c_int]),
    "ag_depth_cloud": (c_int, [c_void_p] * 4 + [c_int] * 4 + [c_void_p] * 3 + [c_size_t, c_void_p]),
    "ag_cloud_voxel_keys": (c_int, [c_void_p] * 2 + [c_int, P(c_double)] + [c_void_p] * 3 + [c_size_t, c_void_p]),
    "ag_cloud_voxel_merge": (c_int, [c_void_p] * 2 + [c_int] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    "ag_cloud_knn_mean": (c_int, [c_void_p] * 2 + [c_int] * 2 + [c_void_p] * 3 + [c_size_t, c_void_p]),
    "ag_cloud_outlier_filter": (c_int, [c_void_p] * 2 + [c_int, c_void_p, P(c_double)] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    "ag_cloud_select": (c_int, [c_void_p] * 2 + [c_int] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    # rope push simulator
    "ag_sim_rope_push": (c_int, [c_void_p] * 12 + [c_int] * 7 + [c_float] * 6 + [c_void_p]),
    # granular push simulator
    "ag_sim_pile_push": (c_int, [c_void_p] * 11 + [c_int] * 8 + [c_float] * 9 + [c_void_p]),
    # cloth grasp-and-drag simulator
    "ag_sim_cloth_push": (c_int, [c_void_p] * 14 + [c_int] * 8 + [c_float] * 8 + [c_void_p]),
    # box push simulator
    "ag_sim_box_push": (c_int, [c_void_p] * 13 + [c_int] * 8 + [c_float] * 9 + [c_void_p]),
    # simulated depth cameras
    "ag_render_depth": (c_int, [c_void_p] * 6 + [c_int] * 5 + [c_void_p] * 3),
    # rollout and planning records drawn as images
    "ag_draw_scratch_bytes": (c_size_t, [c_int] * 2),
    "ag_draw": (c_int, [c_void_p, c_int] * 4 + [c_void_p, c_int, P(c_double)] + [c_int] * 4 + [c_void_p, c_int] * 2 + [c_int] * 2
                + [c_void_p, c_size_t, c_void_p, c_void_p]),
    # records as baseline JPEG scans
    "ag_jpeg_scratch_bytes": (c_size_t, [c_int] * 5),
    "ag_jpeg_out_bytes": (c_size_t, [c_int] * 5),
    "ag_jpeg_encode": (c_int, [c_void_p] + [c_int] * 7 + [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p]),
    # object masks from colour images
    "ag_segment_tile_sizes": (None, [P(c_int), P(c_int)]),
    "ag_segment_scratch_bytes": (c_size_t, [c_int] * 3),
    "ag_segment_color_mask": (c_int, [c_void_p] + [c_int] * 4 + [P(c_int32), c_int, c_void_p, c_void_p]),
    "ag_segment_morph": (c_int, [c_void_p] + [c_int] * 5 + [c_void_p, c_size_t, c_void_p, c_void_p]),
    "ag_segment_label": (c_int, [c_void_p] + [c_int] * 4 + [c_void_p, c_size_t] + [c_void_p] * 3),
    "ag_segment_components": (c_int, [c_void_p] * 2 + [c_int] * 4 + [c_void_p] * 2),
    "ag_segment_select": (c_int, [c_void_p] + [c_int] * 6 + [c_void_p, c_size_t, c_void_p, c_void_p]),
    "ag_segment_fill_holes": (c_int, [c_void_p] + [c_int] * 4 + [c_void_p, c_size_t, c_void_p, c_void_p]),
    "ag_segment_keep": (c_int, [c_void_p] * 2 + [c_int] * 3 + [c_void_p] * 2),
    # training batches assembled on the device
    "ag_gather_clouds": (c_int, [c_void_p] * 2 + [c_int] + [c_void_p] * 2 + [c_int] * 2 + [c_void_p] * 3),
    "ag_assemble_batch": (c_int, [P(BatchDims)] + [c_void_p] * 8 + [P(BatchOut), c_void_p]),
    # training path: graph pieces
    "ag_gather_rows": (c_int, [c_void_p] * 3 + [c_int64, c_int, c_void_p]),
    "ag_segment_sum": (c_int, [c_void_p] * 4 + [c_int64, c_int, c_void_p]),
    "ag_message_forward": (c_int, [c_void_p] * 6 + [c_int64, c_int, c_void_p]),
    "ag_message_backward": (c_int, [c_void_p] * 8 + [c_int64, c_int, c_void_p]),
    "ag_edge_views_workspace_bytes": (c_size_t, [c_int] * 2),
    "ag_edge_views": (c_int, [c_void_p] * 2 + [c_int] * 2 + [c_void_p] * 4),
    "ag_step_update_forward": (c_int, [c_void_p] * 6 + [c_int] * 6 + [c_float] + [c_void_p] * 3),
    "ag_step_update_backward": (c_int, [c_void_p] * 3 + [c_int] * 6 + [c_void_p] * 7),
    # training path: dense stacks
    "ag_train_pack": (c_int, [c_void_p] * 2 + [c_int] * 8 + [c_void_p] * 2),
    "ag_train_chain": (c_int, [c_int] * 3 + [c_void_p] * 2 + [P(c_void_p), c_void_p, P(c_void_p), c_void_p, c_int64, c_int, c_void_p]),
    "ag_edge_inputs_forward": (c_int, [c_void_p] + [c_int] * 3 + [c_void_p] * 3 + [c_int64, c_void_p]),
    "ag_edge_inputs_backward": (c_int, [c_void_p] + [c_int] * 3 + [c_void_p] * 9 + [c_int64, c_int64, c_void_p]),
    "ag_add3_relu": (c_int, [c_void_p] * 4 + [c_int64, c_void_p]),
    "ag_relu_mask": (c_int, [c_void_p] * 3 + [c_int64, c_void_p]),
    "ag_train_weight_grads_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "ag_train_weight_grads": (c_int, [c_int, P(c_void_p), P(c_int32), P(c_void_p), P(c_int32), P(c_int32), c_int64, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "ag_train_weight_grads_into": (c_int, [c_int, P(c_void_p), P(c_int32), P(c_void_p), P(c_int32), P(c_int32), c_int64, c_void_p,
                                           P(c_void_p), P(c_int32), P(c_void_p), P(c_int32), c_void_p, c_size_t, c_void_p]),
    # per-kernel timing
    "ag_profile_enable": (c_int, [c_void_p, c_int]),
    "ag_profile_read": (c_int, [c_void_p, P(c_double), P(c_int64), P(c_int64)]),
}
EXPORTS = tuple(SIGNATURES)


def build(force=False):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h")) or f in ("Makefile", "exports.map")]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "adaptigraph_hip.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-j8"] + (["-B"] if force else []), stdout=subprocess.DEVNULL)
    return LIB_PATH


_LIB = None


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"adaptigraph_amd: {LIB_PATH} is missing. The engine has no CPU fallback; build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc, no GPU required).")
    L = ctypes.CDLL(LIB_PATH)           # (torch is loaded by now: see the import at the top)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is None:
            raise RuntimeError(f"adaptigraph_amd: {LIB_PATH} does not export {name} (stale build?)")
        fn.restype, fn.argtypes = restype, argtypes
    _LIB = L
    return L


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib().ag_last_error().decode()}")


# ---------------------------------------------------------------------------------------------------------------------
# Calling a stream-taking entry point with torch tensors
# ---------------------------------------------------------------------------------------------------------------------
def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def call(name, device, *args):
    """`name(*args, stream)` for an int-returning entry point whose last parameter is the stream: with `device` current, on that device's
    current stream, every torch.Tensor passed as its data_ptr() and None as a null pointer (ints, ctypes arrays, byref(...) and pointer
    arithmetic as they are); a non-zero return code raises with the library's message.  Nothing else: no synchronisation, no allocation,
    no .contiguous() or dtype conversion, which stay with the caller.  `name` may carry a note for the message in parentheses
    ("ag_train_chain(forward)").  Entry points without a stream are called directly: check(lib().ag_x(...), "ag_x")."""
    fn = _ENTRY.get(name) or _entry(name)
    Tensor = torch.Tensor
    ptrs = [a.data_ptr() if isinstance(a, Tensor) else a for a in args]
    if device.index == torch.cuda.current_device():      # already current: the context below would set and restore this same device
        rc = fn(*ptrs, _stream_ptr(device))
    else:
        with torch.cuda.device(device):
            rc = fn(*ptrs, _stream_ptr(device))
    if rc:
        check(rc, name)


_ENTRY = {}     # name as given to call() -> bound function: the training step is host-bound at several hundred of these calls


def _entry(name):
    fn = _ENTRY[name] = getattr(lib(), name.partition("(")[0])
    return fn


_WS = {}


def workspace(device, nbytes):
    """Grow-only scratch buffer handed to the C ABI (the library never allocates scratch), one per (device, stream):
    calls enqueued on different streams may overlap, so they must not share scratch."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def _require_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"adaptigraph_amd: `{name}` must live on an MI355X (got {t.device}); "
                           "the engine has no CPU path")


def _u8(t, device=None):
    """A bool / integer mask as the uint8 tensor the kernels read, on `device` when given: a view of the contiguous bool, otherwise a copy."""
    if t.dtype == torch.bool:
        return t.to(device=device).contiguous().view(torch.uint8)
    return t.to(device=device, dtype=torch.uint8).contiguous()
