"""What more than one simulator uses: the push schedule (steps, frames), the lateral unit vector of a board or gripper, the ordered sum and the
2^22 fixed-point scale of the host statements, the argument checks every `*_push` shares, and `DeviceCall`, the base of the four device calls.
`SimParams` lives here because `push_steps` and `frames_of` default to it; it is the rope's (rope.py)."""
import dataclasses

import numpy as np

F32 = np.float32


@dataclasses.dataclass(frozen=True)
class SimParams:
    dt: float = 1.0 / 60.0
    substeps: int = 8
    g: float = 9.8
    r: float = 0.03            # particle radius
    R: float = 0.05            # pusher radius
    mu: float = 0.1            # the reference scene's dynamicFriction (scenes.py:33)
    speed: float = 0.01        # pusher advance per step
    record_every: int = 10
    settle: int = 120
    lift: float = 0.2

    @property
    def h(self):
        return F32(self.dt / self.substeps)


DEFAULT = SimParams()


def push_steps(push, params=DEFAULT):
    """push (E, 4) float32 xs, zs, xe, ze -> (n_push (E) int32, inv (E) float32): the steps of every push and 1 / its substeps."""
    p = np.asarray(push, F32).astype(np.float64).reshape(-1, 4)
    length = np.sqrt((p[:, 2] - p[:, 0]) ** 2 + (p[:, 3] - p[:, 1]) ** 2)
    n_push = (length / float(params.speed)).astype(np.int64) + 1
    return n_push.astype(np.int32), (1.0 / (n_push * params.substeps)).astype(F32)


def frames_of(n_push, params=DEFAULT):
    """Frames a push of n_push steps records: steps 0, record_every, ... < n_push and the frame after the settle."""
    return (np.asarray(n_push) - 1) // params.record_every + 2


def _ordered_sum(a):
    """Sum over the last axis in index order, starting with the first term (np.sum adds pairwise; a running sum does not)."""
    return np.cumsum(a, axis=-1)[..., -1]


_Q22, _IQ22 = F32(4194304.0), F32(1.0 / 4194304.0)


def board_lateral(push):
    """push (E, 4) float32 -> (E, 2) float32: the unit vector along the board, the push direction turned by a quarter turn (float64, rounded once)."""
    p = np.asarray(push, F32).astype(np.float64).reshape(-1, 4)
    dx, dz = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    length = np.sqrt(dx * dx + dz * dz)
    ok = length > 0
    safe = np.where(ok, length, 1.0)
    return np.stack([np.where(ok, -dz / safe, 0.0), np.where(ok, dx / safe, 1.0)], 1).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# The argument checks every model's _check and _validate share
# ---------------------------------------------------------------------------------------------------------------------
def _as_push(push):
    return np.ascontiguousarray(push, F32).reshape(-1, 4)


def _xv_ok(scene):
    """x and v of shape (E, n_max, 3)."""
    return scene.x.shape == scene.v.shape and scene.x.shape[0] == scene.E and scene.x.shape[2] == 3


def _f_max(total, f_max, params):
    """The frames a call holds: `f_max`, or those of the longest of the pushes of `total` (E) steps."""
    return int(frames_of(total, params).max()) if f_max is None else int(f_max)


def _check_frames(who, noun, total, F, params):
    need = int(frames_of(total, params).max())
    if F < need:
        raise ValueError(f"{who}: f_max = {F} frames, the longest {noun} writes {need}")


# ---------------------------------------------------------------------------------------------------------------------
# The device path
# ---------------------------------------------------------------------------------------------------------------------
class DeviceCall:
    """The arguments of one ag_sim_*_push call as device tensors.  `launch()` enqueues the kernel on the current stream (no synchronisation, no
    allocation: it captures into a HIP graph), reading and writing the tensors named by `state` in place and writing obj (E, F, n_max, 3),
    eef (E, F, *tool_shape) and n_frames (E); it returns the tensors named by `results`.  The arguments go to the library as given: what it
    refuses comes back as its argument error (RuntimeError), and an episode outside the kernel's bounds gets n_frames = 0 with nothing else
    written.  `validate()` refuses what the model's host statement refuses, with its messages; the `*_push` functions and SimEnv call it first.

    A model's call names its C entry (`entry`), the attributes that are its pointer arguments in the entry's order (`pointers`), what `launch`
    returns (`results`), and hands its arrays and float scalars to __init__; `dims` and `floats` are the entry's integer and float scalars, in
    its order, read at every launch."""
    entry = pointers = results = _validate = None
    tool_shape = (3,)
    state = ("x", "v")

    def __init__(self, scene, params, device, total, F, n_max, ints, floats, scalars):
        """total (E) the steps of every episode's push; ints / floats {attribute: host array} uploaded as int32 / float32; scalars the float
        arguments.  The integer arguments are E, n_max, F, the most steps, substeps, iters (if the model has them), record_every, settle."""
        import torch
        self.device = torch.device(device)
        self._refusable = (scene, total, F, params)
        for name, a in ints.items():
            setattr(self, name, self.up(a, np.int32))
        for name, a in floats.items():
            setattr(self, name, self.up(a, F32))
        for name in self.state:
            t = getattr(scene, name)
            setattr(self, name, t.to(self.device).contiguous().clone() if isinstance(t, torch.Tensor) else self.up(t, F32))
        E = scene.E
        self.obj = torch.zeros((E, F, n_max, 3), dtype=torch.float32, device=self.device)
        self.eef = torch.zeros((E, F, *self.tool_shape), dtype=torch.float32, device=self.device)
        self.n_frames = torch.zeros(E, dtype=torch.int32, device=self.device)
        iters = (int(params.iters),) if hasattr(params, "iters") else ()
        self.dims = (E, n_max, F, int(total.max()), int(params.substeps), *iters, int(params.record_every), int(params.settle))
        self.floats = tuple(float(F32(c)) for c in scalars)

    def up(self, a, dtype):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.device)

    def validate(self):
        self._validate(*self._refusable)
        return self

    def launch(self):
        from .. import _lib
        _lib.call(self.entry, self.device, *(getattr(self, p) for p in self.pointers), *self.dims, *self.floats)
        return tuple(getattr(self, r) for r in self.results)
