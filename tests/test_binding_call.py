"""_lib.call, the one way the Python side calls a stream-taking entry point: tensors go as their pointers and None as null, the device
is made current, the device's current stream is appended, and a non-zero return code raises with the entry point's name and the library's
message.  Integer-valued data: every sum is exact, so the comparisons are torch.equal."""
import pytest
import torch

from adaptigraph_amd import _lib, graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _abc(dev, n=8):
    g = torch.Generator(device=dev).manual_seed(3)
    return [torch.randint(-9, 10, (n,), generator=g, device=dev).float() for _ in range(3)]


def test_call_runs_the_kernel_and_raises_the_library_message():
    a, b, c = _abc(DEV)
    y = torch.full_like(a, -1.0)
    assert _lib.call("ag_add3_relu", DEV, a, b, c, y, 8) is None
    assert torch.equal(y, torch.relu((a + b) + c))
    with pytest.raises(RuntimeError) as e:
        _lib.call("ag_add3_relu", DEV, a, b, c, y, 6)
    assert "ag_add3_relu failed (-1)" in str(e.value) and "multiple of 4" in str(e.value)


def test_call_passes_none_as_a_null_pointer_and_a_tensor_as_its_pointer():
    g = torch.Generator(device=DEV).manual_seed(4)
    vals = torch.randint(-9, 10, (7, 4), generator=g, device=DEV).float()
    ptr = torch.tensor([0, 2, 2, 7], dtype=torch.int32, device=DEV)          # 3 segments, the middle one empty
    seg = lambda v: torch.stack([v[0:2].sum(0), v[2:2].sum(0), v[2:7].sum(0)])
    out = torch.full((3, 4), -1.0, device=DEV)
    _lib.call("ag_segment_sum", DEV, vals, ptr, None, out, 3, 4)
    assert torch.equal(out, seg(vals))
    perm = torch.tensor([6, 0, 3, 5, 1, 2, 4], dtype=torch.int32, device=DEV)
    out.fill_(-1.0)
    _lib.call("ag_segment_sum", DEV, vals, ptr, perm, out, 3, 4)
    assert torch.equal(out, seg(vals[perm.long()])) and not torch.equal(out, seg(vals))


def test_call_and_workspace_follow_the_current_stream():
    """Inputs made on a side stream and the call on it: correct after that stream alone is synchronised, and the scratch buffer is the
    side stream's own."""
    default_ws = graph.workspace(DEV, 1024)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        a, b, c = _abc(DEV, 4096)
        y = torch.empty_like(a)
        _lib.call("ag_add3_relu", DEV, a, b, c, y, a.numel())
        ws = graph.workspace(DEV, 1024)
        assert _lib._stream_ptr(DEV).value == s.cuda_stream
        ref = torch.relu((a + b) + c)
    s.synchronize()
    assert torch.equal(y, ref)
    assert ws.data_ptr() != default_ws.data_ptr() and ws is graph._WS[(DEV.type, DEV.index, s.cuda_stream)]
    assert graph._WS is _lib._WS and graph.workspace is _lib.workspace


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs")
def test_call_makes_the_tensors_device_current():
    other = torch.device("cuda:1")
    a, b, c = _abc(other)
    y = torch.empty_like(a)
    with torch.cuda.device(0):
        _lib.call("ag_add3_relu", other, a, b, c, y, 8)
        assert torch.cuda.current_device() == 0
    assert torch.equal(y, torch.relu((a + b) + c))
