"""kasportsformer_amd/_args.py on a box with a GPU: where ``resolve_device`` sends a call (tests/test_args_cpu.py covers what needs no device).  One tiny
tensor each; nothing is launched."""
import pytest
import torch

from kasportsformer_amd import _args

pytestmark = pytest.mark.gpu


def current():
    return torch.device("cuda", torch.cuda.current_device())


def test_host_input_lands_on_the_current_device_with_an_index():
    dev = _args.resolve_device((torch.zeros(2), None), None, "t")
    assert dev == current() and dev.index is not None
    assert _args.resolve_device((), None, "t") == current(), "no tensors at all: what SortTracker passes"


def test_a_bare_cuda_gains_the_current_index():
    for device in ("cuda", torch.device("cuda")):
        dev = _args.resolve_device((torch.zeros(2),), device, "t")
        assert dev == current() and dev.index is not None


def test_a_gpu_tensor_decides_and_may_be_named_explicitly():
    t = torch.zeros(2, device="cuda")
    assert _args.resolve_device((torch.zeros(2), t), None, "t") == t.device
    assert _args.resolve_device((t,), t.device, "t") == t.device
    assert _args.resolve_device((t,), str(t.device), "t") == t.device
    assert _args.resolve_device((t,), "cuda", "t") == t.device, "its own device, named without an index"
    with pytest.raises(RuntimeError, match="no CPU path"):
        _args.resolve_device((t,), "cpu", "t")


def test_a_tensor_on_another_gpu_is_refused():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    t, other = torch.zeros(2, device="cuda:0"), torch.zeros(2, device="cuda:1")
    with pytest.raises(RuntimeError, match="asked for"):
        _args.resolve_device((t,), "cuda:1", "t")
    with pytest.raises(RuntimeError, match="asked for"):
        _args.resolve_device((t, other), None, "t")
    assert _args.resolve_device((other,), None, "t") == other.device


def test_stream_is_the_current_streams_handle():
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert _args.stream().value == s.cuda_stream
    assert (_args.stream().value or 0) == torch.cuda.current_stream().cuda_stream
