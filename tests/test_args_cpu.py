"""kasportsformer_amd/_args.py, the host-side argument plumbing the video and pose ops share, without a device: what each helper refuses and with which
exception type, what it shares with its input, and the rule that no module reaches into a sibling's private names except the ones listed here."""
import ast
import glob
import os

import numpy as np
import pytest
import torch

from kasportsformer_amd import _args

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kasportsformer_amd")

# the lift family shares lift logic through private names; everything else goes through _lib, _args and _tracks
ALLOWED_PRIVATE_IMPORTS = {
    ("stream", "lift"): {"_forward_windows", "_model_device", "_per_row", "_upload"},
    ("tracked", "lift"): {"_forward_windows", "_model_device", "_per_row", "_upload"},
    ("tracked", "stream"): {"_checked_tables", "_decode_on"},
}


def test_resolve_device_refuses_a_host_device_and_a_box_without_gpu():
    t = torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _args.resolve_device((t, None), "cpu", "t")
    with pytest.raises(RuntimeError, match="no CPU path"):
        _args.resolve_device((), torch.device("cpu"), "t")
    if torch.cuda.is_available():
        pytest.skip("the no-GPU refusal needs a box without one")
    with pytest.raises(RuntimeError, match="no GPU available"):
        _args.resolve_device((t,), None, "t")
    with pytest.raises(RuntimeError, match="no GPU available"):
        _args.resolve_device((), None, "t")


def test_index_in_types_and_range():
    assert _args.index_in(np.int64(3), "t", "n", 0, 5) == 3 and type(_args.index_in(np.int64(3), "t", "n")) is int
    assert _args.index_in(5, "t", "n", 0, 5) == 5 and _args.index_in(-7, "t", "n") == -7
    for bad in (True, False, 2.0, "2", None):
        for any_index in (False, True):
            with pytest.raises(TypeError, match="n must be an int"):
                _args.index_in(bad, "t", "n", 0, 5, any_index=any_index)
    with pytest.raises(TypeError, match="n must be an int"):
        _args.index_in(np.bool_(True), "t", "n", 0, 5)
    for bad in (-1, 6, np.int32(6)):
        with pytest.raises(ValueError, match=r"n must be in \[0, 5\]"):
            _args.index_in(bad, "t", "n", 0, 5)

    class Idx:
        def __index__(self):
            return 4
    assert _args.index_in(Idx(), "t", "n", 0, 5, any_index=True) == 4           # the two acceptance rules differ exactly here
    with pytest.raises(TypeError):
        _args.index_in(Idx(), "t", "n", 0, 5)


def test_as_tensor_shares_memory_and_keeps_a_pitch_only_where_asked():
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    t = _args.as_tensor(a, "t", "x", _args.FLOAT32)
    a[1, 2] = -5.0
    assert t[1, 2] == -5.0 and t.data_ptr() == a.ctypes.data
    surface = np.zeros((6, 16), np.uint8)
    view = surface[:, :10]                                                       # a padded pitch
    kept = _args.as_tensor(view, "t", "x", _args.UINT8, keep_pitch=True)
    assert kept.stride() == (16, 1) and kept.data_ptr() == surface.ctypes.data
    assert _args.as_tensor(view, "t", "x", _args.UINT8).stride() == (10, 1)      # packed
    back = _args.as_tensor(view[::-1], "t", "x", _args.UINT8, keep_pitch=True)   # torch takes no negative stride: packed as well
    assert back.stride() == (10, 1) and np.array_equal(back.numpy(), view[::-1])
    g = torch.zeros(2, requires_grad=True)
    assert not _args.as_tensor(g, "t", "x", _args.FLOAT32).requires_grad
    half = _args.as_tensor(np.zeros(2, np.float16), "t", "x", _args.DTYPES)
    assert half.dtype == torch.float16 and _args.as_tensor(torch.zeros(2, dtype=torch.bfloat16), "t", "x", _args.DTYPES).dtype == torch.bfloat16
    with pytest.raises(TypeError, match="x must be float32, got float64"):
        _args.as_tensor(np.zeros(2), "t", "x", _args.FLOAT32)
    with pytest.raises(TypeError, match="x must be float32, float16 or bfloat16, got torch.int32"):
        _args.as_tensor(torch.zeros(2, dtype=torch.int32), "t", "x", _args.DTYPES)
    with pytest.raises(TypeError, match="x must be uint8, got int8"):
        _args.as_tensor(np.zeros(2, np.int8), "t", "x", _args.UINT8)
    with pytest.raises(TypeError, match="x must be a numpy array or a torch tensor, got list"):
        _args.as_tensor([1.0], "t", "x", _args.FLOAT32)
    with pytest.raises(RuntimeError, match="unsupported device"):
        _args.as_tensor(torch.zeros(2, device="meta"), "t", "x", _args.FLOAT32)


def test_frames_shape_rule():
    assert tuple(_args.frames(np.zeros((4, 5, 3), np.uint8), "t").shape) == (4, 5, 3)
    assert tuple(_args.frames(torch.zeros((2, 4, 5, 3), dtype=torch.uint8), "t").shape) == (2, 4, 5, 3)
    for shape in ((4, 5, 4), (0, 4, 5, 3), (4, 5), (0, 5, 3), (4, 0, 3), (1, 2, 4, 5, 3), (_args.MAX_SIDE + 1, 1, 3)):
        with pytest.raises(ValueError, match="expected frame"):
            _args.frames(torch.zeros(shape, dtype=torch.uint8), "t")
    with pytest.raises(TypeError, match="frame must be uint8"):
        _args.frames(np.zeros((4, 5, 3), np.float32), "t")


def test_pitched_and_step():
    buf = torch.zeros(4096, dtype=torch.uint8)
    ok = buf.as_strided((2, 4, 5, 3), (512, 32, 3, 1))
    assert _args.pitched(ok, 3) and _args.step(ok, 1, 15) == 32
    assert not _args.pitched(buf.as_strided((2, 4, 5, 3), (512, 14, 3, 1)), 3), "rows overlap"
    assert not _args.pitched(buf.as_strided((2, 4, 5, 3), (100, 32, 3, 1)), 3), "frames overlap"
    assert not _args.pitched(buf.as_strided((2, 4, 5, 3), (512, 32, 6, 1)), 3), "pixels not interleaved"
    assert not _args.pitched(buf.as_strided((2, 4, 5, 3), (512, 32, 3, 2)), 3)
    one = buf.as_strided((1, 1, 1, 3), (0, 0, 0, 1))                             # dimensions of one element are not looked at
    assert _args.pitched(one, 3) and _args.step(one, 1, 3) == 3
    assert _args.pitched(buf.as_strided((2, 4, 5), (64, 8, 1)), 1) and not _args.pitched(buf.as_strided((2, 4, 5), (64, 8, 2)), 1)


def test_no_module_imports_a_siblings_private_name():
    seen = 0
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        module = os.path.basename(path)[:-3]
        for node in ast.walk(ast.parse(open(path).read())):
            if not isinstance(node, ast.ImportFrom) or node.level != 1:
                continue
            seen += 1
            if node.module is None:                                              # from . import a, b: whole modules
                private = {a.name for a in node.names if a.name.startswith("_")} - {"_lib", "_args"}
                assert not private, f"{module}.py imports the private module(s) {sorted(private)}"
            elif node.module not in ("_lib", "_args"):
                private = {a.name for a in node.names if a.name.startswith("_")}
                extra = private - ALLOWED_PRIVATE_IMPORTS.get((module, node.module), set())
                assert not extra, f"{module}.py imports {sorted(extra)} from {node.module}.py: share it through _args.py"
    assert seen > 20, "the walk found the package's imports"
