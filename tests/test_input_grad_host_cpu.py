"""csrc/k_input_grad.hip without a GPU: the kernel's own source compiled for the host with g++ (-ffp-contract=off) behind the lockstep emulation of its
workgroups (tests/host_emul/) and held to the fp64 restatement of tests/input_grad_ref.py within the fp32 bar.  It shows the kernel's tables and their inverses,
its parameter staging, its null-pointer handling, its grid-stride walk and its summation order; the device's own GELU' arithmetic stays with
tests/test_gpu_input_grad.py (the entry file supplies libm's).

One size past the grid costs 513 workgroups of 256 host threads per launch, so at 2,049 frames only the three gradients together run (one launch, shared by the
tests below); each path alone runs at 1 and 3 frames, where every kernel path but the second walk is taken.

The same entry as a stand-alone program under the sanitizers (run once for the change that added the kernel: no report, exit 0), from a directory that holds a
copy of csrc/k_input_grad.hip:
    g++ -std=c++20 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -DEMUL_INPUT_GRAD_MAIN -x c++ -I. -Itests/host_emul \
        -Ikasportsformer_amd/csrc tests/host_emul/emul_input_grad.cpp -o ig_asan -lpthread && ./ig_asan
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import input_grad_ref as G
from tests import misc_ref as R
from tests.host_emul import build, vp

F32 = np.float32
CANARY = F32(-77.5)
PAD = 64                                                  # canary floats on either side of dx
BIG = G.SECOND_WALK + 1


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    lib = build(tmp_path_factory, "input_grad_host", "emul_input_grad.cpp", copy=("k_input_grad.hip",))
    lib.emul_input_grad.argtypes = [C.c_void_p] * 7 + [C.c_int64]
    return lib


@pytest.fixture(scope="module")
def model():
    """(flat fp32 parameters as numpy, KasfProOff as int64 words, name -> fp32 tensor) of a layout-only model with name-seeded limb-MLP parameters"""
    from kasportsformer_amd import _lib
    lib = _lib.load()
    cfg, h = _lib.KasfConfig(1, 4, 8, 4, 1, 0), C.c_void_p()
    _lib.check(lib.kasf_model_create_layout_only(C.byref(cfg), C.byref(h)))
    ents = _lib.param_entries(h)
    flat = R.fill_params(ents, lib.kasf_param_count(h))
    lib.kasf_model_destroy(h)
    where = {n: o for n, o, _ in ents}
    off = np.zeros(51 * 4 + 9, np.int64)
    for i in range(17):
        for ch, name in enumerate(G._CH):
            pre = f"bone_refusion.mlp_layers.{i}.{name}."
            off[(i * 3 + ch) * 4:(i * 3 + ch) * 4 + 4] = [where[pre + "fc1.weight"], where[pre + "fc1.bias"], where[pre + "fc2.weight"], where[pre + "fc2.bias"]]
    return np.ascontiguousarray(flat.numpy()), off, R.named(flat, ents, torch.float32)


def run(emul, model, x, a, b, c):
    """dx [frames,17,3] of one emulated kasf_launch_input_grad; the canaries around dx and every input must come back as they were"""
    flat, off, _ = model
    frames = x.shape[0]
    arr = [None if t is None else np.ascontiguousarray(t.numpy(), F32) for t in (x, a, b, c)]
    keep = [None if t is None else t.copy() for t in arr]
    buf = np.full(frames * 51 + 2 * PAD, CANARY, F32)
    buf[PAD:PAD + frames * 51] = np.nan
    out = buf[PAD:PAD + frames * 51]
    n = emul.emul_input_grad(vp(arr[0]), vp(flat), vp(off), *[None if t is None else vp(t) for t in arr[1:]], vp(out), frames)
    assert n == 1, "one launch per call"
    assert (buf[:PAD] == CANARY).all() and (buf[PAD + frames * 51:] == CANARY).all(), "dx was written out of bounds"
    assert all(k is None or np.array_equal(k, t) for k, t in zip(keep, arr)), "an input was written"
    assert np.isfinite(out).all(), "every element of dx is written, and finite at the zero-length bones"
    return torch.from_numpy(out.copy()).view(frames, 17, 3)


@pytest.fixture(scope="module")
def big(emul, model):
    i = G.inputs(BIG)
    return run(emul, model, i["x"], i["a"], i["b"], i["c"])


@pytest.mark.parametrize("path", list(G.PATHS))
@pytest.mark.parametrize("frames", [1, 3])
def test_kernel_source_on_the_host_follows_the_restatement(frames, path, emul, model):
    i = G.inputs(frames)
    got = run(emul, model, i["x"], *G.picked(i, path))
    err = G.frame_err(got, G.reference64(frames, path, model[2]))
    print(f"frames {frames} {path}: {err:.2e} (bar {G.BAR32:.0e})")
    assert err <= G.BAR32
    again = run(emul, model, i["x"], *G.picked(i, path))
    assert again.numpy().tobytes() == got.numpy().tobytes(), "two runs give identical bits"


def test_one_frame_past_the_grid(big, model):
    """2,049 frames: 512 workgroups of four frames, and workgroup 0 walks on to frame 2,048, where prologue_x plants its zero-length bones again"""
    x = G.inputs(BIG)["x"]
    assert float((x[G.SECOND_WALK, 2, :2] - x[G.SECOND_WALK, 3, :2]).abs().max()) == 0 and not x[2].any()
    err = G.frame_err(big, G.reference64(BIG, "all", model[2]))
    print(f"frames {BIG} all: {err:.2e} (bar {G.BAR32:.0e})")
    assert err <= G.BAR32


def test_a_frame_alone_has_the_bits_it_has_in_the_batch(big, emul, model):
    i = G.inputs(BIG)
    for f in (0, 2, 5, 2047, G.SECOND_WALK):               # the planted frames, an ordinary one, the last of the first walk and the second walk's
        alone = run(emul, model, i["x"][f:f + 1], i["a"][f:f + 1], i["b"][f:f + 1], i["c"][f:f + 1])
        assert alone[0].numpy().tobytes() == big[f].numpy().tobytes(), f


def test_the_three_paths_add_up(emul, model):
    """each path alone is what it contributes to the sum: the joints path is `a` itself, the bones leave the confidence channel alone, and the three re-added
    on the host are the launch with all three, to fp32 rounding (the fp32 bar)"""
    i = G.inputs(3)
    parts = {p: run(emul, model, i["x"], *G.picked(i, p)) for p in G.PATHS}
    assert torch.equal(parts["joints"], i["a"])
    assert not parts["bones"][..., 2].any(), "the confidence channel receives nothing from the bones"
    assert G.frame_err(parts["joints"] + parts["bones"] + parts["limbs"], parts["all"]) <= G.BAR32
