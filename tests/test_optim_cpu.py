"""kasportsformer_amd.AdamW's host logic without a device: the planner (segments -> runs -> chunks), what the constructor refuses, the state-dict interchange with
a stock torch.optim.AdamW over a model on the CPU, and its standing as a torch.optim.Optimizer.  No step is taken here (there is no CPU update)."""
import io

import numpy as np
import pytest
import torch

import kasportsformer_amd as K
from kasportsformer_amd import _lib
from kasportsformer_amd.optim import CHUNK_DTYPE, plan_chunks
from tests import optim_ref as R


@pytest.fixture(scope="module")
def model():
    return K.KASportsFormer(n_layers=1, n_frames=9)


def check_plan(offsets, numels, classes, n, chunk_max=_lib.OPT_CHUNK_MAX):
    """Coverage count: every listed element in exactly one chunk of its own class, nothing else in any; the bounds on a chunk; runs merged within a class only."""
    t = plan_chunks(offsets, numels, classes, chunk_max)
    assert t.dtype == CHUNK_DTYPE
    want_cls = np.full(n, -1, np.int64)
    for o, c, k in zip(offsets, numels, classes):
        want_cls[o:o + c] = k
    count, got_cls = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    for ch in t:
        b, c = int(ch["begin"]), int(ch["count"])
        assert 1 <= c <= chunk_max and 0 <= b and b + c <= n
        count[b:b + c] += 1
        got_cls[b:b + c] = ch["cls"]
    assert np.array_equal(count, (want_cls >= 0).astype(np.int64)), "every listed element exactly once, no other element at all"
    assert np.array_equal(got_cls, want_cls), "a chunk never spans two classes"
    assert (np.diff(t["begin"]) > 0).all()
    # as few chunks as the runs allow: a run of L elements beginning at b gives ceil((b % 4 + L) / chunk_max) chunks, so neighbours of one class were merged
    change = np.flatnonzero(np.diff(np.concatenate([[-1], want_cls, [-1]])) != 0)
    runs = [(lo, hi) for lo, hi in zip(change[:-1], change[1:]) if want_cls[lo] >= 0]
    assert len(t) == sum(-(-(lo % 4 + hi - lo) // chunk_max) for lo, hi in runs)
    for ch in t:                                   # all but a run's first chunk begin on a 16-byte boundary
        if not any(lo == ch["begin"] for lo, _ in runs):
            assert ch["begin"] % 4 == 0
    return t


def test_planner_on_the_odd_layout():
    offs, nums, cls = zip(*R.SEGMENTS)
    t = check_plan(offs, nums, cls, R.N_FLAT)
    assert t[0]["begin"] == 3 and t[0]["count"] == 3, "[3, 4) and [4, 6) share a class: one run"
    assert {(int(c["begin"]), int(c["count"]), int(c["cls"])) for c in t[1:3]} == {(7, 3, 1), (10, 4, 0)}, "[7, 10) and [10, 14) touch across classes: two runs"
    for cm in (4, 8, 64):
        check_plan(offs, nums, cls, R.N_FLAT, cm)
    shuffled = np.random.default_rng(0).permutation(len(offs))
    assert np.array_equal(plan_chunks(np.array(offs)[shuffled], np.array(nums)[shuffled], np.array(cls)[shuffled]), t), "the order of the segments does not matter"
    assert len(plan_chunks([], [], [])) == 0 and len(plan_chunks([5], [0], [0])) == 0
    with pytest.raises(ValueError):
        plan_chunks([0, 3], [4, 2], [0, 0])


def test_planner_on_a_real_parameter_list(model):
    live = [(off, n) for _, off, n, _ in model._live]
    offs, nums = zip(*live)
    one = check_plan(offs, nums, [0] * len(live), model.n_flat)
    full = int((one["count"] == _lib.OPT_CHUNK_MAX).sum())
    assert len(one) - full < len(live) / 2, "one class: neighbours merge into runs (the layout pads odd-sized tensors apart, so not into one)"
    # the issue's no-decay split: 1-D tensors and the three position embeddings against the rest; then every third tensor frozen
    names = {id(p): n for n, p in model.named_parameters()}
    cls = [1 if (p.dim() == 1 or names[id(p)].endswith("pos_embed")) else 0 for p, _, _, _ in model._live]
    check_plan(offs, nums, cls, model.n_flat)
    keep = [i for i in range(len(live)) if i % 3]
    check_plan([offs[i] for i in keep], [nums[i] for i in keep], [cls[i] for i in keep], model.n_flat)
    assert min(nums) == 1 and 3 in nums, "fc2.bias [1] and fusion_three_channel.bias [3] are in the list"


def test_what_the_constructor_refuses(model):
    params = list(model.parameters())
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=flag):
            K.AdamW(params, **{flag: True})
        with pytest.raises(NotImplementedError, match=flag):
            K.AdamW([{"params": params, flag: True}])
    with pytest.raises(ValueError, match="lr"):
        K.AdamW(params, lr=torch.tensor(1e-3))
    with pytest.raises(ValueError, match="lr"):
        K.AdamW([{"params": params, "lr": torch.tensor(1e-3)}])
    with pytest.raises(ValueError, match="parameter 1 .*belongs to no"):
        K.AdamW([params[0], torch.nn.Parameter(torch.zeros(3))])
    other = K.KASportsFormer(n_layers=1, n_frames=9)
    with pytest.raises(ValueError, match=r"parameter 2 \(head\.bias.*second KASportsFormer"):
        K.AdamW([model.head.weight, model.head.bias, other.head.bias])
    K.AdamW(params, foreach=True)
    K.AdamW(params, fused=True)
    K.AdamW(filter(lambda p: p.requires_grad, model.parameters()), lr=5e-4, weight_decay=0.01)          # the reference's call


def test_it_is_a_torch_optimizer_and_schedulers_take_it(model):
    opt = K.AdamW([{"params": [model.head.weight], "lr": 1e-2, "weight_decay": 0.0}, {"params": [model.head.bias]}], lr=5e-4, max_grad_norm=1.0)
    assert isinstance(opt, torch.optim.Optimizer) and isinstance(opt, torch.optim.AdamW)
    assert opt.grad_norm is None and opt.clip_coef is None and opt.grad_scale == 1.0
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == [5e-3, 2.5e-4]
    never_used = [p for n, p in model.named_parameters() if "att_spatial.norm1_limb" in n]
    assert never_used and K.AdamW(never_used)._live.sum() == 0, "the norm1_limb tensors beyond n_live are accepted and never step"
    with pytest.raises(RuntimeError, match="MI355X"):
        model.head.weight.grad = torch.zeros_like(model.head.weight)
        try:
            opt.step()
        finally:
            model.head.weight.grad = None


def stock_state(params, steps):
    """A hand-made torch.optim.AdamW state over `params` (those with a step of 0 have none), steps differing."""
    g = torch.Generator().manual_seed(7)
    state = {i: {"step": torch.tensor(float(s)), "exp_avg": torch.randn(p.shape, generator=g), "exp_avg_sq": torch.rand(p.shape, generator=g)}
             for i, (p, s) in enumerate(zip(params, steps)) if s}
    group = {"lr": 3e-4, "betas": (0.8, 0.99), "eps": 1e-7, "weight_decay": 0.02, "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
             "differentiable": False, "fused": None, "decoupled_weight_decay": True, "params": list(range(len(params)))}
    return {"state": state, "param_groups": [group]}


def test_state_round_trips_through_a_stock_adamw_without_a_step(model):
    params = [p for p, _, _, _ in model._live]
    steps = [(0, 3, 5, 5, 11)[i % 5] for i in range(len(params))]
    sd = stock_state(params, steps)
    opt = K.AdamW(params)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 3e-4 and opt.param_groups[0]["betas"] == (0.8, 0.99) and opt.param_groups[0]["weight_decay"] == 0.02
    # the state lives in the flat arrays, as views; the steps in one CPU vector
    for i, p in enumerate(params):
        if steps[i]:
            st = opt.state[p]
            assert st["exp_avg"].untyped_storage().data_ptr() == opt._exp_avg.untyped_storage().data_ptr() and st["exp_avg"].shape == p.shape
            assert st["step"].dim() == 0 and st["step"].dtype == torch.float32 and not st["step"].is_cuda and float(st["step"]) == steps[i]
            off = model._p_entries[next(n for n, q in model.named_parameters() if q is p)][0]
            assert torch.equal(opt._exp_avg[off:off + p.numel()], sd["state"][i]["exp_avg"].reshape(-1))
        else:
            assert p not in opt.state or not opt.state[p]
    out = opt.state_dict()
    assert sorted(out["state"]) == sorted(sd["state"])
    ptrs = [t.untyped_storage().data_ptr() for st in out["state"].values() for t in st.values()]
    assert len(set(ptrs)) == len(ptrs), "no two tensors of a state dict alias"
    buf = io.BytesIO()
    torch.save(out, buf)
    buf.seek(0)
    out = torch.load(buf, weights_only=True)
    stock = torch.optim.AdamW(params)
    stock.load_state_dict(out)
    back = stock.state_dict()
    assert {k: v for k, v in back["param_groups"][0].items()} == {k: v for k, v in sd["param_groups"][0].items()}
    for i, st in sd["state"].items():
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][key], st[key]), (i, key)
    again = K.AdamW(params)
    again.load_state_dict(back)
    assert torch.equal(again._exp_avg, opt._exp_avg) and torch.equal(again._exp_avg_sq, opt._exp_avg_sq) and torch.equal(again._steps, opt._steps)
    with pytest.raises(ValueError):
        K.AdamW(params[:-1]).load_state_dict(sd)


def test_checkpoint_helpers_dispatch_on_a_torch_optimizer(model):
    params = list(model.parameters())
    live = {id(p) for p, _, _, _ in model._live}
    sd = stock_state(params, [4 if id(p) in live else 0 for p in params])
    opt = K.AdamW(params)
    K.load_adamw_state_dict(opt, sd)
    out = K.adamw_state_dict(opt)
    assert all(not t.is_cuda for st in out["state"].values() for t in st.values()) and sorted(out["state"]) == sorted(sd["state"])
    fused_like = K.adamw_state_dict(opt)
    assert fused_like["param_groups"][0]["params"] == list(range(len(params)))
    with pytest.raises(ValueError, match="flat"):
        K.load_adamw_state_dict(opt, {"step": 1, "exp_avg": None, "exp_avg_sq": None, "param_groups": []})
