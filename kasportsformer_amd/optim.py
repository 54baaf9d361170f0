"""AdamW over the model's flat parameter array (one kernel instead of 2,611 small updates).

Semantics are torch.optim.AdamW's (train_and_evaluate_sp.py:270-272: lr 5e-4, wd 0.01, betas (0.9, 0.999),
eps 1e-8); parameters that never receive a gradient (the 208 norm1_limb tensors of the non-bone blocks,
KASportsFormer.py:73) are skipped exactly like torch skips ``grad is None``.

``FusedAdamW(model)`` is the leanest form: one group, one step count, one launch over ``[0, n_live)``.  ``AdamW(params, ...)`` below is the drop-in one: a
``torch.optim.AdamW`` subclass with groups, subsets, per-parameter steps and norm clipping, one launch over a chunk table.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from .model import parameter_owner


class FusedAdamW:
    def __init__(self, model, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
        self.model = model
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)]
        self.step_index = 0
        self.exp_avg = torch.zeros(model.n_live, dtype=torch.float32, device=model._flat.device)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.grad_scale = 1.0            # DataParallel sets 1/world_size (all-reduce is a sum)

    def zero_grad(self, set_to_none=True):
        self.model.flat_grad = None
        if self.model.attach_param_grads:
            for p in self.model.parameters():
                p.grad = None

    @torch.no_grad()
    def step(self):
        m = self.model
        if m.flat_grad is None:
            raise RuntimeError("FusedAdamW.step() called before backward")
        g = self.param_groups[0]
        self.step_index += 1
        _lib.check(_lib.load().kasf_adamw_step(m._flat.data_ptr(), m.flat_grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                               m.n_live, g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.step_index,
                                               self.grad_scale, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        if m._const_index is not None:   # use_layer_scale=False: the layer-scale slices are the constant 1, not parameters
            m._flat.index_fill_(0, m._const_index, 1.0)
        m.mark_weights_dirty()

    def state_dict(self):
        return {"step": self.step_index, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "param_groups": self.param_groups}

    def load_state_dict(self, sd):
        self.step_index = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.param_groups = sd["param_groups"]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# AdamW as torch.optim spells it: parameters in, groups, subsets, per-parameter steps, norm clipping -- still one update launch over the flat arrays
# ---------------------------------------------------------------------------------------------------------------------------------------------------------
CHUNK_DTYPE = np.dtype([("begin", "<i8"), ("count", "<i4"), ("cls", "<i4")])      # KasfOptChunk (include/kasf.h)


def plan_chunks(offsets, numels, classes, chunk_max: int = _lib.OPT_CHUNK_MAX) -> np.ndarray:
    """The chunk table of ``kasf_adamw_segments`` / ``kasf_grad_norm`` (include/kasf.h) for segments ``(offset, numel, class)`` of the flat array, pure numpy:
    segments sorted by offset, those that touch and share a class merged into runs, every run cut into chunks of at most ``chunk_max`` elements.  A run is cut
    where ``(position - (run begin rounded down to 4)) % chunk_max == 0``, so every chunk but a run's first begins on a 16-byte boundary whatever the run's
    begin.  Segments must not overlap; empty ones are dropped.  Returns a ``CHUNK_DTYPE`` array in ascending order of ``begin``."""
    off, num, cls = (np.asarray(a, np.int64).reshape(-1) for a in (offsets, numels, classes))
    if not (len(off) == len(num) == len(cls)):
        raise ValueError("plan_chunks: offsets, numels and classes differ in length")
    if chunk_max < 4 or chunk_max % 4:
        raise ValueError("plan_chunks: chunk_max must be a positive multiple of 4")
    keep = num > 0
    off, num, cls = off[keep], num[keep], cls[keep]
    if len(off) == 0:
        return np.zeros(0, CHUNK_DTYPE)
    order = np.argsort(off, kind="stable")
    off, num, cls = off[order], num[order], cls[order]
    end = off + num
    if (off < 0).any() or (num < 0).any() or (off[1:] < end[:-1]).any():
        raise ValueError("plan_chunks: segments overlap or lie before element 0")
    first = np.ones(len(off), bool)
    first[1:] = (off[1:] != end[:-1]) | (cls[1:] != cls[:-1])
    starts = np.flatnonzero(first)
    run_begin, run_end, run_cls = off[starts], end[np.append(starts[1:], len(off)) - 1], cls[starts]
    grid0 = run_begin & ~np.int64(3)                                # where the run's cutting grid starts
    per_run = -((grid0 - run_end) // chunk_max)                     # ceil((run_end - grid0) / chunk_max)
    run = np.repeat(np.arange(len(starts)), per_run)
    j = np.arange(per_run.sum()) - np.repeat(np.cumsum(per_run) - per_run, per_run)
    out = np.zeros(len(run), CHUNK_DTYPE)
    lo = np.maximum(grid0[run] + j * chunk_max, run_begin[run])
    out["begin"] = lo
    out["count"] = np.minimum(grid0[run] + (j + 1) * chunk_max, run_end[run]) - lo
    out["cls"] = run_cls[run]
    return out


class AdamW(torch.optim.AdamW):
    """``torch.optim.AdamW`` for the parameters of ONE ``KASportsFormer``, with the stock signature (torch 2.10) plus keyword-only ``max_grad_norm``: the
    reference's ``optim.AdamW(filter(lambda p: p.requires_grad, model.parameters()), lr, weight_decay)`` (train_and_evaluate_sp.py:270-272) becomes
    ``K.AdamW(...)`` with the same arguments.  It is a ``torch.optim.Optimizer`` (``lr_scheduler.*`` take it), has parameter groups with their own ``lr`` /
    ``betas`` / ``eps`` / ``weight_decay``, steps any subset of the model's parameters, skips a parameter whose ``.grad`` is None and keeps a step count per
    parameter exactly like torch -- and every parameter that steps still goes out in ONE launch over the model's flat array (``kasf_adamw_segments``:
    a chunk table on the device says which elements, the groups' hyper-parameters travel in the kernel arguments).

    ``max_grad_norm``: clip by the global L2 norm of the gradients of exactly the parameters that step, all groups together -- ``clip_grad_norm_(params,
    max_grad_norm)`` in front of the step, as two more launches over the same table (``kasf_grad_norm``, fp64 sums in a fixed order: bit-reproducible), with
    no host read-back: ``grad_norm`` and ``clip_coef`` are 0-dim CUDA tensors holding the last step's values (None without ``max_grad_norm``;
    ``max_grad_norm=float('inf')`` measures without clipping).  UNLIKE ``clip_grad_norm_``, ``p.grad`` itself is NOT scaled: the coefficient is applied to
    the gradient as the update reads it.  With ``grad_scale`` (``DataParallel`` sets 1 / world_size) the norm is that of the averaged gradient.

    Refused: ``amsgrad``, ``maximize``, ``capturable``, ``differentiable`` (NotImplementedError); a tensor ``lr`` or ``betas`` (reading it would synchronise);
    a parameter that belongs to no ``KASportsFormer``, or parameters of two models (ValueError; a second model gets a second optimiser).  ``foreach`` and
    ``fused`` are accepted and ignored.  The never-used ``norm1_limb`` tensors are accepted and never stepped (their ``.grad`` is always None).  ``step()``
    needs ``model.attach_param_grads = True`` (the default): it reads ``p.grad`` -- in place when it is the model's own view of ``flat_grad``, through a
    staging copy when the caller put another tensor there.

    State: ``state[p]['exp_avg'] / ['exp_avg_sq']`` are views of two flat arrays the optimiser owns, ``state[p]['step']`` a 0-dim view of one CPU float32
    vector; ``state_dict()`` returns the stock layout with tensors of their own, ``load_state_dict()`` takes that and a stock ``torch.optim.AdamW``'s,
    differing per-parameter steps included.  ``step()`` and ``zero_grad()`` never synchronise with the device."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None, capturable=False,
                 differentiable=False, fused=None, max_grad_norm=None):
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("kasportsformer_amd.AdamW: lr and betas must be Python floats (a tensor would have to be read back on every step)")
        self._bound = False
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, foreach=None, capturable=capturable,
                         differentiable=differentiable, fused=None)
        self.max_grad_norm = max_grad_norm
        self.grad_scale = 1.0            # DataParallel sets 1 / world_size (the all-reduce is a sum)
        self._exp_avg = self._exp_avg_sq = self._stage = self._clip = self._partial = None
        self._plan_key, self._launches, self._table, self._pinned = None, [], None, []
        self._bind()

    # ------------------------------------------------------------------ what the optimiser covers
    @staticmethod
    def _check_groups(groups):
        for g in groups:
            for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
                if g.get(flag):
                    raise NotImplementedError(f"kasportsformer_amd.AdamW: {flag}=True is not built (use torch.optim.AdamW over model.parameters())")
            if isinstance(g.get("lr"), torch.Tensor) or any(isinstance(b, torch.Tensor) for b in g.get("betas", ())):
                raise ValueError("kasportsformer_amd.AdamW: lr and betas must be Python floats (a tensor would have to be read back on every step)")

    def _bind(self):
        self._check_groups(self.param_groups)
        self._params = [p for g in self.param_groups for p in g["params"]]
        model, offs = None, []
        for i, p in enumerate(self._params):
            m, off = parameter_owner(p)
            if m is None:
                raise ValueError(f"kasportsformer_amd.AdamW: parameter {i} (shape {tuple(p.shape)}) belongs to no kasportsformer_amd.KASportsFormer; "
                                 "give parameters of other modules to an optimiser of their own")
            if model is None:
                model = m
            elif m is not model:
                name = next((n for n, q in m.named_parameters() if q is p), "?")
                raise ValueError(f"kasportsformer_amd.AdamW: parameter {i} ({name}, shape {tuple(p.shape)}) belongs to a second KASportsFormer; "
                                 "one optimiser steps one model -- give the second model a second optimiser")
            offs.append(off)
        self._model_ref = weakref.ref(model)
        self._slot = {p: i for i, p in enumerate(self._params)}
        self._off = np.asarray(offs, np.int64)
        self._numel = np.asarray([p.numel() for p in self._params], np.int64)
        self._group_of = np.asarray([k for k, g in enumerate(self.param_groups) for _ in g["params"]], np.int64)
        self._live = self._off < model.n_live                      # the norm1_limb tensors behind n_live never step
        live_here = {int(o) for o in self._off[self._live]}
        self._covers_model = all(off in live_here for _, off, _, _ in model._live)
        old = getattr(self, "_steps", None)
        self._steps = torch.zeros(len(self._params), dtype=torch.float32)      # CPU: state[p]['step'] are its 0-dim views, a step is one vectorised add
        if old is not None:
            self._steps[:len(old)] = old
            for p, st in self.state.items():
                if st and p in self._slot:
                    st["step"] = self._steps[self._slot[p]]
        self._steps_np = self._steps.numpy()
        self._plan_key = None
        self._bound = True

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if self._bound:                   # after construction: the new parameters join the slots behind the old ones
            self._bind()

    def _model(self):
        model = self._model_ref()
        if model is None:
            raise RuntimeError("kasportsformer_amd.AdamW: the model these parameters belonged to is gone")
        return model

    @property
    def grad_norm(self):
        """0-dim CUDA fp32: the norm the last clipped step measured (of the averaged gradient under ``grad_scale``); None without ``max_grad_norm``."""
        return None if self.max_grad_norm is None or self._clip is None else self._clip[0]

    @property
    def clip_coef(self):
        """0-dim CUDA fp32: ``min(1, max_grad_norm / (grad_norm + 1e-6))`` of the last clipped step; None without ``max_grad_norm``."""
        return None if self.max_grad_norm is None or self._clip is None else self._clip[1]

    # ------------------------------------------------------------------ flat state
    def _moments(self, device):
        """The two flat moment arrays on `device` (created as zeros, moved along when the model moved), state views re-pointed after a move."""
        if self._exp_avg is None:
            n = self._model().n_live
            self._exp_avg = torch.zeros(n, dtype=torch.float32, device=device)
            self._exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=device)
        elif self._exp_avg.device != device:
            self._exp_avg, self._exp_avg_sq = self._exp_avg.to(device), self._exp_avg_sq.to(device)
            self._stage = self._clip = self._partial = None
            for p, st in self.state.items():
                if st and p in self._slot:
                    self._point(p, st)

    def _point(self, p, st):
        i = self._slot[p]
        off, n = int(self._off[i]), int(self._numel[i])
        st["step"] = self._steps[i]
        st["exp_avg"] = self._exp_avg[off:off + n].view(p.shape)
        st["exp_avg_sq"] = self._exp_avg_sq[off:off + n].view(p.shape)

    def _upload(self, table, device):
        host = torch.from_numpy(table.view(np.int64).reshape(-1, 2).copy()).pin_memory()      # pinned + non_blocking: no synchronisation
        self._pinned.append(host)                                                          # alive until the copy has run
        return host.to(device, non_blocking=True)

    def _replan(self, idx, inv, n_classes, device):
        """A new partition -- which parameters step, and into which classes -- : state for the newcomers, the chunk table built and uploaded."""
        self._moments(device)
        for i in idx.tolist():
            p = self._params[i]
            if not self.state.get(p):
                self._point(p, self.state[p])
        table = plan_chunks(self._off[idx], self._numel[idx], inv)
        assert len(table) and table["begin"].min() >= 0 and (table["begin"] + table["count"]).max() <= self._exp_avg.numel() and table["count"].min() >= 1 \
            and table["count"].max() <= _lib.OPT_CHUNK_MAX
        self._pinned = []
        self._table = (self._upload(table, device), len(table))                               # the norm reads every chunk, whatever its class
        if n_classes <= _lib.OPT_MAX_CLASSES:
            self._launches = [(self._table[0], len(table), 0, n_classes)]
        else:                                                                                # beyond 32 classes: one launch per 32 of them
            self._launches = []
            for lo in range(0, n_classes, _lib.OPT_MAX_CLASSES):
                part = table[(table["cls"] >= lo) & (table["cls"] < lo + _lib.OPT_MAX_CLASSES)].copy()
                part["cls"] -= lo
                self._launches.append((self._upload(part, device), len(part), lo, min(_lib.OPT_MAX_CLASSES, n_classes - lo)))
        self._partial = torch.empty(len(table), dtype=torch.float64, device=device)

    # ------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        model = self._model()
        if not model.attach_param_grads:
            raise RuntimeError("kasportsformer_amd.AdamW.step() reads p.grad, and with model.attach_param_grads = False every p.grad is None: nothing would "
                               "be updated.  Leave attach_param_grads = True, or step the whole flat array with kasportsformer_amd.FusedAdamW(model)")
        flat = model._flat                                    # read at every step: model.to(...) re-creates it
        if not flat.is_cuda:
            raise RuntimeError("kasportsformer_amd runs on an MI355X only (move the model to 'cuda'); there is no CPU fallback")
        self._check_groups(self.param_groups)
        # one pass over the parameters: p.grad and where it lives (-1: None).  This pass is step()'s host cost, some 0.15 us per parameter.
        grads = [p.grad for p in self._params]
        where = np.fromiter((-1 if g is None else g.data_ptr() for g in grads), np.int64, len(grads))
        has = (where != -1) & self._live
        idx = np.flatnonzero(has)
        if len(idx) == 0:
            return loss
        # classes: (group, step count) of the parameters that step; the table depends on who is in which class, not on the counts themselves
        uniq, inv = np.unique((self._group_of[idx] << 32) | self._steps_np[idx].astype(np.int64), return_inverse=True)
        key = (has.tobytes(), inv.astype(np.int32).tobytes(), flat.device)
        if key != self._plan_key:
            self._replan(idx, inv, len(uniq), flat.device)
            self._plan_key = key
        # the gradient: the model's flat array where every p.grad is its view of it, a staging copy where the caller put tensors of their own
        fg = model.flat_grad
        ptrs = where[idx] - 4 * self._off[idx]
        if fg is not None and fg.device == flat.device and fg.dtype == torch.float32 and (ptrs == fg.data_ptr()).all():
            garr = fg
        else:
            if self._stage is None:
                self._stage = torch.zeros(model.n_live, dtype=torch.float32, device=flat.device)
            garr = self._stage
            for i in idx.tolist():
                off, n = int(self._off[i]), int(self._numel[i])
                garr[off:off + n].copy_(grads[i].reshape(-1))
        self._steps_np[idx] += 1.0
        self._launch(model, garr, uniq)
        model.mark_weights_dirty()
        return loss

    def _launch(self, model, garr, uniq):
        """The device work of one step over the cached table: the norm's two launches when clipping, then the update; `uniq` holds each class's
        (group << 32 | step count before the increment)."""
        flat = model._flat
        lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
        clip = None
        if self.max_grad_norm is not None:
            if self._clip is None:
                self._clip = torch.zeros(2, dtype=torch.float32, device=flat.device)
            clip = self._clip.data_ptr()
            _lib.check(lib.kasf_grad_norm(garr.data_ptr(), model.n_live, self._table[0].data_ptr(), self._table[1], self._partial.data_ptr(),
                                          self.grad_scale, float(self.max_grad_norm), clip, stream))
        for table, n_chunks, lo, n_cls in self._launches:
            classes = (_lib.KasfAdamwClass * n_cls)()
            for k in range(n_cls):
                u = int(uniq[lo + k])
                g = self.param_groups[u >> 32]
                classes[k] = _lib.KasfAdamwClass(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], 0.0, 0.0, (u & 0xFFFFFFFF) + 1)
            _lib.check(lib.kasf_adamw_segments(flat.data_ptr(), garr.data_ptr(), self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(), model.n_live,
                                               table.data_ptr(), n_chunks, classes, n_cls, self.grad_scale, clip, stream))

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none=set_to_none)
        if set_to_none and self._covers_model:          # every live gradient is gone: the flat array with them, so that the next backward starts afresh
            self._model().flat_grad = None

    # ------------------------------------------------------------------ state dicts
    def state_dict(self):
        """The stock layout; every tensor a copy of its own (no views of the flat arrays), so it goes through ``torch.save`` and into a stock
        ``torch.optim.AdamW.load_state_dict`` over the same parameter list."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (v.clone() if isinstance(v, torch.Tensor) else v) for n, v in st.items()} for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Its own ``state_dict()`` or a stock ``torch.optim.AdamW``'s over the same parameter list (per-parameter steps may differ): scattered into the flat
        arrays, the state views re-pointed."""
        self._check_groups(state_dict["param_groups"])
        super().load_state_dict(state_dict)                # validates the groups, casts to the parameters' device, takes the saved hyper-parameters
        model = self._model()
        for g in self.param_groups:
            g["foreach"] = g["fused"] = None
        loaded = {p: st for p, st in self.state.items() if st and isinstance(p, torch.Tensor) and p in self._slot}
        for p, st in loaded.items():
            i = self._slot[p]
            if not self._live[i]:
                raise ValueError("optimizer state present for a parameter that never receives a gradient")
            if tuple(st["exp_avg"].shape) != tuple(p.shape) or tuple(st["exp_avg_sq"].shape) != tuple(p.shape):
                raise ValueError(f"optimizer state shape {tuple(st['exp_avg'].shape)} does not match parameter {tuple(p.shape)}")
        self._moments(model._flat.device)
        self._exp_avg.zero_()
        self._exp_avg_sq.zero_()
        self._steps.zero_()
        for p, st in loaded.items():
            i = self._slot[p]
            off, n = int(self._off[i]), int(self._numel[i])
            self._exp_avg[off:off + n].copy_(st["exp_avg"].reshape(-1))
            self._exp_avg_sq[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            self._steps[i] = float(st["step"])
            self._point(p, st)
        self._plan_key = None
