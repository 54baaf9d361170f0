"""Fused training losses of the path: the three-term loss the reference trains with (utils/loss_calc.py:6-27 combined as in train_and_evaluate_sp.py:212-222)
and its complete seven-term loss (utils/loss_calc.py:30-94, train_and_evaluate_sp.py:216-220)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


class _Loss3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, lambda_n, lambda_v):
        if not pred.is_cuda:
            raise RuntimeError("kasportsformer_amd.loss3 runs on the GPU only")
        pred, target = pred.contiguous().float(), target.contiguous().float()
        B, T = pred.shape[0], pred.shape[1]
        dpred = torch.empty_like(pred)
        scratch = torch.empty(4 + 4 * B, dtype=torch.float32, device=pred.device)      # [0:4] the result, the rest per-clip sums (kasf.h)
        lib = _lib.load()
        _lib.check(lib.kasf_loss3(pred.data_ptr(), target.data_ptr(), dpred.data_ptr(), scratch.data_ptr(), scratch.numel(), B, T, float(lambda_n), float(lambda_v),
                                  1.0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        losses = scratch[:4]
        ctx.save_for_backward(dpred)
        ctx.mark_non_differentiable(losses)
        return losses[0].clone(), losses

    @staticmethod
    def backward(ctx, g_total, _g_parts):
        (dpred,) = ctx.saved_tensors
        return dpred * g_total, None, None, None


def loss3(pred: torch.Tensor, target: torch.Tensor, lambda_n_mpjpe: float = 0.5, lambda_velocity: float = 20.0):
    """Returns (total, parts) with parts = [total, mpjpe, n_mpjpe, velocity] (device tensor, no host sync).
    total = mpjpe + lambda_n * n_mpjpe + lambda_v * velocity (configs/*.yaml:30-31)."""
    return _Loss3.apply(pred, target, lambda_n_mpjpe, lambda_velocity)


# the reference's loss_record_names_complete (train_and_evaluate_sp.py:335) with loss_total first: the layout of loss7's parts
LOSS7_NAMES = ("loss_total", "loss_mpjpe", "loss_n_mpjpe", "loss_velocity", "loss_limb_len_var", "loss_limb_len", "loss_limb_len_cos_simi",
               "loss_limb_len_cos_simi_velocity")


class _Loss7(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, *lambdas):
        if not pred.is_cuda or not target.is_cuda:
            raise RuntimeError("kasportsformer_amd.loss7 runs on the GPU only")
        pred, target = pred.contiguous().float(), target.contiguous().float()
        if pred.dim() != 4 or tuple(pred.shape[2:]) != (17, 3) or pred.shape != target.shape:
            raise ValueError(f"loss7: pred and target must be [B,T,17,3] of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
        B, T = pred.shape[0], pred.shape[1]
        dpred = torch.empty_like(pred)
        scratch = torch.empty(8 + 8 * B, dtype=torch.float32, device=pred.device)      # [0:8] the result, the rest per-clip sums (kasf.h)
        lam = (C.c_float * 6)(*[float(v) for v in lambdas])
        lib = _lib.load()
        with torch.cuda.device(pred.device):
            _lib.check(lib.kasf_loss7(pred.data_ptr(), target.data_ptr(), dpred.data_ptr(), scratch.data_ptr(), scratch.numel(), B, T, lam, 1.0,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        losses = scratch[:8]
        ctx.save_for_backward(dpred)
        ctx.mark_non_differentiable(losses)
        return losses[0].clone(), losses

    @staticmethod
    def backward(ctx, g_total, _g_parts):
        (dpred,) = ctx.saved_tensors
        return (dpred * g_total, None) + (None,) * 6


def loss7(pred: torch.Tensor, target: torch.Tensor, lambda_n_mpjpe: float = 0.5, lambda_velocity: float = 20.0, lambda_limb_len_var: float = 0.0,
          lambda_limb_len: float = 0.0, lambda_limb_cos_simi: float = 0.0, lambda_limb_cos_simi_velocity: float = 0.0):
    """The reference's complete loss (train_and_evaluate_sp.py:216-220) and its gradient in one launch.  Returns (total, parts) with parts laid out as
    LOSS7_NAMES = [total, mpjpe, n_mpjpe, velocity, limb_len_var, limb_len, cos_simi, cos_simi_velocity] (device tensor, no host sync); all seven parts are
    computed whatever the lambdas (configs yaml :29-35) are.  With the four new lambdas zero the total, parts[:4] and the gradient are loss3's bits."""
    return _Loss7.apply(pred, target, lambda_n_mpjpe, lambda_velocity, lambda_limb_len_var, lambda_limb_len, lambda_limb_cos_simi,
                        lambda_limb_cos_simi_velocity)
