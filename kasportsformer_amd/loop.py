"""The per-epoch training loop that drives the path (train_and_evaluate_sp.py:201-243 / train_and_evaluate_wp.py:187-229).

Same order of operations -- forward, zero_grad, loss, backward, step -- with the four ``.item()`` host synchronisations per step
of the reference replaced by a device-side running sum: the batch-size-weighted averages (what ``AverageMetering`` reports) are read
once per epoch.  The loss is the 3-term one the reference trains with, or its complete 7-term one when any of the four limb lambdas is set.
"""
from __future__ import annotations

import torch

from .functional import LOSS7_NAMES, loss3, loss7


def train_one_epoch(model, train_loader, optimizer, data_parallel=None, lambda_n_mpjpe: float = 0.5, lambda_mpjpe_velocity: float = 20.0,
                    device="cuda", lambda_limb_len_var: float = 0.0, lambda_limb_len: float = 0.0, lambda_limb_cos_simi: float = 0.0,
                    lambda_limb_cos_simi_velocity: float = 0.0) -> dict:
    """One pass over ``train_loader`` (batches ``(x, y)`` like the reference's DataLoader or ``DeviceClipLoader``).  Returns the epoch
    averages ``{'loss_total', 'loss_mpjpe', 'loss_n_mpjpe', 'loss_velocity'}`` weighted by batch size (utils/utilities.py:95-108).
    The lambdas carry the yaml's names (configs yaml :29-35).  With the four limb lambdas at 0 -- every shipped config -- the step is the 3-term ``loss3``;
    with any of them set it is ``loss7`` (train_and_evaluate_sp.py:216-220) and the result carries all eight ``LOSS7_NAMES``."""
    model.train()
    complete = any(float(v) != 0.0 for v in (lambda_limb_len_var, lambda_limb_len, lambda_limb_cos_simi, lambda_limb_cos_simi_velocity))
    sums = torch.zeros(8 if complete else 4, dtype=torch.float64, device=device)
    count = 0
    for x, y in train_loader:
        x, y = x.to(device), y.to(device)
        predict_result = model(x)
        optimizer.zero_grad()
        if complete:
            loss_total, parts = loss7(predict_result, y, lambda_n_mpjpe, lambda_mpjpe_velocity, lambda_limb_len_var, lambda_limb_len, lambda_limb_cos_simi,
                                      lambda_limb_cos_simi_velocity)                           # parts laid out as LOSS7_NAMES
        else:
            loss_total, parts = loss3(predict_result, y, lambda_n_mpjpe, lambda_mpjpe_velocity)    # parts = [total, mpjpe, n_mpjpe, velocity]
        sums += parts.double() * x.shape[0]
        count += x.shape[0]
        loss_total.backward()
        if data_parallel is not None:
            data_parallel.finish_gradients(optimizer)
        optimizer.step()
    avg = (sums / max(count, 1)).cpu().tolist()               # the only host synchronisation of the epoch
    return dict(zip(LOSS7_NAMES, avg))                        # the first four names when the 3-term loss ran
