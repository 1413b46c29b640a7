"""The learning-rate schedule of the reference's training scripts, as a list (host only).

``train_denoising_syn.py:77-85,260`` wraps ``CosineAnnealingLR(T_max=epochs - warmup_epochs, eta_min=lr_min)`` in
``GradualWarmupScheduler(multiplier=1, total_epoch=warmup_epochs)`` and calls ``scheduler.step()`` once per epoch.  What the optimizer then
sees is NOT the textbook warm-up + cosine curve: at the hand-over the wrapper asks the cosine scheduler for a rate without stepping it, so
the cosine recursion runs once with its epoch counter at 0 -- ``(1 + cos 0) / (1 + cos(-pi / T))`` times the current rate -- and the first
epoch after the warm-up OVERSHOOTS the base rate; the epoch after it is back on the curve.  A run resumed from a reference checkpoint
expects exactly these values, so the recursion is restated here (nothing is imported from the reference) and pinned to the reference's own
output by tests/golden/lr_schedule.json.
"""
from __future__ import annotations

import math
from typing import List


def warmup_cosine(lr: float, lr_min: float, epochs: int, warmup_epochs: int) -> List[float]:
    """One learning rate per epoch, ``epochs`` of them: the rate the reference's optimizer holds DURING epoch ``e`` (0-based).  Resuming at
    epoch ``e`` means indexing the list (the reference replays ``scheduler.step()`` ``e`` times, which gives the same values).

    Every line is the reference's own double expression, in its order of operations, so the values are the same doubles."""
    for name, v in (("epochs", epochs), ("warmup_epochs", warmup_epochs)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} {v!r}: an integer is expected")
    epochs, warmup = int(epochs), int(warmup_epochs)
    if warmup < 0 or epochs <= warmup:
        raise ValueError(f"epochs {epochs}, warmup_epochs {warmup}: 0 <= warmup_epochs < epochs is expected (T_max = epochs - warmup_epochs)")
    base, eta_min = float(lr), float(lr_min)
    t_max = epochs - warmup
    out: List[float] = []
    cur = base                                    # the optimizer's group["lr"]
    for e in range(epochs):
        if e + 1 <= warmup:
            cur = base * (float(e + 1) / warmup)                       # the wrapper's own branch (multiplier == 1)
        else:
            k = e - warmup                        # the cosine scheduler's last_epoch: 0 at the hand-over (asked, not stepped), then 1, 2, ...
            if (k - 1 - t_max) % (2 * t_max) == 0:
                cur = cur + (base - eta_min) * (1 - math.cos(math.pi / t_max)) / 2
            else:
                cur = (1 + math.cos(math.pi * k / t_max)) / (1 + math.cos(math.pi * (k - 1) / t_max)) * (cur - eta_min) + eta_min
        out.append(cur)
    return out


def cosine(lr: float, lr_min: float, epochs: int) -> List[float]:
    """One learning rate per epoch, ``epochs`` of them: what ``CosineAnnealingLR(T_max=epochs, eta_min=lr_min)`` gives the optimizer DURING
    epoch ``e`` with one ``scheduler.step()`` per epoch (train_SISR.py:98-101, 324).  torch evaluates the schedule by its recursion, not by
    the closed form, and the two differ in the last bits; the recursion is restated here in its order of operations, so the values are the
    same doubles.  Resuming at epoch ``e`` means indexing the list (the reference steps the scheduler ``e`` times, :118-119)."""
    if isinstance(epochs, bool) or int(epochs) != epochs or int(epochs) < 1:
        raise ValueError(f"epochs {epochs!r}: a positive integer is expected")
    t_max = int(epochs)
    base, eta_min = float(lr), float(lr_min)
    out: List[float] = [base]
    cur = base
    for k in range(1, t_max):                     # the scheduler's last_epoch
        if (k - 1 - t_max) % (2 * t_max) == 0:
            cur = cur + (base - eta_min) * (1 - math.cos(math.pi / t_max)) / 2
        else:
            cur = (1 + math.cos(math.pi * k / t_max)) / (1 + math.cos(math.pi * (k - 1) / t_max)) * (cur - eta_min) + eta_min
        out.append(cur)
    return out
