"""KL annealing rules for the native loop (reference: hulc2/utils/kl_callbacks.py:5-60, conf/callbacks/kl_schedule/*.yaml).

Under Lightning the reference's own callbacks run and call `Hulc2.set_kl_beta` every epoch.  `ArenaTrainer` has no callbacks: attach one of
these with `ArenaTrainer.set_kl_schedule(fn)` and call `ArenaTrainer.begin_epoch(epoch)` where an epoch starts.  Each factory returns
`fn(epoch) -> KL weight`, with the reference's edges kept as they are (the one difference: end_epoch <= start_epoch raises ValueError
when the rule is built, where the reference divides by zero or steps from 0 to max):

  * epoch < start_epoch: exactly 0.0;
  * epoch > end_epoch (strictly): exactly max_kl_beta;
  * linear reaches max_kl_beta AT end_epoch; the sigmoid is sigmoid(6) * max_kl_beta there (0.9975...) and jumps to max_kl_beta one epoch later;
  * the sigmoid is evaluated in float32 by torch.sigmoid on (epoch - shift) / (scale / 12), the argument formed in Python floats.
"""
from typing import Callable, Optional

import torch


def constant() -> Callable[[int], Optional[float]]:
    """conf/callbacks/kl_schedule/constant.yaml: the weight is never set — fn returns None and `ArenaTrainer.begin_epoch` then leaves the
    model alone (its configured `kl_beta` keeps going to the kernels by value)."""
    return lambda epoch: None


def _check(start_epoch, end_epoch) -> None:
    """one deviation from the reference, on purpose: its callbacks accept end_epoch <= start_epoch (end < start gives a step from 0 to max by
    the two comparisons, end == start divides by zero at that epoch); here both are refused when the rule is built"""
    if end_epoch <= start_epoch:
        raise ValueError(f"kl_schedule: end_epoch ({end_epoch}) must lie after start_epoch ({start_epoch})")


def linear(start_epoch: int, end_epoch: int, max_kl_beta: float) -> Callable[[int], float]:
    """conf/callbacks/kl_schedule/linear.yaml: a straight ramp from 0 at start_epoch to max_kl_beta at end_epoch"""
    _check(start_epoch, end_epoch)

    def fn(epoch: int) -> float:
        if epoch < start_epoch:
            return 0.0
        if epoch > end_epoch:
            return max_kl_beta
        return max_kl_beta * (epoch - start_epoch) / (end_epoch - start_epoch)      # (this order of operations: the values are compared exactly)
    return fn


def sigmoid(start_epoch: int, end_epoch: int, max_kl_beta: float) -> Callable[[int], float]:
    """conf/callbacks/kl_schedule/sigmoid.yaml: a logistic curve centred between the two epochs that spans sigmoid(-6) .. sigmoid(6) over them"""
    _check(start_epoch, end_epoch)
    width = (end_epoch - start_epoch) / 12
    centre = (end_epoch + start_epoch) / 2

    def fn(epoch: int) -> float:
        if epoch < start_epoch:
            return 0.0
        if epoch > end_epoch:
            return max_kl_beta
        return torch.sigmoid(torch.tensor([(epoch - centre) / width], dtype=torch.float32)).item() * max_kl_beta
    return fn
