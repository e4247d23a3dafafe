"""The control of the weights' average: torch_ema 0.3's ExponentialMovingAverage as far as the tests need it -- its `update` as the three torch
expressions it runs per parameter tensor (on whatever device the tensors are on), its warm-up rule for the decay, and its state_dict format.
Written from torch_ema's documented behaviour; it shares no code with palettenerf_amd.optim."""
import torch


def decay_at(decay, num_updates):
    """The decay of update number `num_updates` (counted from 1), in Python doubles."""
    return min(decay, (1 + num_updates) / (10 + num_updates))


class ControlEMA:
    def __init__(self, parameters, decay, use_num_updates=True):
        self.parameters = list(parameters)
        self.decay = decay
        self.num_updates = 0 if use_num_updates else None
        self.shadow_params = [p.clone().detach() for p in self.parameters]
        self.collected_params = None

    def update(self):
        decay = self.decay
        if self.num_updates is not None:
            self.num_updates += 1
            decay = decay_at(decay, self.num_updates)
        one_minus_decay = 1.0 - decay
        with torch.no_grad():
            for s_param, param in zip(self.shadow_params, self.parameters):
                tmp = s_param - param
                tmp.mul_(one_minus_decay)
                s_param.sub_(tmp)

    def state_dict(self):
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": self.shadow_params, "collected_params": self.collected_params}
