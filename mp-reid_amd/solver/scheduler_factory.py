"""Drop-in for the reference's ``solver/scheduler_factory.py``: ``create_scheduler(optimizer, num_epochs, lr_min,
warmup_lr_init, warmup_t, noise_range=None)`` -> an object with ``step(epoch)`` and ``_get_lr(epoch)``.

The reference configures its cosine scheduler (solver/cosine_lr.py:67-93) as ONE cycle over ``num_epochs`` stepped per epoch:
  epoch < warmup_t                 lr = warmup_lr_init + epoch * (base_lr - warmup_lr_init) / warmup_t
  warmup_t <= epoch < num_epochs   lr = lr_min + 0.5 * (base_lr - lr_min) * (1 + cos(pi * epoch / num_epochs))
  epoch >= num_epochs              lr = lr_min
where base_lr is each parameter group's learning rate at construction (kept as ``initial_lr``) and the cosine counts from epoch
0, not from the end of the warm-up.  Construction sets the groups to ``warmup_lr_init`` when there is a warm-up.  The
learning-rate noise of the reference's scheduler is never configured by its callers: a ``noise_range`` other than None is
refused.  The optimizer is anything with ``param_groups`` (torch.optim.* or mpreid.ops.PromptAdam).
"""
import math


class CosineOneCycle:
    def __init__(self, optimizer, num_epochs, lr_min, warmup_lr_init, warmup_t):
        if num_epochs <= 0 or lr_min < 0 or warmup_t < 0:
            raise ValueError("create_scheduler: num_epochs > 0, lr_min >= 0 and warmup_t >= 0")
        self.optimizer = optimizer
        self.t_initial, self.lr_min, self.warmup_lr_init, self.warmup_t = num_epochs, lr_min, warmup_lr_init, warmup_t
        for group in optimizer.param_groups:
            group.setdefault("initial_lr", group["lr"])
        self.base_values = [group["initial_lr"] for group in optimizer.param_groups]
        if warmup_t:
            self.warmup_steps = [(v - warmup_lr_init) / warmup_t for v in self.base_values]
            self._set([warmup_lr_init] * len(self.base_values))
        else:
            self.warmup_steps = [1 for _ in self.base_values]
            self._set(self.base_values)

    def _set(self, values):
        for group, v in zip(self.optimizer.param_groups, values):
            group["lr"] = v

    def _get_lr(self, t):
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * s for s in self.warmup_steps]
        if t >= self.t_initial:
            return [self.lr_min for _ in self.base_values]
        return [self.lr_min + 0.5 * (v - self.lr_min) * (1 + math.cos(math.pi * t / self.t_initial)) for v in self.base_values]

    def step(self, epoch, metric=None):
        self._set(self._get_lr(epoch))

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, state_dict):
        self.__dict__.update(state_dict)


def create_scheduler(optimizer, num_epochs, lr_min, warmup_lr_init, warmup_t, noise_range=None):
    if noise_range is not None:
        raise NotImplementedError("create_scheduler: learning-rate noise (noise_range) is not implemented; the reference's "
                                  "training scripts pass None")
    return CosineOneCycle(optimizer, num_epochs, lr_min, warmup_lr_init, warmup_t)
