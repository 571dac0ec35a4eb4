"""Drop-in for the reference's ``solver/lr_scheduler.py``: ``WarmupMultiStepLR(optimizer, milestones, gamma=0.1,
warmup_factor=1/3, warmup_iters=500, warmup_method="linear", last_epoch=-1)``, the schedule of stage 2.

At ``last_epoch = t`` every group's learning rate is
  base_lr * f(t) * gamma ** (number of milestones <= t)
  f(t) = 1 for t >= warmup_iters, else warmup_factor ('constant') or warmup_factor * (1 - t / warmup_iters) + t / warmup_iters
  ('linear'),
in this order of operations, where base_lr is the group's learning rate at construction (kept as ``initial_lr``).  Construction
takes the first step, as torch's schedulers do: ``last_epoch`` becomes 0 and the groups carry the rate of epoch 0.
``step()`` advances one epoch; ``step(epoch)`` -- what the reference's stage-2 loop calls -- jumps to that epoch.  The loop
steps per EPOCH while SOLVER.STAGE2.WARMUP_ITERS counts 500 of them, so a reference run of 100 epochs never leaves its warm-up;
that is the reference's behaviour and it is kept.  The optimizer is anything with ``param_groups`` (torch.optim.* or
mpreid.ops.TensorOptimizer); nothing here subclasses torch's scheduler.
"""
from bisect import bisect_right


class WarmupMultiStepLR:
    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=500, warmup_method="linear",
                 last_epoch=-1):
        if not list(milestones) == sorted(milestones):
            raise ValueError("Milestones should be a list of increasing integers. Got {}".format(milestones))
        if warmup_method not in ("constant", "linear"):
            raise ValueError("Only 'constant' or 'linear' warmup_method accepted got {}".format(warmup_method))
        self.optimizer = optimizer
        self.milestones, self.gamma = list(milestones), gamma
        self.warmup_factor, self.warmup_iters, self.warmup_method = warmup_factor, warmup_iters, warmup_method
        if last_epoch == -1:
            for group in optimizer.param_groups:
                group.setdefault("initial_lr", group["lr"])
        elif any("initial_lr" not in group for group in optimizer.param_groups):
            raise KeyError("param 'initial_lr' is not specified in param_groups when resuming an optimizer")
        self.base_lrs = [group["initial_lr"] for group in optimizer.param_groups]
        self.last_epoch = last_epoch
        self.step()

    def get_lr(self):
        warmup_factor = 1
        if self.last_epoch < self.warmup_iters:
            if self.warmup_method == "constant":
                warmup_factor = self.warmup_factor
            else:
                alpha = self.last_epoch / self.warmup_iters
                warmup_factor = self.warmup_factor * (1 - alpha) + alpha
        return [base_lr * warmup_factor * self.gamma ** bisect_right(self.milestones, self.last_epoch) for base_lr in self.base_lrs]

    def get_last_lr(self):
        return list(self._last_lr)

    def step(self, epoch=None):
        self.last_epoch = self.last_epoch + 1 if epoch is None else epoch
        self._last_lr = self.get_lr()
        for group, lr in zip(self.optimizer.param_groups, self._last_lr):
            group["lr"] = lr

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, state_dict):
        self.__dict__.update(state_dict)
