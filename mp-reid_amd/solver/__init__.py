"""The stage-1 optimizer and schedule of the reference's ``solver`` package: ``make_optimizer_prompt.make_optimizer_1stage``
and ``scheduler_factory.create_scheduler``."""
