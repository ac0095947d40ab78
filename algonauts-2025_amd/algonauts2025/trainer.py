"""The fit loop around `BrainModule.training_step`: the part of `lightning.Trainer.fit` the reference's run relies on.

Reference: /root/reference/algonauts2025/main.py:351-405 builds `pl.Trainer(max_epochs, limit_train_batches, strategy=ddp...,
callbacks=[JitterWindows, StochasticWeightAveraging, ...])` and calls `trainer.fit(brain_module, train, val)`; the optimiser and
its `OneCycleLR` schedule come from `configure_optimizers` (pl_module.py:138-144, interval "step").  Lightning is not a dependency
of this build (and loggers, checkpoints, early stopping and progress bars are control plane, out of scope): this class is the
epoch / step / hook ordering only, with the MI355X pieces plugged in -- HipAdam (one launch per step), GradReducer (bucketed
RCCL all-reduce overlapped with backward, one process per GPU) and the HIP weight-averaging kernel behind the SWA callback.
Callbacks receive `(trainer, pl_module)` exactly as Lightning passes them.

`gradient_clip_val` / `gradient_clip_algorithm` carry Lightning's names and documented meaning (`"norm"`: the global L2 norm of all
gradients of the optimiser is clipped to the value with torch's `clip_grad_norm_` rule; `"value"`: every gradient element is clamped to
[-value, value]; `None` or a value <= 0: no clipping).  Lightning is not installed here: this is restated from its documentation and
is "parity unpinned", like `StochasticWeightAveraging`.  Clipping runs after `GradReducer.finish()`, i.e. on the averaged gradients, so
every rank computes the same coefficient.  With `HipAdam` the norm is one streaming read (tribe_grad_norm), its coefficient stays on
the device and the optimiser kernel applies it as it loads each gradient (tribe_adam_step_clipped): `p.grad` is not rewritten.
"""

from __future__ import annotations

import typing as tp

import torch

from .distributed import GradReducer, world


class Trainer:
    def __init__(self, max_epochs: int, callbacks: tp.Sequence[tp.Any] = (), limit_train_batches: int | None = None,
                 device: str | torch.device = "cuda", bucket_bytes: int = 512 << 20, reduce_gradients: bool | None = None,
                 gradient_clip_val: float | None = None, gradient_clip_algorithm: str = "norm") -> None:
        if max_epochs < 1:
            raise ValueError("max_epochs must be >= 1")
        if gradient_clip_algorithm not in ("norm", "value"):
            raise ValueError(f"gradient_clip_algorithm must be 'norm' or 'value', got {gradient_clip_algorithm!r}")
        self.gradient_clip_val = float(gradient_clip_val) if gradient_clip_val is not None and gradient_clip_val > 0 else None
        self.gradient_clip_algorithm = gradient_clip_algorithm
        self.max_epochs, self.callbacks, self.limit_train_batches = max_epochs, list(callbacks), limit_train_batches
        self.device, self.bucket_bytes = device, bucket_bytes
        self.reduce_gradients = reduce_gradients                # None: whenever the process group has more than one rank
        self.current_epoch = 0
        self.global_step = 0
        self.optimizers: list[torch.optim.Optimizer] = []
        self.lr_scheduler: dict[str, tp.Any] | None = None     # {"scheduler", "interval"}: callbacks (SWA) may replace it
        self.train_dataloader: tp.Any = None
        self.reducer: GradReducer | None = None
        self.history: list[dict[str, float]] = []

    def _call(self, hook: str, module: tp.Any) -> None:
        for cb in self.callbacks:
            fn = getattr(cb, hook, None)
            if fn is not None:
                fn(self, module)

    def _n_batches(self, loader: tp.Any) -> int:
        n = len(loader)
        return n if self.limit_train_batches is None else min(n, self.limit_train_batches)

    def _clipped_step(self, opt: torch.optim.Optimizer) -> torch.Tensor | None:
        """The optimiser step under `gradient_clip_val`; returns the total norm (a tensor, not read here) for "norm"."""
        from modeling_utils.optim import HipAdam, clip_grad_norm_, clip_grad_value_, hip_clip_eligible
        from tribe_hip import ops

        params = [p for g in opt.param_groups for p in g["params"]]
        by_norm = self.gradient_clip_algorithm == "norm"
        grads = [p.grad for p in params if p.grad is not None]
        if isinstance(opt, HipAdam) and hip_clip_eligible(grads):        # fused: the step's kernel clips as it loads, p.grad stays
            if by_norm:
                norm, coef = ops.grad_norm(grads, self.gradient_clip_val, 2.0)
                opt.step(grad_scale=coef)
                return norm
            opt.step(grad_clip_value=self.gradient_clip_val)
            return None
        norm = clip_grad_norm_(params, self.gradient_clip_val) if by_norm else clip_grad_value_(params, self.gradient_clip_val)
        opt.step()
        return norm

    @property
    def estimated_stepping_batches(self) -> int:
        return self._n_batches(self.train_dataloader) * self.max_epochs

    def fit(self, module: tp.Any, train_loader: tp.Any, val_loader: tp.Any = None) -> None:
        self.train_dataloader = train_loader
        module.to(self.device)
        module.trainer = self
        built = module.configure_optimizers(total_steps=self.estimated_stepping_batches)
        if isinstance(built, dict):
            self.optimizers, self.lr_scheduler = [built["optimizer"]], built.get("lr_scheduler")
        else:
            self.optimizers, self.lr_scheduler = [built], None
        opt = self.optimizers[0]
        if (world()[1] > 1) if self.reduce_gradients is None else self.reduce_gradients:
            self.reducer = GradReducer([p for g in opt.param_groups for p in g["params"]], bucket_bytes=self.bucket_bytes)
        self._call("on_fit_start", module)
        for epoch in range(self.max_epochs):
            self.current_epoch = epoch
            module.train()
            self._call("on_train_epoch_start", module)
            total, count, grad_norm = 0.0, 0, None
            for i, batch in enumerate(train_loader):
                if i >= self._n_batches(train_loader):
                    break
                if self.reducer is not None:
                    self.reducer.zero_grad()
                else:
                    opt.zero_grad(set_to_none=True)
                loss = module.training_step(batch.to(self.device), i)
                loss.backward()
                if self.reducer is not None:
                    self.reducer.finish()
                if self.gradient_clip_val is None:
                    opt.step()
                else:
                    grad_norm = self._clipped_step(opt)
                if self.lr_scheduler is not None and self.lr_scheduler["interval"] == "step":
                    self.lr_scheduler["scheduler"].step()
                self.global_step += 1
                total, count = total + float(loss.detach()), count + 1
            if self.lr_scheduler is not None and self.lr_scheduler["interval"] == "epoch":
                self.lr_scheduler["scheduler"].step()
            self._call("on_train_epoch_end", module)
            record = {"epoch": epoch, "train/loss": total / max(1, count), "lr": opt.param_groups[0]["lr"]}
            if grad_norm is not None:
                record["grad_norm"] = float(grad_norm)                 # the last step's total norm: the one read of the epoch
            if val_loader is not None:
                module.eval()
                with torch.no_grad():
                    for i, batch in enumerate(val_loader):
                        module.validation_step(batch.to(self.device), i)
                module.on_validation_epoch_end()
            self.history.append(record)
        self.current_epoch = self.max_epochs                   # Lightning leaves the counter one past the last epoch
        self._call("on_train_end", module)
        if self.reducer is not None:
            self.reducer.remove()
            self.reducer = None
