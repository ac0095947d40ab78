"""Per-subject voxel head and the projector builder, HIP-backed.

API mirror of /root/reference/modeling_utils/modeling_utils/models/common.py:
  * `SubjectLayers(in_channels, out_channels, n_subjects, bias, init_id, average_subjects)`
    with parameters `weights [S, C, D]`, `bias [S, D]` and `forward(x[B, C, T], subjects) -> [B, D, T]`
    (common.py:14-71);
  * `MlpConfig(...).build(input_size, output_size)` (common.py:86-141) -- on the default path
    `hidden_sizes` is None and it returns a bare `nn.Linear` (common.py:124-128); with hidden sizes it returns `Mlp`, an
    `nn.Sequential` of stock torch modules in the layout of the `torchvision.ops.MLP` the reference returns (common.py:130-141):
    per hidden size Linear, norm (if set), activation, Dropout; then the last Linear and a Dropout.  The layout is restated from
    torchvision's source (torchvision is not a dependency): `state_dict()` keys `0.weight, 0.bias, 1.weight, 1.bias, 4.weight, ...`
    with a norm and `0.*, 3.*, ...` without one.  `Mlp.forward` runs LayerNorm / GELU, ReLU, ELU, identity blocks on the GPU through
    HIP (bf16 MFMA GEMM per Linear, tribe_norm_act_fwd / _bwd in between) and everything else through the stock modules.

Two deliberate differences from the reference's `MlpConfig.build`:
  * the reference appends `output_size` to the config's own `hidden_sizes` list on every call (common.py:131-132), so a second
    `build` of the same config grows the network; here `build` leaves the config as it is;
  * `norm_layer="unit"` is a KeyError inside the reference's build (its table has no such entry); here it is a ValueError.

Differences that do not change results: the reference gathers one [C, D] weight copy per
sample (`index_select`, common.py:61) and runs a batched einsum; here one grouped MFMA GEMM
reads each subject's packed bf16 weights in place (tribe_voxel_head_fwd).
"""

from __future__ import annotations

import typing as tp
import weakref

import pydantic
import torch
from torch import nn

from tribe_hip import ops

from .._pack import PackCache, f32c


class SubjectLayers(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, n_subjects: int, bias: bool = False, init_id: bool = False,
                 average_subjects: bool = False):
        super().__init__()
        self.weights = nn.Parameter(torch.empty(n_subjects, in_channels, out_channels))
        self.bias = nn.Parameter(torch.empty(n_subjects, out_channels)) if bias else None
        with torch.no_grad():
            if init_id:
                if in_channels != out_channels:
                    raise ValueError("in_channels and out_channels must be the same for identity initialization.")
                self.weights[:] = torch.eye(in_channels)[None]
                if self.bias is not None:
                    self.bias.zero_()
            else:
                self.weights.normal_()
                if self.bias is not None:
                    self.bias.normal_()
            self.weights *= 1 / in_channels**0.5
            if self.bias is not None:
                self.bias *= 1 / in_channels**0.5
        self.average_subjects = average_subjects
        self._packs = PackCache()

    # -- packed parameter views -------------------------------------------------------
    def packed(self) -> tuple[torch.Tensor, torch.Tensor | None]:
        def build():
            w = f32c(self.weights)
            b = None if self.bias is None else f32c(self.bias)
            if self.average_subjects:  # common.py:56-59: one shared head = mean over subjects
                w = w.mean(dim=0, keepdim=True)
                b = None if b is None else b.mean(dim=0, keepdim=True)
            return ops.pack_subject_weights(w), b

        return self._packs.get("w", [self.weights, self.bias], build)

    def check_subjects(self, subjects: torch.Tensor) -> torch.Tensor:
        n = self.weights.shape[0]
        # common.py:53-55.  The reference's assert costs a device->host sync on every forward; the verdict is
        # remembered for the very same tensor object (weak reference + version counter), so re-running a batch
        # that was already validated does not synchronise again.
        seen = getattr(self, "_checked", None)
        if seen is None or seen[0]() is not subjects or seen[1] != subjects._version:
            lo, hi = (int(v) for v in torch.aminmax(subjects))    # one device->host sync for both bounds
            assert hi < n, "Subject index higher than number of subjects used to initialize the weights."
            if lo < 0:   # the reference's index_select / nn.Embedding raise on a negative id; the kernels gather unchecked
                raise IndexError(f"index out of range in self: subject id {lo} < 0")
            self._checked = (weakref.ref(subjects), subjects._version)
        subjects = subjects.flatten().to(torch.int64)
        if self.average_subjects:
            subjects = torch.zeros_like(subjects)
        return subjects.contiguous()

    def forward_tokens(self, x_btc: torch.Tensor, subjects: torch.Tensor) -> torch.Tensor:
        """x bf16 [B, T, C_pad] (token-major, as the encoder leaves it) -> f32 [B, D, T]."""
        w_packed, bias = self.packed()
        return ops.voxel_head(x_btc, w_packed, bias, self.check_subjects(subjects), self.weights.shape[2])

    def forward(self, x: torch.Tensor, subjects: torch.Tensor) -> torch.Tensor:
        """Reference signature: x [B, C, T] (a transposed view of [B, T, C] at model.py:117)."""
        B, C, T = x.shape
        if C != self.weights.shape[1]:
            raise ValueError(f"SubjectLayers: expected {self.weights.shape[1]} channels, got {C}")
        # pack_features is exactly the cast + "b c t -> b t c" relayout needed here (L = 1)
        xt = ops.pack_features(x.contiguous(), layer_mean=False).view(B, T, -1)
        return self.forward_tokens(xt, subjects)

    def __repr__(self) -> str:
        S, C, D = self.weights.shape
        return f"SubjectLayers({C}, {D}, {S})"


class MlpConfig(pydantic.BaseModel):
    model_config = pydantic.ConfigDict(extra="forbid")
    name: tp.Literal["Mlp"] = "Mlp"
    input_size: int | None = None
    hidden_sizes: list[int] | None = None
    norm_layer: tp.Literal["layer", "batch", "instance", "unit", None] = None
    activation_layer: tp.Literal["relu", "gelu", "elu", "prelu", None] = "relu"
    bias: bool = True
    dropout: float = 0.0
    # Not in the reference: who runs an ACTIVE dropout (training, p > 0) of the returned Mlp on the GPU.  "torch": the stock f32 modules
    # with torch's generator (masks and route as they always were); "hip": the HIP route with counter-based masks (Mlp docstring)
    dropout_backend: tp.Literal["torch", "hip"] = "torch"

    def build(self, input_size: int | None = None, output_size: int | None = None) -> nn.Module:
        input_size = self.input_size if input_size is None else input_size
        assert input_size is not None, "input_size cannot be None."
        if not self.hidden_sizes:
            assert output_size is not None, "output_size cannot be None if hidden_sizes is empty."
            # parameter holder; FmriEncoder runs it through tribe_projector_fwd
            return nn.Linear(input_size, output_size)
        if self.norm_layer not in _NORMS:
            raise ValueError(f"MlpConfig: norm_layer={self.norm_layer!r} has no module (the reference raises KeyError here)")
        sizes = list(self.hidden_sizes) + ([output_size] if output_size is not None else [])   # a copy: the config is not mutated
        norm, act = _NORMS[self.norm_layer], _ACTIVATIONS[self.activation_layer]
        layers: list[nn.Module] = []
        width = input_size
        for h in sizes[:-1]:
            layers.append(nn.Linear(width, h, bias=self.bias))
            if norm is not None:
                layers.append(norm(h))
            layers += [act(), nn.Dropout(self.dropout)]
            width = h
        layers += [nn.Linear(width, sizes[-1], bias=self.bias), nn.Dropout(self.dropout)]
        if self.dropout_backend == "hip" and not 0.0 <= self.dropout < 1.0:
            raise ValueError(f"MlpConfig: dropout_backend='hip' needs 0 <= dropout < 1, got {self.dropout}")
        return Mlp(layers, self.norm_layer, self.activation_layer, self.dropout, self.dropout_backend)


_NORMS: dict[str | None, tp.Any] = {"layer": nn.LayerNorm, "batch": nn.BatchNorm1d, "instance": nn.InstanceNorm1d, None: None}
_ACTIVATIONS: dict[str | None, tp.Any] = {"relu": nn.ReLU, "gelu": nn.GELU, "elu": nn.ELU, "prelu": nn.PReLU, None: nn.Identity}


MLP_OUT_BLOCK = 0xFFFF   # the block number of an Mlp's output dropout in its site numbering (hidden blocks count from 0)


def draw_dropout_key() -> int:
    """One 63-bit key of the counter-based dropout masks from torch's default CPU generator (torch.manual_seed reproduces it)."""
    return int(torch.randint(0, 2**63 - 1, (1,), dtype=torch.int64).item())


class Mlp(nn.Sequential):
    """What `MlpConfig.build` returns for a non-empty `hidden_sizes`: stock modules in torchvision.ops.MLP's order (see the module
    docstring), so parameters, `state_dict()` and the CPU forward are those of the reference's module.

    forward(x[..., in], f32 or bf16) -> f32 [..., out] has two routes:
      * HIP: x on the GPU, norm None or "layer", activation relu / gelu / elu / None, dropout inactive (p == 0 or eval mode) or
        dropout_backend == "hip".  Every Linear is the bf16 MFMA GEMM with f32 output, norm + activation one row kernel
        (modeling_utils.autograd.NormAct); with grad enabled the route is differentiable through the HIP backward kernels.
      * stock: everything else runs nn.Sequential.forward unchanged (CPU tensors, "batch" / "instance" norms, PReLU, active dropout
        under dropout_backend == "torch").
    `hip_calls` / `stock_calls` count the forwards each route served.

    Active dropout on the HIP route (dropout_backend "hip", training, p > 0) stands where torchvision's Dropout modules stand: after every
    hidden activation, on the bf16 operand [M, H_pad64] over its H logical columns, and after the last Linear on its f32 output
    (tribe_dropout_apply, in place on tensors the route owns; the backward applies the same mask to the gradient).  `forward` draws one
    64-bit key per call from torch's default CPU generator and keeps it as `last_dropout_key`; hidden block i uses site
    `dropout_site + i`, the output `dropout_site + MLP_OUT_BLOCK`.  The masks are not torch's: a different stream, and a dropped
    element is +0.0 whatever it held."""

    def __init__(self, layers: tp.Sequence[nn.Module], norm_layer: str | None, activation_layer: str | None, dropout: float,
                 dropout_backend: str = "torch"):
        super().__init__(*layers)
        self.norm_layer, self.activation_layer, self.dropout, self.dropout_backend = norm_layer, activation_layer, dropout, dropout_backend
        self.hip_calls = self.stock_calls = 0
        self.dropout_site = 0                       # site of hidden block 0 (FmriEncoder numbers its projectors and heads: model.py)
        self.last_dropout_key: int | None = None

    def hip_supported(self) -> bool:
        return (self.norm_layer in (None, "layer") and self.activation_layer in ops.NORM_ACT_ACTS
                and (self.dropout == 0 or not self.training or self.dropout_backend == "hip"))

    def hip_dropout_active(self) -> bool:
        return self.dropout_backend == "hip" and self.dropout > 0 and self.training

    def blocks(self) -> tuple[list[tuple[nn.Linear, nn.LayerNorm | None]], nn.Linear]:
        """([(Linear, its LayerNorm or None) per hidden size], the last Linear)."""
        mods = list(self)
        linears = [i for i, m in enumerate(mods) if isinstance(m, nn.Linear)]
        hidden = [(mods[i], mods[i + 1] if isinstance(mods[i + 1], nn.LayerNorm) else None) for i in linears[:-1]]
        return hidden, mods[linears[-1]]

    def hidden_operand(self, packed: torch.Tensor, input_grad: bool = False, drop_key: int | None = None) -> torch.Tensor:
        """The hidden blocks on a packed bf16 [M, K_pad64] input -> the bf16 [M, H_pad64] operand of the last Linear.  input_grad: the
        input itself needs a gradient (a feature does not: then the first Linear computes none).  drop_key: the pass key of an active
        HIP dropout (None: no dropout)."""
        from .. import autograd as ag

        a = packed
        for i, (lin, norm) in enumerate(self.blocks()[0]):
            if i == 0 and not input_grad:
                z = ag.ProjectorFuse.apply(a, lin.weight, lin.bias)
            else:
                z = ag.Linear.apply(a, lin.weight, lin.bias, None, None, True)
            if norm is None:
                a = ag.NormAct.apply(z, None, None, 0.0, self.activation_layer, False)
            else:
                a = ag.NormAct.apply(z, norm.weight, norm.bias, norm.eps, self.activation_layer, True)
            if drop_key is not None:
                a = ag.Dropout.apply(a, self.dropout, drop_key, self.dropout_site + i, lin.out_features, True)
        return a

    def output(self, operand: torch.Tensor, drop_key: int | None = None) -> torch.Tensor:
        """The last Linear on hidden_operand's result -> f32 [M, out], followed by the output dropout when drop_key is given."""
        from .. import autograd as ag

        last = self.blocks()[1]
        out = ag.Linear.apply(operand, last.weight, last.bias, None, None, True)
        if drop_key is not None:
            out = ag.Dropout.apply(out, self.dropout, drop_key, self.dropout_site + MLP_OUT_BLOCK, None, True)
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not (x.is_cuda and self.hip_supported()):
            self.stock_calls += 1
            return super().forward(x)
        from .. import autograd as ag

        self.hip_calls += 1
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"Mlp: expected an f32 or bf16 input, got {x.dtype}")
        key = None
        if self.hip_dropout_active():
            key = self.last_dropout_key = draw_dropout_key()
        input_grad = torch.is_grad_enabled() and x.requires_grad
        out = self.output(self.hidden_operand(ag.PackRows.apply(x.reshape(-1, x.shape[-1])), input_grad, key), key)
        return out.view(*x.shape[:-1], out.shape[-1])
