"""Test helper: x_transformers' `Decoder` restated on top of the oracle's `Encoder` -- the same module with one mask.  Scores whose key index
exceeds the query index are filled with -finfo(dtype).max before the softmax; parameters, `state_dict` keys and rotary are untouched."""

from __future__ import annotations

import torch

from oracle import xt_encoder


class CausalAttention(xt_encoder.Attention):
    """oracle.xt_encoder.Attention with the causal mask (x_transformers Attend: `sim.masked_fill(causal_mask, -finfo.max)`)."""

    def forward(self, x: torch.Tensor, freqs: torch.Tensor | None, interleaved: bool) -> torch.Tensor:
        B, T, _ = x.shape
        h, d = self.heads, self.dim_head
        q = self.to_q(x).view(B, T, h, d).transpose(1, 2)
        k = self.to_k(x).view(B, T, h, d).transpose(1, 2)
        v = self.to_v(x).view(B, T, h, d).transpose(1, 2)
        if freqs is not None:
            q = xt_encoder.apply_rotary_pos_emb(q, freqs, interleaved)
            k = xt_encoder.apply_rotary_pos_emb(k, freqs, interleaved)
        sim = torch.einsum("bhid,bhjd->bhij", q, k) * self.scale
        future = torch.ones(T, T, dtype=torch.bool, device=x.device).triu(1)          # key j > query i
        sim = sim.masked_fill(future, -torch.finfo(sim.dtype).max)
        attn = sim.softmax(dim=-1, dtype=torch.float64 if sim.dtype == torch.float64 else torch.float32).type(sim.dtype)
        out = torch.einsum("bhij,bhjd->bhid", attn, v)
        out = out.transpose(1, 2).reshape(B, T, h * d)
        return self.to_out(out)


def make_causal(encoder: xt_encoder.Encoder) -> xt_encoder.Encoder:
    """Swap the class of every attention block of an oracle encoder (in place; returns it).  No parameter moves."""
    n = 0
    for _, block, _ in encoder.layers:
        if isinstance(block, xt_encoder.Attention):
            block.__class__ = CausalAttention
            n += 1
    assert n == encoder.depth
    return encoder


def tril_mask(rows: int, T: int, row0: int = 0) -> torch.Tensor:
    """bool [rows, T]: True where column j <= i, i = (row0 + r) % T the query of slab row r of the logical [B * heads * T, T] tensor."""
    i = (torch.arange(rows, dtype=torch.int64) + row0) % T
    return torch.arange(T, dtype=torch.int64)[None, :] <= i[:, None]
