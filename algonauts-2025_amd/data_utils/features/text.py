"""Llama-3.2 text feature extractor on MI355X HIP kernels.

Mirror of the reference plugin `LLAMA3p2` (/root/reference/data_utils/data_utils/features/text.py:42-256): for
every word, its left context is tokenised (right padding, left truncation, text.py:166-168,226-232), run through
`LlamaModel(..., output_hidden_states=True)` (text.py:236-240) and every hidden state is averaged over the last
`len(word)` non-pad positions (text.py:245-254) -> `[n_layers + 1, hidden]` per word; layer groups are then formed by
`_aggregate_layers` (text.py:129-149).

Here the model forward AND the pooling run in one C call (`tribe_llama_fwd`: RMSNorm, fused q|k|v MFMA GEMM, rotary,
causal grouped-query flash attention, SwiGLU GEMM epilogue, f32 residual stream); only `[B, n_states, hidden]` floats
leave the GPU, where the reference copies every hidden state to the host (text.py:240).

`LLAMA3p2(share_prefixes=True)` runs one forward per RUN of nested contexts instead of one per word (`prefix_groups`,
`HipLlamaModel.forward_windows` -> `tribe_llama_windows_fwd`): exact while each context is a prefix of the next, which ends
where the cap on the context length starts to drop words on the left.  Off by default.

Weights come from any `transformers` LlamaModel / state_dict (names `embed_tokens.weight`,
`layers.N.self_attn.{q,k,v,o}_proj.weight`, `layers.N.mlp.{gate,up,down}_proj.weight`, `layers.N.*layernorm.weight`,
`norm.weight`).  The reference fetches `meta-llama/Llama-3.2-3B` by name; that checkpoint is not available offline, so
parity is tested against the installed `transformers` implementation with random weights (tests/test_gpu_extractors.py).
"""

from __future__ import annotations

import ctypes as C
import math
import typing as tp

import numpy as np
import pydantic
import torch

from tribe_hip import _lib, ops
from tribe_hip._lib import LlamaDesc, LlamaFp8Layer, LlamaLayer

from .extractor_host import ExtractorHost
from .plugin import HbmFeaturePlugin

# Llama-3.2-3B hyper-parameters (public model card; not verifiable offline -> configuration input)
LLAMA_3P2_3B = dict(
    vocab_size=128256, hidden_size=3072, intermediate_size=8192, num_hidden_layers=28, num_attention_heads=24,
    num_key_value_heads=8, head_dim=128, rms_norm_eps=1e-5, max_position_embeddings=131072,
    rope_parameters={"rope_type": "llama3", "rope_theta": 500000.0, "factor": 32.0, "low_freq_factor": 1.0,
                     "high_freq_factor": 4.0, "original_max_position_embeddings": 8192},
)


def rope_inv_freq(head_dim: int, rope: dict[str, tp.Any]) -> torch.Tensor:
    """Inverse frequencies of HF's LlamaRotaryEmbedding: 'default' and 'llama3' (modeling_rope_utils llama3 rule:
    wavelengths above original_ctx / low_freq_factor are divided by `factor`, the band down to
    original_ctx / high_freq_factor is interpolated smoothly)."""
    base = float(rope.get("rope_theta", 10000.0))
    inv = 1.0 / (base ** (torch.arange(0, head_dim, 2, dtype=torch.float32) / head_dim))
    kind = rope.get("rope_type", "default")
    if kind == "default":
        return inv
    if kind != "llama3":
        raise NotImplementedError(f"rope_type {kind!r} is not used by Llama-3.2")
    factor, lo, hi = float(rope["factor"]), float(rope["low_freq_factor"]), float(rope["high_freq_factor"])
    old = float(rope["original_max_position_embeddings"])
    wavelen = 2 * math.pi / inv
    scaled = torch.where(wavelen > old / lo, inv / factor, inv)
    smooth = (old / wavelen - lo) / (hi - lo)
    smoothed = (1 - smooth) * scaled / factor + smooth * scaled
    medium = ~(wavelen < old / hi) & ~(wavelen > old / lo)
    return torch.where(medium, smoothed, scaled)


class HipLlamaModel(ExtractorHost):
    """Packed bf16 weights of a LlamaModel + the forward-with-pooling launcher.  enable_fp8(calibration_ids [B, T]) switches the four
    Linear GEMMs of every layer to e4m3; its amax table columns are qkv in, o_proj in, gate_up in, down in."""

    FORWARD, FP8_LAYER, FP8_FIELDS = "tribe_llama_fwd", LlamaFp8Layer, ("w_qkv", "w_o", "w_gate_up", "w_down")
    FP8_WIDTHS_ERROR = "fp8 path: hidden_size, num_attention_heads * head_dim and intermediate_size must be multiples of 128"

    def __init__(self, config: tp.Any, state_dict: dict[str, torch.Tensor], device: str | torch.device = "cuda"):
        super().__init__(config, {k.removeprefix("model."): v for k, v in state_dict.items()}, device)
        g, f32, own = self.cfg, self.f32, self.own
        self.dim, self.depth, self.inter = g("hidden_size"), g("num_hidden_layers"), g("intermediate_size")
        self.heads_q, self.heads_kv = g("num_attention_heads"), g("num_key_value_heads")
        try:
            self.dim_head = g("head_dim") or self.dim // self.heads_q
        except (KeyError, AttributeError):
            self.dim_head = self.dim // self.heads_q
        self.eps, self.vocab = float(g("rms_norm_eps")), g("vocab_size")
        try:
            rope = g("rope_parameters")
        except (KeyError, AttributeError):
            rope = None
        self.inv_freq = rope_inv_freq(self.dim_head, dict(rope) if rope else {"rope_type": "default", "rope_theta": 10000.0})
        self.fp8_widths = (self.dim, self.heads_q * self.dim_head, self.inter)
        self.embed = f32("embed_tokens.weight").to(torch.bfloat16).contiguous()  # bf16 table: 0.79 GB for the 3B vocab
        self.layers = (LlamaLayer * max(self.depth, 1))()
        self.packs: list[tuple[torch.Tensor, ...]] = []      # bf16 (qkv, o, gate_up, down) per layer, the source of the fp8 packs
        for i in range(self.depth):
            p = f"layers.{i}."
            L = self.layers[i]
            wqkv = torch.cat([f32(p + "self_attn.q_proj.weight"), f32(p + "self_attn.k_proj.weight"), f32(p + "self_attn.v_proj.weight")])
            gate, up = f32(p + "mlp.gate_proj.weight"), f32(p + "mlp.up_proj.weight")
            gate_up = torch.stack([gate, up], dim=1).reshape(2 * self.inter, self.dim).contiguous()  # rows: g0, u0, g1, u1, ...
            packs = (ops.pack_weight(wqkv), ops.pack_weight(f32(p + "self_attn.o_proj.weight")), ops.pack_weight(gate_up),
                     ops.pack_weight(f32(p + "mlp.down_proj.weight")))
            self.packs.append(packs)
            L.input_norm_w = own(f32(p + "input_layernorm.weight"))
            L.w_qkv, L.w_o, L.w_gate_up, L.w_down = (t.data_ptr() for t in packs)
            L.post_norm_w = own(f32(p + "post_attention_layernorm.weight"))
            del wqkv, gate, up, gate_up
        self.final_norm = f32("norm.weight")
        del self._sd
        self._tabs: dict[int, tuple[torch.Tensor, torch.Tensor]] = {}

    def _tables(self, T: int) -> tuple[torch.Tensor, torch.Tensor]:
        if T not in self._tabs:
            freqs = torch.outer(torch.arange(T, dtype=torch.float32), self.inv_freq)  # attention_scaling == 1 for llama3
            self._tabs[T] = (freqs.cos().to(self.device).contiguous(), freqs.sin().to(self.device).contiguous())
        return self._tabs[T]

    def _calibrate(self, calibration_ids: torch.Tensor, amax: torch.Tensor) -> None:
        B, T = calibration_ids.shape
        zeros, full = torch.zeros(B, dtype=torch.int64), torch.full((B,), T, dtype=torch.int64)
        self.forward_pooled(calibration_ids, zeros, full, _amax=amax)

    def _describe(self, input_ids: torch.Tensor) -> tuple[LlamaDesc, torch.Tensor]:
        """The descriptor of one forward over input_ids [B, T], but for what is pooled, and the device ids it points to."""
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        B, T = ids.shape
        if int(ids.min()) < 0 or int(ids.max()) >= self.vocab:
            raise ValueError("token id outside the vocabulary")
        cos, sin = self._tables(T)
        d = LlamaDesc()
        d.B, d.T = B, T
        d.dim, d.depth, d.heads_q, d.heads_kv, d.dim_head, d.inter = self.dim, self.depth, self.heads_q, self.heads_kv, self.dim_head, self.inter
        d.rms_eps = self.eps
        d.embed, d.embed_dtype, d.vocab = self.embed.data_ptr(), _lib.BF16, self.vocab
        d.layers_host = C.cast(self.layers, C.POINTER(LlamaLayer))
        d.final_norm_w = self.final_norm.data_ptr()
        d.cos_tab, d.sin_tab = cos.data_ptr(), sin.data_ptr()
        d.ids = ids.data_ptr()
        return d, ids

    def forward_pooled(self, input_ids: torch.Tensor, pool_start: torch.Tensor, pool_len: torch.Tensor, fp8: bool | None = None,
                       _amax: torch.Tensor | None = None) -> torch.Tensor:
        """input_ids int64 [B, T] (right padded); returns f32 [n_layers + 1, B, dim]: every hidden state averaged over
        positions [pool_start[b], pool_start[b] + pool_len[b]).  fp8: None = use the e4m3 GEMMs when enable_fp8() has run."""
        d, ids = self._describe(input_ids)
        start = pool_start.to(device=self.device, dtype=torch.int64).contiguous()
        length = pool_len.to(device=self.device, dtype=torch.int64).contiguous()
        d.pool_start, d.pool_len = start.data_ptr(), length.data_ptr()
        states = torch.empty(self.depth + 1, ids.shape[0], self.dim, dtype=torch.float32, device=self.device)
        return self._launch(d, states, fp8, _amax, "forward_pooled")

    def forward_windows(self, input_ids: torch.Tensor, win_row: tp.Any, win_start: tp.Any, win_len: tp.Any,
                        fp8: bool | None = None) -> torch.Tensor:
        """The same forward pooled over a LIST of W windows: window w averages positions [win_start[w], win_start[w] + win_len[w]) of
        row win_row[w]; several windows may share a row, overlap or repeat.  Returns f32 [n_layers + 1, W, dim].  With the causal mask
        and right padding, position t sees tokens 0..t only, so one row holding the longest of a run of nested contexts gives the
        states of every shorter one (see prefix_groups).  Windows are validated here, on the host, before anything is launched."""
        row, start, length = (torch.as_tensor(t, dtype=torch.int64).cpu().flatten() for t in (win_row, win_start, win_len))
        B, T = input_ids.shape
        W = row.numel()
        if W == 0 or start.numel() != W or length.numel() != W:
            raise ValueError(f"forward_windows: win_row, win_start and win_len must have one length > 0, got {W} / {start.numel()} / {length.numel()}")
        if int(row.min()) < 0 or int(row.max()) >= B:
            raise ValueError(f"forward_windows: win_row outside [0, {B})")
        if int(start.min()) < 0 or int(length.min()) < 0 or int((start + length).max()) > T:
            raise ValueError(f"forward_windows: a window leaves [0, {T})")
        d, ids = self._describe(input_ids)
        wins = torch.stack([row, start, length]).to(self.device)   # one upload: rows 0 / 1 / 2 of an int64 [3, W]
        states = torch.empty(self.depth + 1, W, self.dim, dtype=torch.float32, device=self.device)
        extra = (wins[0].data_ptr(), wins[1].data_ptr(), wins[2].data_ptr(), W)
        return self._launch(d, states, fp8, None, "forward_windows", forward="tribe_llama_windows_fwd", extra=extra)


def prefix_groups(token_rows: tp.Sequence[tp.Sequence[int]]) -> list[tuple[list[int], list[int]]]:
    """Runs of nested contexts.  Walks the real (unpadded) token rows in the order given and returns, per group, (the group's longest
    row, the indices of its members).  A row joins the current group when the group's longest row is a prefix of it (it becomes the
    longest: the next word of a timeline) or when it is itself a prefix of the longest row (a repeat, a shorter context, an empty
    one); any other row opens a new group.  The test is on token ids, not on strings: a tokenizer need not map a string prefix to a
    token prefix.  Members of a group are consecutive inputs, and every member's tokens sit at the same positions in the longest row
    as in its own, so `word_pool_windows` of the member addresses the longest row unchanged."""
    groups: list[tuple[list[int], list[int]]] = []
    for i, r in enumerate(token_rows):
        row = [int(t) for t in r]
        if groups:
            longest, members = groups[-1]
            n = len(longest)
            if len(row) >= n and row[:n] == longest:
                groups[-1] = (row, members + [i])
                continue
            if len(row) < n and longest[:len(row)] == row:
                members.append(i)
                continue
        groups.append((row, [i]))
    return groups


def word_pool_windows(input_ids: torch.Tensor, target_words: tp.Sequence[str], pad_id: int) -> tuple[torch.Tensor, torch.Tensor]:
    """text.py:245-252: n_pads = #tokens equal to pad_id; keep [:-n_pads]; average the last len(word) positions
    (python slicing semantics: a window longer than the sequence -- or len(word) == 0 -- takes everything)."""
    ids = input_ids.cpu()
    T = ids.shape[1]
    n_real = T - (ids == pad_id).sum(dim=1)
    k = torch.tensor([len(w) for w in target_words], dtype=torch.int64)
    k = torch.where((k == 0) | (k > n_real), n_real, k)
    return (n_real - k).to(torch.int64), k.to(torch.int64)


class LLAMA3p2(HbmFeaturePlugin):
    """The reference's text feature (text.py:42-256) on the HIP Llama forward: fields `name`, `layers`, `layer_aggregation`,
    `device`, `infra`; `prepare(events)`, `__call__(events, start, duration, trigger) -> Tensor[L, D, T]` and
    `_get_data(events) -> Iterator[np.ndarray [n_states, hidden]]` (data_utils/features/plugin.py).  One latent per Word
    event (item uid `text_context`, text.py:199-203), held for the word's duration."""

    name: tp.Literal["LLAMA3p2"] = "LLAMA3p2"
    batch_size: int = 8                                   # text.py:212 (DataLoader batch of contexts)
    pretrained: str = "meta-llama/Llama-3.2-3B"           # text.py:166-173; resolved from the local HF cache only
    share_prefixes: bool = False                          # one forward per run of nested contexts (a schedule, not a result): see extract
    _EVENT_TYPE: tp.ClassVar[str] = "Word"
    _KIND: tp.ClassVar[str] = "words"
    _model: tp.Any = pydantic.PrivateAttr(default=None)
    _tokenizer: tp.Any = pydantic.PrivateAttr(default=None)

    @classmethod
    def _exclude_from_cls_uid(cls) -> list[str]:
        return super()._exclude_from_cls_uid() + ["share_prefixes"]

    def _exclude_from_cache_uid(self) -> list[str]:
        # a field at its default never enters a uid, so the schedule needs excluding only where it is set: a default plugin keeps the
        # reference's list (text.py:157-158) as it is
        return super()._exclude_from_cache_uid() + (["share_prefixes"] if self.share_prefixes else [])

    def attach(self, model: HipLlamaModel, tokenizer: tp.Any) -> "LLAMA3p2":
        """Provide weights + tokenizer explicitly (offline use: the reference fetches them by name)."""
        self._model, self._tokenizer = model, tokenizer
        return self

    @property
    def model(self) -> HipLlamaModel:
        if self._model is None:
            from transformers import AutoModel, AutoTokenizer  # local cache only: there is no network on the GPU boxes

            tok = AutoTokenizer.from_pretrained(self.pretrained, truncation_side="left", local_files_only=True)
            hf = AutoModel.from_pretrained(self.pretrained, local_files_only=True)
            if tok.pad_token is None:
                tok.pad_token = tok.eos_token
            self._model, self._tokenizer = HipLlamaModel(hf.config, hf.state_dict()), tok
        return self._model

    @property
    def tokenizer(self) -> tp.Any:
        self.model
        return self._tokenizer

    def _item_uid(self, event: tp.Any) -> str:
        return f"{event.text}_{event.context}"

    def _compute(self, events: list[tp.Any]) -> tp.Iterator[np.ndarray]:
        return self.extract([e.text for e in events], [e.context for e in events])

    def extract(self, target_words: tp.Sequence[str], contexts: tp.Sequence[str]) -> tp.Iterator[np.ndarray]:
        """The body of the reference's `_get_data` loop (text.py:204-256): yields [n_states, hidden] per word.

        share_prefixes: inside a timeline the context of word i + 1 is the context of word i plus one word, until the cap on the
        context length starts to drop words on the left.  Such a run of N nested contexts takes ONE row -- its longest context --
        and N pooling windows (`prefix_groups`, `forward_windows`) instead of N rows: ceil(groups / batch_size) forwards instead of
        ceil(N / batch_size).  Once the context window slides, no context is a prefix of the next and every word is its own group:
        those words still cost one forward each."""
        if self.share_prefixes:
            yield from self._extract_shared(target_words, contexts)
            return
        model, tok = self.model, self.tokenizer
        pad_id = tok.eos_token_id
        for i in range(0, len(contexts), self.batch_size):
            words, ctx = list(target_words[i:i + self.batch_size]), list(contexts[i:i + self.batch_size])
            enc = tok(ctx, add_special_tokens=False, return_tensors="pt", padding=True, truncation=True)
            start, length = word_pool_windows(enc["input_ids"], words, pad_id)
            states = model.forward_pooled(enc["input_ids"], start, length).cpu().numpy()  # [n_states, B, dim]
            for j in range(len(words)):
                yield states[:, j]

    def _extract_shared(self, target_words: tp.Sequence[str], contexts: tp.Sequence[str]) -> tp.Iterator[np.ndarray]:
        model, tok = self.model, self.tokenizer
        pad_id = tok.eos_token_id
        rows: list[list[int]] = []
        windows: list[tuple[int, int]] = []
        for i in range(0, len(contexts), self.batch_size):   # tokenised exactly as on the per-word route, then the padding is stripped
            words, ctx = list(target_words[i:i + self.batch_size]), list(contexts[i:i + self.batch_size])
            ids = tok(ctx, add_special_tokens=False, return_tensors="pt", padding=True, truncation=True)["input_ids"]
            start, length = word_pool_windows(ids, words, pad_id)
            for j in range(len(words)):
                rows.append(ids[j, :int(start[j] + length[j])].tolist())   # start + length = the number of real tokens
                windows.append((int(start[j]), int(length[j])))
        groups = prefix_groups(rows)
        for i in range(0, len(groups), self.batch_size):
            batch = groups[i:i + self.batch_size]
            ids = torch.full((len(batch), max(1, max(len(longest) for longest, _ in batch))), pad_id, dtype=torch.int64)
            for g, (longest, _) in enumerate(batch):
                ids[g, :len(longest)] = torch.tensor(longest, dtype=torch.int64)
            win_row = [g for g, (_, members) in enumerate(batch) for _ in members]
            win = [windows[m] for _, members in batch for m in members]
            states = model.forward_windows(ids, win_row, [s for s, _ in win], [n for _, n in win]).cpu().numpy()  # [n_states, W, dim]
            for w in range(len(win)):   # members of a group are consecutive inputs: this is the input order
                yield states[:, w]

    def aggregate(self, latents: np.ndarray) -> np.ndarray:
        return self._aggregate_layers(latents)
