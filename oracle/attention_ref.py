"""Float64 references, rounding-error bounds and fault-injecting emulations for the attention kernels.  CPU only.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Three layers:

* `attention_f64` / `attention_backward_f64`: the operation in float64, nothing else.
* `forward_bound` / `lse_bound` / `row_errors`: what a correct bf16 kernel may differ from it by.
* `emulate_forward` / `emulate_backward`: torch-f32 restatements that round where the kernels and
  `modeling_utils/autograd.py::Attention.backward` round, with flags that each inject ONE fault of the kind attention kernels
  have (a dropped or doubled key of a ragged tile, an off-by-one mask, band or bias offset, a stale pad column, a skipped
  rescale, a wrong scale).  tests/test_attention_host.py runs them to show, without a GPU, that the bounds pass the clean
  arithmetic and catch every fault.

Layouts: q [B, heads, T, d], k / v [B, heads, T, d] with grouped-query heads already repeated (`repeat_kv`); the fused device
buffer is [B*T, (heads_q + 2 heads_kv) d] = q heads | k heads | v heads (`pack_qkv` / `unpack_qkv`).
A relative-key bias (and any `bias`) is added to q.k BEFORE the scale: s_ij = (q_i.k_j + bias_ij) * scale.
"""

from __future__ import annotations

import math

import torch

LOG2E = 1.4426950408889634
U_BF16 = 2.0**-8      # unit roundoff of bf16 (8 significant bits, round to nearest even)
U_F32 = 2.0**-24
KEY_TILE = 32         # keys per step of the flash-style kernels
ROW_BLOCK = 32        # query rows that decide a deferred-max rescale together (one wave of the dim_head 384 kernel)

FORWARD_FAULTS = ("drop_last_key", "double_last_key", "exclude_diagonal", "band_left_short", "band_right_short", "skip_rescale")
BACKWARD_FAULTS = ("zero_last_dk_row", "stale_pad_column", "chunk_bias_off_by_one", "scale_dq")


def bf(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest even) and back to the input's dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def diffuse(B: int, T: int, heads_q: int, d: int, seed: int, heads_kv: int | None = None):
    """randn q, k, v, bf16-exact: every key carries a little weight in every row."""
    heads_kv = heads_kv or heads_q
    g = torch.Generator().manual_seed(seed)
    q = bf(torch.randn(B, heads_q, T, d, generator=g))
    k = bf(torch.randn(B, heads_kv, T, d, generator=g))
    v = bf(torch.randn(B, heads_kv, T, d, generator=g))
    return q, k, v


def perm_targets(T: int, heads_q: int, causal: bool) -> torch.Tensor:
    """pi[head, i]: the key row i is aimed at.  Bidirectional: (T-1-i + 17 head) mod T -- a permutation, so every key (the last one of
    a ragged tile too) is the target of exactly one row, and row 0 of head 0 meets its maximum in the last key tile.  Causal: the
    diagonal for even i, i // 2 for odd i."""
    i = torch.arange(T)
    if causal:
        return torch.where(i % 2 == 0, i, i // 2)[None].expand(heads_q, T)
    return (T - 1 - i[None] + 17 * torch.arange(heads_q)[:, None]) % T


def perm(c: float, B: int, T: int, heads_q: int, d: int, seed: int, heads_kv: int | None = None, causal: bool = False):
    """q_i = bf16(c * k_pi(i)): row i puts most of its weight on key pi(i).  c = 2 is near one-hot, c = 0.6 concentrated with several
    keys that matter."""
    heads_kv = heads_kv or heads_q
    g = torch.Generator().manual_seed(seed)
    k = bf(torch.randn(B, heads_kv, T, d, generator=g))
    v = bf(torch.randn(B, heads_kv, T, d, generator=g))
    pi = perm_targets(T, heads_q, causal)
    kq = repeat_kv(k, heads_q)
    q = bf(c * torch.gather(kq, 2, pi[None, :, :, None].expand(B, heads_q, T, d)))
    return q, k, v


KINDS = ("diffuse", "perm2", "perm06")


def make_inputs(kind: str, B: int, T: int, heads_q: int, d: int, seed: int, heads_kv: int | None = None, causal: bool = False):
    """kind: diffuse | perm2 (c = 2) | perm06 (c = 0.6) | conc (c = 0.6 sqrt(64 / d): the logit lead c sqrt(d) = 4.8 that perm06 has at
    dim_head 64, at every head size -- at dim_head 384 perm06 itself leads by 11.8 and is as one-hot as perm2)."""
    if kind == "diffuse":
        return diffuse(B, T, heads_q, d, seed, heads_kv)
    c = {"perm2": 2.0, "perm06": 0.6, "conc": 0.6 * math.sqrt(64.0 / d)}[kind]
    return perm(c, B, T, heads_q, d, seed, heads_kv, causal)


# the attention() grid of the GPU tests: lengths on and either side of the key-tile (32) and query-block (128) edges, one key only, fewer
# keys than a tile, ragged tails; dim_head 64 adds 1000 (an odd count of 32-key sub-tiles in the 64-row kernels)
FORWARD_LENGTHS = (1, 7, 32, 33, 128, 129, 161, 300)
FORWARD_BATCH_HEADS = ((1, 1), (3, 1), (2, 4), (3, 3))     # B * heads % 8 = 1, 3, 0, 1; (3, 3) needs a second group of 8
RELATIVE_KEY_GEOMETRIES = ((70, 5, 3), (161, 0, 0), (300, 64, 8), (300, 100, 90))     # (T, left, right)


def forward_lengths(d: int) -> tuple:
    return FORWARD_LENGTHS + ((1000,) if d == 64 else ())


def forward_batch_heads(i_length: int, i_kind: int) -> tuple:
    """The (B, heads) a (length, input kind) pair of the grid runs at: cycled, so each kernel meets all four."""
    return FORWARD_BATCH_HEADS[(i_length + i_kind) % len(FORWARD_BATCH_HEADS)]


def repeat_kv(x: torch.Tensor, heads_q: int) -> torch.Tensor:
    """[B, heads_kv, T, d] -> [B, heads_q, T, d]: q head i reads kv head i // group."""
    return x if x.shape[1] == heads_q else x.repeat_interleave(heads_q // x.shape[1], dim=1)


def pack_qkv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    B, _, T, _ = q.shape
    return torch.cat([t.transpose(1, 2).reshape(B * T, -1) for t in (q, k, v)], dim=1).contiguous()


def unpack_qkv(qkv: torch.Tensor, B: int, T: int, heads: int, d: int):
    return tuple(t.transpose(1, 2) for t in qkv.view(B, T, 3, heads, d).unbind(2))


def unpack_out(out: torch.Tensor, B: int, T: int, heads: int, d: int) -> torch.Tensor:
    """Device output [B*T, heads*d] -> [B, heads, T, d]."""
    return out.view(B, T, heads, d).transpose(1, 2)


def relative_key_table(q: torch.Tensor, left: int, right: int, seed: int) -> torch.Tensor:
    """qe[b, h, i, p] = q_i . E[p] (f32, the table the kernel is given), E ~ N(0, 1): q.E has the spread of q.k for randn k."""
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(left + right + 1, q.shape[-1], generator=g)
    return torch.einsum("bhid,pd->bhip", q.float(), emb)


def relative_key_bias(qe: torch.Tensor, T: int, left: int, right: int, clamp_left: int | None = None,
                      clamp_right: int | None = None) -> torch.Tensor:
    """bias[b, h, i, j] = qe[b, h, i, clamp(j - i, -left, right) + left] (HF Wav2Vec2-BERT relative_key)."""
    lo = left if clamp_left is None else clamp_left
    hi = right if clamp_right is None else clamp_right
    dist = (torch.arange(T)[None, :] - torch.arange(T)[:, None]).clamp(-lo, hi) + left
    return torch.gather(qe, 3, dist[None, None].expand(*qe.shape[:2], T, T))


def rotary_tables(T: int, rot_dim: int) -> tuple[torch.Tensor, torch.Tensor]:
    """cos / sin [T, rot_dim / 2] f32 of the x_transformers rotary (theta 10000)."""
    inv = 1.0 / (10000 ** (torch.arange(0, rot_dim, 2).float() / rot_dim))
    ang = torch.arange(T).float()[:, None] * inv[None]
    return ang.cos().contiguous(), ang.sin().contiguous()


def rotate_interleaved(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """Partial rotary on interleaved pairs of the first 2 * cos.shape[1] dims of x [..., T, d], in x's dtype, no rounding."""
    rot = 2 * cos.shape[1]
    c, s = cos.to(x.dtype), sin.to(x.dtype)
    a, b = x[..., 0:rot:2], x[..., 1:rot:2]
    y = x.clone()
    y[..., 0:rot:2] = a * c - b * s
    y[..., 1:rot:2] = b * c + a * s
    return y


# ------------------------------------------------------------------------------------------------
# float64 references
# ------------------------------------------------------------------------------------------------
def attention_f64(q, k, v, scale: float, *, causal: bool = False, bias=None):
    """out = softmax((q k^T + bias) * scale) v.  Returns out [B,h,T,d], P [B,h,T,T] and lse2 [B,h,T] = log2 sum_j exp(s_ij), float64."""
    q, k, v = q.double(), k.double(), v.double()
    s = torch.einsum("bhid,bhjd->bhij", q, k)
    if bias is not None:
        s = s + bias.double()
    s = s * scale
    if causal:
        T = s.shape[-1]
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), -math.inf)
    m = s.amax(-1, keepdim=True)
    e = (s - m).exp()
    l = e.sum(-1, keepdim=True)
    P = e / l
    return P @ v, P, (m.squeeze(-1) + l.squeeze(-1).log()) / math.log(2.0)


def attention_backward_f64(q, k, v, P, dout, scale: float):
    """Gradients of out = P v w.r.t. q, k, v for P = softmax(scale q k^T) (float64, closed form; equals autograd)."""
    q, k, v, dout = q.double(), k.double(), v.double(), dout.double()
    dv = P.transpose(-1, -2) @ dout
    dP = dout @ v.transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True)) * scale
    return dS @ k, dS.transpose(-1, -2) @ q, dv


# ------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------
def forward_bound(P: torch.Tensor, v: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Per element: 2^-8 (P @ |v|) + 2^-7 |out| + 1e-6, with u = 2^-8 the bf16 unit roundoff:
    each p_j is rounded once before P V (u sum_j P_ij |v_jd|); the denominator may be the sum of the rounded p (u |out|); the output is
    rounded once (u |out|); the f32 work (score accumulation, exp2, the running sum) sits under the constant.  The deferred maximum
    (p up to 2^8) scales numerator and denominator alike and leaves the relative roundings as they are."""
    return U_BF16 * (P.double() @ v.double().abs()) + 2 * U_BF16 * out.double().abs() + 1e-6


def lse_bound(q: torch.Tensor, k: torch.Tensor, scale: float, T: int, K: int, *, rounded_p_sum: bool = False) -> torch.Tensor:
    """Per row, for a kernel whose running sum adds the unrounded f32 p:
    2 [ K 2^-24 scale log2e max_j sum_d |q_id k_jd|  +  (T + 16) 2^-24 / ln 2 ]:
    f32 accumulation of K products in the score that dominates the row, then an f32 sum of T terms plus exp2 / log2.
    rounded_p_sum: the kernel sums bf16-rounded p instead -- the sum is off by at most a factor 1 +- 2^-8, log2(1 + 2^-8) more."""
    dots = (q.double().abs() @ k.double().abs().transpose(-1, -2)).amax(-1)
    b = 2.0 * (K * U_F32 * scale * LOG2E * dots + (T + 16) * U_F32 / math.log(2.0))
    return b + (math.log2(1.0 + U_BF16) if rounded_p_sum else 0.0)


def ratio_report(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor) -> tuple[float, tuple]:
    """Largest |got - want| / bound over ALL elements and its index; a non-finite value counts as infinitely wrong."""
    r = (got.double() - want).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf))
    i = int(r.argmax())
    return float(r.flatten()[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), r.shape))


def row_errors(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """got / want: gradients of the fused buffer viewed [B, T, 3, h, d].  e[b, t, tensor, head] = |got_t - want_t|_2 / RMS_t |want_t|_2:
    the error of one row of dq / dk / dv of one (sequence, head) against the typical row of that slice, so a garbage or zeroed row
    scores about 1 however many rows the tensor has."""
    got, want = got.double(), want.double()
    diff = (got - want).norm(dim=-1)
    diff = torch.where(torch.isfinite(diff), diff, torch.full_like(diff, math.inf))
    rms = want.norm(dim=-1).pow(2).mean(dim=1, keepdim=True).sqrt()
    return diff / rms


def gain_errors(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """g[b, tensor, head] = <got, want> / <want, want> - 1 over one (sequence, head) slice of dq / dk / dv: the systematic part of the
    error.  Rounding noise has no preferred sign and averages out over the T d elements of a slice; a wrong scale does not."""
    got, want = got.double(), want.double()
    g = (got * want).sum(dim=(1, 4)) / want.pow(2).sum(dim=(1, 4)) - 1.0
    return torch.where(torch.isfinite(g), g, torch.full_like(g, math.inf))


# ------------------------------------------------------------------------------------------------
# emulations
# ------------------------------------------------------------------------------------------------
def emulate_forward(q, k, v, scale: float, *, causal: bool = False, bias=None, rel=None, fault: str | None = None):
    """The flash-style kernels in torch f32: key tiles of 32, running maximum with the deferred rescale (only when some row of a block
    of 32 rows sees its maximum grow by more than 2^8), p = exp2(s scale log2e - m) added UNROUNDED to the running sum and ROUNDED TO
    BF16 into P V (f32 accumulation), output rounded to bf16.  rel = (qe, left, right) builds the relative-key bias.
    Returns out [B,h,T,d] (bf16 values in f32) and lse2 [B,h,T] f32.

    fault injects one error (named inputs: where tests/test_attention_host.py shows it breaks forward_bound by >= 3x):
      drop_last_key     key T-1 is never visited (ragged tile cut one short).           bidirectional perm2, perm06
      double_last_key   key T-1 is visited twice (tile overlap).                         bidirectional diffuse; perm06 at dim_head 64
      exclude_diagonal  causal mask j >= i instead of j > i (rows >= 1).                 causal perm2, perm06, diffuse
      band_left_short   relative-key distance clamped at -(left-1).                      relative-key diffuse, perm06 (left >= 1)
      band_right_short  relative-key distance clamped at right-1.                        relative-key diffuse, perm06 (right >= 1)
      skip_rescale      O is not rescaled when the maximum grows by more than 2^8.       bidirectional perm2 (T > 32)
    """
    assert fault is None or fault in FORWARD_FAULTS, fault
    q, k, v = q.float(), k.float(), v.float()
    B, h, T, d = q.shape
    if rel is not None:
        qe, left, right = rel
        assert (fault != "band_left_short" or left >= 1) and (fault != "band_right_short" or right >= 1), "no band to shorten"
        bias = relative_key_bias(qe, T, left, right, clamp_left=left - 1 if fault == "band_left_short" else None,
                                 clamp_right=right - 1 if fault == "band_right_short" else None)
    s = torch.einsum("bhid,bhjd->bhij", q, k)
    if bias is not None:
        s = s + bias.float()
    s = s * (scale * LOG2E)
    if causal:
        mask = torch.ones(T, T, dtype=torch.bool).triu(0 if fault == "exclude_diagonal" else 1)
        mask[0, 0] = False
        s = s.masked_fill(mask, -math.inf)
    vv = v
    if fault == "drop_last_key":
        s = s[..., : T - 1]
        vv = v[:, :, : T - 1]
    elif fault == "double_last_key":
        s = torch.cat([s, s[..., T - 1:]], dim=-1)
        vv = torch.cat([v, v[:, :, T - 1:]], dim=2)
    nk = s.shape[-1]
    m_run = torch.full((B, h, T), -math.inf)
    l_run = torch.zeros(B, h, T)
    o = torch.zeros(B, h, T, d)
    nblk = (T + ROW_BLOCK - 1) // ROW_BLOCK
    for j0 in range(0, nk, KEY_TILE):
        st = s[..., j0:j0 + KEY_TILE]
        pmax = st.amax(-1)
        if causal:   # a tile wholly above the diagonal for some rows: those rows keep their state
            pmax = torch.where(torch.isfinite(pmax), pmax, m_run)
        grow = torch.nn.functional.pad(pmax - m_run > 8.0, (0, nblk * ROW_BLOCK - T)).view(B, h, nblk, ROW_BLOCK).any(-1)
        grow = grow.repeat_interleave(ROW_BLOCK, dim=-1)[..., :T]
        m_new = torch.where(grow, torch.maximum(m_run, pmax), m_run)
        alpha = torch.where(torch.isfinite(m_run), torch.exp2(m_run - m_new), torch.zeros_like(m_run))
        alpha = torch.where(grow, alpha, torch.ones_like(alpha))
        m_run = m_new
        l_run = l_run * alpha
        if fault != "skip_rescale":
            o = o * alpha[..., None]
        p = torch.exp2(st - m_run[..., None])
        p = torch.where(torch.isfinite(st), p, torch.zeros_like(p))
        l_run = l_run + p.sum(-1)
        o = o + bf(p) @ vv[:, :, j0:j0 + KEY_TILE]
    return bf(o / l_run[..., None]), m_run + torch.log2(l_run)


def emulate_backward(q, k, v, dout, scale: float, *, fused: bool, chunk_seqs: int | None = None, rotary=None, fault: str | None = None):
    """modeling_utils/autograd.py::Attention.backward in torch f32, rounding to bf16 wherever it stores bf16.  q, k, v, dout:
    [B, h, T, d] bf16-exact.  Returns dq, dk, dv [B, h, T, d] (bf16 values in f32).

    fused (dim_head 384, FUSED_SOFTMAX): O (bf16) and lse2 come from the forward kernel; P = bf16(exp2(scale log2e q.k - lse2)),
    D = rowsum(dO * O), dS = bf16((scale dO.v - scale D) * P) with the bf16 P.
    materialised: S = scale q.k (f32), P = bf16(softmax(S)), dP = dO.v (f32), dS = bf16(scale P (dP - rowsum(P dP))) with the bf16 P.
    Then dQ = bf16(dS K), dK = bf16(dS^T Q), dV = bf16(P^T dO), f32 accumulation.
    rotary = (cos, sin): RotaryAttention -- q and k are rotated and rounded to bf16 first, dq and dk rotated back and rounded again.

    fault injects one error (where tests/test_attention_host.py shows it breaks the backward bound by >= 3x):
      zero_last_dk_row       row T-1 of dK is never written.                                              every case
      stale_pad_column       column T of the T_pad-wide P holds a stale 0.25 where the K = T_pad products expect zero; the operand row
                             it meets is a stale copy of row 0.  Reaches dQ (through dS) when T is no multiple of 64.
      chunk_bias_off_by_one  fused path, sequences after the first chunk: the row biases -lse2 and -scale D are read one row late.
                             Needs chunk_seqs < B.
      scale_dq               dQ is 1.025 x too large.                                                     every case
    """
    assert fault is None or fault in BACKWARD_FAULTS, fault
    q, k, v, dout = q.float(), k.float(), v.float(), bf(dout.float())
    B, h, T, d = q.shape
    if rotary is not None:
        cos, sin = rotary
        q, k = bf(rotate_interleaved(q, cos, sin)), bf(rotate_interleaved(k, cos, sin))
    chunk_seqs = chunk_seqs or B
    s = torch.einsum("bhid,bhjd->bhij", q, k)
    dP = torch.einsum("bhid,bhjd->bhij", dout, v)
    if fused:
        out, lse2 = emulate_forward(q, k, v, scale)
        bias_p = -lse2                                   # [B, h, T] row biases of the two GEMM epilogues
        bias_d = -scale * (dout * out).sum(-1)
        if fault == "chunk_bias_off_by_one" and chunk_seqs < B:
            late = lambda t: torch.cat([t.flatten()[1:], t.flatten()[-1:]]).view_as(t)   # noqa: E731
            bias_p = torch.cat([bias_p[:chunk_seqs], late(bias_p)[chunk_seqs:]])
            bias_d = torch.cat([bias_d[:chunk_seqs], late(bias_d)[chunk_seqs:]])
        P = bf(torch.exp2(s * (scale * LOG2E) + bias_p[..., None]))
        dS = bf((scale * dP + bias_d[..., None]) * P)
    else:
        P = bf((s * scale).softmax(-1))
        dS = bf(scale * P * (dP - (P * dP).sum(-1, keepdim=True)))
    dq = dS @ k
    if fault == "stale_pad_column" and T % 64 != 0:
        p_pad = torch.full((B, h, T), 0.25)
        dp_pad = torch.einsum("bhid,bhd->bhi", dout, v[:, :, 0])
        if fused:
            ds_pad = bf((scale * dp_pad + bias_d) * p_pad)
        else:
            ds_pad = bf(scale * p_pad * (dp_pad - (P * dP).sum(-1) - p_pad * dp_pad))
        dq = dq + ds_pad[..., None] * k[:, :, :1]
    dk = dS.transpose(-1, -2) @ q
    dv = P.transpose(-1, -2) @ dout
    if fault == "scale_dq":
        dq = dq * 1.025
    dq, dk, dv = bf(dq), bf(dk), bf(dv)
    if fault == "zero_last_dk_row":
        dk[:, :, T - 1] = 0
    if rotary is not None:
        dq, dk = bf(rotate_interleaved(dq, cos, -sin)), bf(rotate_interleaved(dk, cos, -sin))
    return dq, dk, dv


def grads_view(dq, dk, dv) -> torch.Tensor:
    """dq, dk, dv [B, h, T, d] -> [B, T, 3, h, d], the view of the fused gradient buffer that row_errors takes."""
    return torch.stack([t.transpose(1, 2) for t in (dq, dk, dv)], dim=2)


# ------------------------------------------------------------------------------------------------
# the backward cases, shared by tests/test_attention_host.py (CPU: floors, faults) and tests/test_gpu_attention_bounds.py
# ------------------------------------------------------------------------------------------------
# (path, B, T, heads, dim_head, chunk_seqs, rot_dim).  fused = dim_head 384 with the forward kernel's log-sum-exp; B = 3 in chunks of 2
# leaves a short last chunk; T = 70 / 298 have pad columns (T_pad 128 / 320); T = 128 / 1024 take the transposed-operand GEMM.
# materialised = the S / dP + softmax kernels: dim_head 64 / 128 as they come, dim_head 384 with FUSED_SOFTMAX off.
# rot_dim != 0 = RotaryAttention (rotate-back of dq, dk).
BACKWARD_CASES = (
    ("fused", 3, 70, 2, 384, 2, 0), ("fused", 3, 128, 2, 384, 2, 0), ("fused", 2, 298, 1, 384, 1, 0), ("fused", 1, 1024, 1, 384, 1, 0),
    ("materialised", 3, 70, 2, 64, 3, 0), ("materialised", 2, 128, 2, 64, 2, 0),
    ("materialised", 3, 70, 2, 128, 3, 0), ("materialised", 2, 128, 2, 128, 2, 0),
    ("materialised", 3, 70, 2, 384, 3, 0), ("materialised", 2, 128, 2, 384, 2, 0),
    ("fused", 2, 70, 2, 384, 1, 192),
)
# `conc` is perm(0.6) carried to every head size at the logit lead it has at dim_head 64 (make_inputs).  perm(0.6) itself at dim_head
# 384 leads by 11.8: rows as one-hot as perm(2), where dS = P (dP - D) cancels against a D made from the bf16 O -- the clean emulation
# then errs by up to 4.6 row norms, which is rounding noise on a vanishing gradient and no kernel fault, and a floor of 4.6 bounds nothing.
BACKWARD_KINDS = ("diffuse", "conc")

# Largest clean-emulation error over every (case, kind) of a path, measured on the CPU by tests/test_attention_host.py and rounded up
# in the second digit:  row metric (row_errors): fused 0.0252, materialised 0.0208;  gain metric (gain_errors): 1.27e-3 / 1.16e-3.
# The bound a kernel is held to is 4 x the floor (MFMA summation order, hardware exp2); it is never taken from GPU output.
BACKWARD_ROW_FLOOR = {"fused": 0.026, "materialised": 0.021}
BACKWARD_GAIN_FLOOR = {"fused": 1.3e-3, "materialised": 1.2e-3}
BACKWARD_MARGIN = 4.0


def backward_case_inputs(case, kind: str):
    """q, k, v, dout [B, h, T, d] (bf16-exact), scale, rotary tables or None, and the float64 gradients viewed [B, T, 3, h, d]."""
    _, B, T, h, d, _, rot = case
    q, k, v = make_inputs(kind, B, T, h, d, seed=100 + T + d)
    g = torch.Generator().manual_seed(7 + T)
    dout = bf(torch.randn(B, h, T, d, generator=g))
    scale = d**-0.5
    rotary = rotary_tables(T, rot) if rot else None
    q64, k64 = q.double(), k.double()
    if rot:
        q64, k64 = rotate_interleaved(q64, *rotary), rotate_interleaved(k64, *rotary)
    _, P, _ = attention_f64(q64, k64, v, scale)
    dq, dk, dv = attention_backward_f64(q64, k64, v, P, dout, scale)
    if rot:
        dq, dk = rotate_interleaved(dq, rotary[0], -rotary[1]), rotate_interleaved(dk, rotary[0], -rotary[1])
    return q, k, v, dout, scale, rotary, grads_view(dq, dk, dv)
