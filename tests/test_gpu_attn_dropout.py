"""GPU: attention dropout -- the softmax-dropout row kernels (ops.softmax_dropout_fwd / _bwd), modeling_utils.autograd.Attention /
RotaryAttention with (p, seed, site), and FmriEncoder's attn_dropout.  References are float64 torch compositions multiplied by the masks of
tests/dropout_restatement.py on the logical [B * heads * T, T] tensor; the function-level bounds are the ones tests/test_gpu_training.py and
tests/test_gpu_dropout_training.py apply (2e-2 output, 3e-2 per q / k / v third of dqkv, relative L2).

Kernel-level bounds.  Forward: a kept element is bf16(f32 softmax * scale_keep); the f32 softmax is within a few 1e-7 of float64, so the
element is within one bf16 step (2^-8 relative) of float64 softmax * scale_keep.  Backward: dS = bf16(P * fma(scale, m * dPd, negD)) with
negD = f32(-scale * D): four f32 roundings (negD, m * dPd, the fma, the product), each at most 2^-24 of |scale m dPd| + |scale D| times P,
so |dS - float64| <= 2^-8 |float64| + 2^-21 P (|scale m dPd| + |scale D|) -- the second term only matters where m dPd and D cancel."""

import functools
import random

import pytest
import torch

from tests.dropout_restatement import keep_mask, multiplier, scale as keep_scale

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
SITE = (4 << 56) | 1
KERNEL_SHAPES = [(33, 33), (280, 70), (64, 64), (576, 192), (1192, 298), (8, 256), (8, 512), (8, 1024), (8, 2048), (3, 1500)]   # rows x T
SPLITS = {33: 13, 280: 101, 64: 6, 576: 101, 1192: 597, 8: 3, 3: 1}                               # rows -> a first-slab size, never % 4 == 0
SCALE = 0.125


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _pad(T):
    return (T + 63) // 64 * 64


@functools.lru_cache(maxsize=None)
def _kernel_case(rows, T):
    """Scores, their float64 softmax / base-2 log-sum-exp, and the backward's operands -- computed once per shape, never modified."""
    g = torch.Generator().manual_seed(rows * 10007 + T)
    S = torch.randn(rows, T, generator=g) * 2.0
    soft = S.double().softmax(-1)
    lse2 = torch.logsumexp(S.double(), -1) / torch.log(torch.tensor(2.0, dtype=torch.float64))
    P = torch.zeros(rows, _pad(T), dtype=torch.bfloat16)
    P[:, :T] = soft.to(torch.bfloat16)
    dPd = torch.randn(rows, T, generator=g)
    return S, soft, lse2, P, dPd


def _scores_on_gpu(S):
    """The f32 scores as the leading T columns of a [rows, T_pad] buffer (the pitch the score GEMM writes with)."""
    rows, T = S.shape
    buf = torch.full((rows, _pad(T)), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :T] = S.cuda()
    return buf[:, :T]


# ---- forward kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows,T", KERNEL_SHAPES)
def test_forward_kernel_vs_float64_and_restated_mask(rows, T, p):
    from tribe_hip import ops

    S, soft, lse2, _, _ = _kernel_case(rows, T)
    Tp = _pad(T)
    out = torch.full((rows, Tp), 1.0, dtype=torch.bfloat16, device="cuda")
    Pd, lse = ops.softmax_dropout_fwd(_scores_on_gpu(S), p, SEED, SITE, out=out)
    assert Pd.data_ptr() == out.data_ptr()
    Pd, lse = Pd.cpu(), lse.cpu()
    keep = torch.from_numpy(keep_mask(rows, T, p, SEED, SITE))
    assert torch.equal(Pd[:, :T] != 0, keep)                                         # the zero / non-zero pattern IS the mask
    assert not bool(_bits(Pd[:, T:]).any()) and not bool(_bits(Pd[:, :T])[~keep].any())   # pad and dropped: zero bits (+0.0)
    want = soft * float(keep_scale(p))
    err = ((Pd[:, :T].double() - want).abs() / want)[keep].max()
    lse_err = ((lse.double() - lse2).abs() / lse2.abs()).max()
    print(f"[{rows}, {T}] p={p}: kept max rel err {float(err):.2e} (bound {2**-8:.2e}), lse2 max rel err {float(lse_err):.2e}")
    assert err <= 2.0**-8 and lse_err < 1e-5


@pytest.mark.parametrize("rows,T", KERNEL_SHAPES)
def test_forward_kernel_p_zero_is_tribe_softmax_fwd(rows, T):
    from tribe_hip import ops
    from tribe_hip._lib import check, lib

    S = _scores_on_gpu(_kernel_case(rows, T)[0])
    Tp = _pad(T)
    got, _ = ops.softmax_dropout_fwd(S, 0.0, SEED, SITE)
    want = torch.full((rows, Tp), 1.0, dtype=torch.bfloat16, device="cuda")
    check(lib().tribe_softmax_fwd(S.data_ptr(), rows, T, S.stride(0), want.data_ptr(), Tp, Tp, torch.cuda.current_stream().cuda_stream),
          "tribe_softmax_fwd")
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("rows,T", KERNEL_SHAPES)
def test_row0_makes_the_mask_independent_of_the_slab(rows, T):
    """One call over the slab against two calls split at a row that is no multiple of 4, the second with row0 moved: equal bits, forward
    and backward (the whole slab itself starts at row0 = 5 of the logical tensor)."""
    from tribe_hip import ops

    S, _, _, P, dPd = _kernel_case(rows, T)
    cut, base, p = SPLITS[rows], 5, 0.1
    assert 0 < cut < rows and cut % 4
    Sg = _scores_on_gpu(S)
    whole, lse = ops.softmax_dropout_fwd(Sg, p, SEED, SITE, row0=base)
    parts = torch.empty_like(whole)
    lse_parts = torch.empty_like(lse)
    ops.softmax_dropout_fwd(Sg[:cut], p, SEED, SITE, row0=base, out=parts[:cut], lse=lse_parts[:cut])
    ops.softmax_dropout_fwd(Sg[cut:], p, SEED, SITE, row0=base + cut, out=parts[cut:], lse=lse_parts[cut:])
    assert torch.equal(_bits(whole), _bits(parts)) and torch.equal(_bits(lse), _bits(lse_parts))
    assert torch.equal(whole[:, :T].cpu() != 0, torch.from_numpy(keep_mask(base + rows, T, p, SEED, SITE)[base:]))
    negD = torch.randn(rows, generator=torch.Generator().manual_seed(1)).cuda()
    Pg, dg = P.cuda(), dPd.cuda()
    dS, Pd = ops.softmax_dropout_bwd(Pg.clone(), dg, negD, SCALE, p, SEED, SITE, row0=base)
    dS2, Pd2 = torch.empty_like(dS), Pg.clone()
    ops.softmax_dropout_bwd(Pd2[:cut], dg[:cut], negD[:cut], SCALE, p, SEED, SITE, row0=base, dS=dS2[:cut])
    ops.softmax_dropout_bwd(Pd2[cut:], dg[cut:], negD[cut:], SCALE, p, SEED, SITE, row0=base + cut, dS=dS2[cut:])
    assert torch.equal(_bits(dS), _bits(dS2)) and torch.equal(_bits(Pd), _bits(Pd2))


# ---- backward kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("rows,T", KERNEL_SHAPES)
def test_backward_kernel_vs_float64(rows, T, p):
    from tribe_hip import ops

    _, _, _, P, dPd = _kernel_case(rows, T)
    Tp = _pad(T)
    keep = torch.from_numpy(keep_mask(rows, T, p, SEED, SITE))
    m = multiplier(rows, T, p, SEED, SITE)
    P64 = P[:, :T].double()
    D = (m * P64 * dPd.double()).sum(-1, keepdim=True)                               # rowsum(Pd * dPd)
    want = SCALE * P64 * (m * dPd.double() - D)
    negD = (-SCALE * D[:, 0]).float().cuda()
    Pg, dg = P.cuda(), dPd.cuda()
    # two buffers: P stays, Pd and dS are written in full (their pad columns too)
    dS = torch.full((rows, Tp), 1.0, dtype=torch.bfloat16, device="cuda")
    Pd = torch.full((rows, Tp), 1.0, dtype=torch.bfloat16, device="cuda")
    P_in = Pg.clone()
    ops.softmax_dropout_bwd(P_in, dg, negD, SCALE, p, SEED, SITE, dS=dS, Pd=Pd)
    assert torch.equal(_bits(P_in), _bits(Pg))
    # in place: P is overwritten by Pd
    P_io = Pg.clone()
    dS_io, Pd_io = ops.softmax_dropout_bwd(P_io, dg, negD, SCALE, p, SEED, SITE)
    assert Pd_io.data_ptr() == P_io.data_ptr()
    assert torch.equal(_bits(dS_io), _bits(dS)) and torch.equal(_bits(Pd_io), _bits(Pd))
    # Pd = bf16(P * m): one f32 multiply by float32(1 / (1 - p)), one rounding to bf16, +0.0 where dropped or padded
    want_pd = torch.zeros(rows, Tp, dtype=torch.bfloat16)
    want_pd[:, :T] = torch.where(keep, (P[:, :T].float() * torch.tensor(float(keep_scale(p)), dtype=torch.float32)).to(torch.bfloat16),
                                 torch.zeros((), dtype=torch.bfloat16))
    assert torch.equal(_bits(Pd.cpu()), _bits(want_pd))
    got = dS.cpu()
    assert not bool(_bits(got[:, T:]).any())
    slack = 2.0**-21 * P64 * ((SCALE * m * dPd.double()).abs() + (SCALE * D).abs())
    excess = ((got[:, :T].double() - want).abs() - 2.0**-8 * want.abs() - slack).max()
    rel = _rel(got[:, :T], want)
    print(f"[{rows}, {T}] p={p}: dS rel L2 {rel:.2e}, worst |err| - bound {float(excess):.2e} (<= 0 passes)")
    assert excess <= 0
    assert bool((got[:, :T][~keep] != 0).any())                                      # a dropped score keeps -scale * P * D


# ---- Attention.apply / RotaryAttention.apply --------------------------------------------------------------------------------------------
ATTN_SHAPES = [(2, 70, 2, 64), (1, 192, 3, 384), (2, 128, 2, 64), (1, 298, 1, 128)]   # (B, T, h, d)
P_ATTN = 0.2


def _rot_dim(d):
    return max(d // 2, 32)


@functools.lru_cache(maxsize=None)
def _attn_case(B, T, h, d, rotary):
    """(qkv, dout, float64 output, float64 dqkv) of softmax(scale q k^T) * m @ v with the restated mask, p = P_ATTN."""
    from oracle import xt_encoder

    g = torch.Generator().manual_seed(14)
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)  # noqa: E731
    qkv = bf(torch.randn(B * T, 3 * h * d, generator=g))
    dout = bf(torch.randn(B * T, h * d, generator=g))
    qt = qkv.double().requires_grad_()
    q, k, v = (t.transpose(1, 2) for t in qt.view(B, T, 3, h, d).unbind(2))          # [B, h, T, d]
    if rotary:
        freqs = xt_encoder.RotaryEmbedding(_rot_dim(d), interleaved=True)(T).double()
        q, k = (xt_encoder.apply_rotary_pos_emb(t, freqs, True) for t in (q, k))
    att = (torch.einsum("bhid,bhjd->bhij", q, k) * d**-0.5).softmax(-1)
    att = att * multiplier(B * h * T, T, P_ATTN, SEED, SITE).view(B, h, T, T)
    out = torch.einsum("bhij,bhjd->bhid", att, v).transpose(1, 2).reshape(B * T, h * d)
    out.backward(dout.double())
    return qkv, dout, out.detach(), qt.grad


def _run_attention(B, T, h, d, rotary, qkv, dout, *drop):
    from modeling_utils import autograd as ag
    from oracle import xt_encoder

    qg = qkv.cuda().bfloat16().requires_grad_()
    if rotary:
        rot = _rot_dim(d)
        half = torch.einsum("i,j->ij", torch.arange(T).float(), xt_encoder.RotaryEmbedding(rot).inv_freq.float())
        cos, sin = half.cos().cuda().contiguous(), half.sin().cuda().contiguous()
        out, _ = ag.RotaryAttention.apply(qg * 1, cos, sin, (-sin).contiguous(), B, T, h, d, d**-0.5, rot, True, *drop)
    else:
        out = ag.Attention.apply(qg, B, T, h, d, d**-0.5, *drop)
    out.backward(dout.cuda().bfloat16())
    return out.detach(), qg.grad


def _thirds(grad, B, T, h, d):
    g = grad.view(B, T, 3, h, d)
    return {"dq": g[:, :, 0], "dk": g[:, :, 1], "dv": g[:, :, 2]}


@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("B,T,h,d", ATTN_SHAPES)
def test_attention_with_dropout_vs_float64(B, T, h, d, rotary):
    qkv, dout, want, want_grad = _attn_case(B, T, h, d, rotary)
    got, grad = _run_attention(B, T, h, d, rotary, qkv, dout, P_ATTN, SEED, SITE)
    err = _rel(got.float().cpu(), want)
    print(f"(B, T, h, d) = {(B, T, h, d)} rotary={rotary}: output rel L2 {err:.2e}")
    assert err < 2e-2
    wants = _thirds(want_grad, B, T, h, d)
    for name, g in _thirds(grad.float().cpu(), B, T, h, d).items():
        err = _rel(g, wants[name])
        print(f"(B, T, h, d) = {(B, T, h, d)} rotary={rotary}: {name} rel L2 {err:.2e}")
        assert err < 3e-2, name


@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("B,T,h,d", ATTN_SHAPES)
def test_mask_does_not_depend_on_the_chunking(B, T, h, d, rotary, monkeypatch):
    """One sequence per chunk against every sequence in one chunk: a mask indexed by the chunk's own rows would differ by O(1)."""
    from modeling_utils import autograd as ag

    qkv, dout, _, _ = _attn_case(B, T, h, d, rotary)
    monkeypatch.setattr(ag.Attention, "CHUNK_BYTES", B * h * T * _pad(T) * 4)
    whole, whole_grad = _run_attention(B, T, h, d, rotary, qkv, dout, P_ATTN, SEED, SITE)
    monkeypatch.setattr(ag.Attention, "CHUNK_BYTES", h * T * _pad(T) * 4)
    each, each_grad = _run_attention(B, T, h, d, rotary, qkv, dout, P_ATTN, SEED, SITE)
    errs = [_rel(each.float(), whole.float())] + [_rel(a, b) for a, b in zip(_thirds(each_grad.float(), B, T, h, d).values(),
                                                                               _thirds(whole_grad.float(), B, T, h, d).values())]
    print(f"(B, T, h, d) = {(B, T, h, d)} rotary={rotary}: one sequence per chunk vs one chunk, rel L2 {max(errs):.2e}")
    assert max(errs) < 2e-2


@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("B,T,h,d", ATTN_SHAPES)
def test_p_zero_is_the_call_without_the_arguments(B, T, h, d, rotary):
    qkv, dout, _, _ = _attn_case(B, T, h, d, rotary)
    a, ga = _run_attention(B, T, h, d, rotary, qkv, dout)
    b, gb = _run_attention(B, T, h, d, rotary, qkv, dout, 0.0, SEED, SITE)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(ga), _bits(gb))


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
FDIMS = {"text": (2, 40), "audio": (2, 24), "video": (2, 33)}
V, TOUT, S, B, T = 60, 13, 3, 2, 64
DEPTH = 2
P_MODEL = 0.2


def _model(like=None, **kw):
    from algonauts2025.model import FmriEncoderConfig

    torch.manual_seed(5)
    model = FmriEncoderConfig(n_subjects=S, hidden=768, depth=DEPTH, heads=4, projector_hidden_sizes=[96], **kw).build(FDIMS, V, TOUT)
    if like is not None:
        model.load_state_dict(like.state_dict())
    return model.cuda()


@pytest.fixture(scope="module")
def batch():
    from data_utils.dataloader import SegmentData
    from oracle import tribe_ref

    data = tribe_ref.synthetic_batch(B, T, FDIMS, S, seed=1)
    data["fmri"] = torch.randn(B, V, TOUT, generator=torch.Generator().manual_seed(9))
    return SegmentData(data={k: v.cuda() for k, v in data.items()}, segments=[None] * B)


def _training_loss(model, batch):
    from algonauts2025.pl_module import BrainModule
    from modeling_utils.losses import TorchLossConfig

    return BrainModule(model, TorchLossConfig(name="MSELoss").build(), None, {}).training_step(batch, 0)


def _step(model, batch, seed):
    torch.manual_seed(seed)
    random.seed(seed)
    model.train().zero_grad(set_to_none=True)
    loss = _training_loss(model, batch)
    loss.backward()
    return loss.detach().clone(), {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None}


def test_eval_ignores_attn_dropout(batch):
    plain = _model()
    dropped = _model(like=plain, attn_dropout=P_MODEL)
    with torch.no_grad():
        a, b = plain.eval()(batch), dropped.eval()(batch)
        assert torch.equal(_bits(a), _bits(b))
        c = dropped.train()(batch)                          # train mode under no_grad: the fused path, no dropout, no key
        assert torch.equal(_bits(a), _bits(c)) and dropped.last_dropout_key is None


def test_training_is_reproducible_and_differs_from_no_dropout(batch):
    plain = _model()
    model = _model(like=plain, attn_dropout=P_MODEL)
    loss_a, grads_a = _step(model, batch, 3)
    key_a = model.last_dropout_key
    loss_b, grads_b = _step(model, batch, 3)
    assert key_a is not None and model.last_dropout_key == key_a
    assert torch.equal(_bits(loss_a), _bits(loss_b)) and grads_a.keys() == grads_b.keys()
    assert all(torch.equal(_bits(grads_a[n]), _bits(grads_b[n])) for n in grads_a)
    loss_0, grads_0 = _step(plain, batch, 3)
    assert float(loss_0) != float(loss_a)
    assert not torch.equal(grads_0["encoder.layers.0.1.to_q.weight"], grads_a["encoder.layers.0.1.to_q.weight"])


def test_one_mask_call_per_attention_sub_layer(batch, monkeypatch):
    from algonauts2025.model import SITE_ATTN
    from tribe_hip import ops

    for seed in range(50):                                  # a seed under which stochastic depth skips exactly one attention sub-layer
        random.seed(seed)
        drops = [random.random() < 0.5 for _ in range(2 * DEPTH)]
        if sum(drops[0::2]) == 1:
            break
    fwd, bwd = [], []
    real_f, real_b = ops.softmax_dropout_fwd, ops.softmax_dropout_bwd
    monkeypatch.setattr(ops, "softmax_dropout_fwd", lambda S_, p, seed, site, **kw: (fwd.append((p, seed, site)), real_f(S_, p, seed, site, **kw))[1])
    monkeypatch.setattr(ops, "softmax_dropout_bwd",
                        lambda P_, dP, nd, sc, p, seed, site, **kw: (bwd.append((p, seed, site)), real_b(P_, dP, nd, sc, p, seed, site, **kw))[1])
    for layer_dropout, skipped in ((0.0, [False] * DEPTH), (0.5, drops[0::2])):
        model = _model(attn_dropout=P_MODEL, layer_dropout=layer_dropout).train()
        fwd.clear(), bwd.clear()
        torch.manual_seed(6)
        random.seed(seed)
        loss = _training_loss(model, batch)
        assert not bwd
        loss.backward()
        want = [(P_MODEL, model.last_dropout_key, (SITE_ATTN << 56) | i) for i in range(DEPTH) if not skipped[i]]
        assert model.last_dropout_key is not None and fwd == want and sorted(bwd) == want, (layer_dropout, fwd, bwd)
        assert model.last_layer_drops == (drops if layer_dropout else None)


def test_key_draw_and_rng_stream(batch):
    # all-zero settings: the modality-dropout draws are all a pass consumes
    model = _model(attn_dropout=0.0).train()
    torch.manual_seed(8)
    for _ in FDIMS:
        torch.rand(1)
    want = torch.get_rng_state()
    torch.manual_seed(8)
    model(batch)
    assert torch.equal(torch.get_rng_state(), want) and model.last_dropout_key is None
    # attn_dropout alone: one key, drawn right after them
    key = int(torch.randint(0, 2**63 - 1, (1,), dtype=torch.int64).item())
    want = torch.get_rng_state()
    model = _model(attn_dropout=P_MODEL).train()
    torch.manual_seed(8)
    model(batch)
    assert model.last_dropout_key == key and torch.equal(torch.get_rng_state(), want)


def test_active_attn_dropout_never_shares_contrastive_latents(batch):
    for kw, hits in ((dict(), 1), (dict(attn_dropout=0.1), 0)):
        model = _model(contrastive_enabled=True, modality_dropout=0.0, **kw).train()
        torch.manual_seed(2)
        random.seed(2)
        _training_loss(model, batch)
        assert getattr(model, "shared_latent_hits", 0) == hits, kw
