"""GPU: dropout on the training path -- modeling_utils.autograd.Dropout, FeedForward's (p, seed, site), Mlp's HIP dropout backend and
FmriEncoder's ff_dropout / layer_dropout / projector_dropout.  References are float64 torch compositions that multiply by the masks of
tests/dropout_restatement.py; the bounds are the ones tests/test_gpu_training.py and tests/test_gpu_mlp.py apply to the same functions
without dropout (2e-2 output, 3e-2 gradients, relative L2: bf16 GEMM operands against a float64 graph)."""

import random

import pytest
import torch
from torch import nn

from tests.dropout_restatement import multiplier

pytestmark = pytest.mark.gpu

SEED, SITE = 0x5EED0123456789AB, (1 << 56) | 3
MLP_OUT_BLOCK = 0xFFFF


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- autograd functions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("width,dim", [(100, None), (128, 100), (64, None)])
def test_dropout_function_backward_is_the_same_map(dtype, width, dim):
    from modeling_utils import autograd as ag
    from tribe_hip import ops

    g = torch.Generator().manual_seed(0)
    x = torch.randn(37, width, generator=g).to(dtype).cuda().requires_grad_()
    dy = torch.randn(37, width, generator=g).to(dtype).cuda()
    d = width if dim is None else dim
    y = ag.Dropout.apply(x, 0.15, SEED, SITE, dim)
    assert y.data_ptr() != x.data_ptr()
    assert torch.equal(_bits(y[:, :d]), _bits(ops.dropout_apply(x.detach()[:, :d], 0.15, SEED, SITE))) and not bool(y[:, d:].any())
    y.backward(dy)
    assert torch.equal(_bits(x.grad[:, :d]), _bits(ops.dropout_apply(dy[:, :d], 0.15, SEED, SITE))) and not bool(x.grad[:, d:].any())
    # in place: the very tensor comes back, pad columns as they were
    z = torch.randn(37, width, generator=g).to(dtype).cuda()
    want = ops.dropout_apply(z[:, :d], 0.15, SEED, SITE)
    pad = z[:, d:].clone()
    out = ag.Dropout.apply(z, 0.15, SEED, SITE, dim, True)
    assert out.data_ptr() == z.data_ptr() and torch.equal(_bits(out[:, :d]), _bits(want)) and torch.equal(out[:, d:], pad)


def _ff_tensors():
    """The FeedForward operands of test_autograd_blocks_vs_torch (tests/test_gpu_training.py)."""
    g = torch.Generator().manual_seed(0)
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)  # noqa: E731
    M, D, Fh = 200, 128, 256
    x = bf(torch.randn(M, D, generator=g)); w1 = bf(torch.randn(Fh, D, generator=g) / D**0.5); b1 = torch.randn(Fh, generator=g) * 0.1
    w2 = bf(torch.randn(D, Fh, generator=g) / Fh**0.5); b2 = torch.randn(D, generator=g) * 0.1
    res = torch.randn(M, D, generator=g); rs = torch.rand(D, generator=g) + 0.5; dy = bf(torch.randn(M, D, generator=g))
    return (x, w1, b1, w2, b2, res, rs), dy


def _ff_gpu(tensors):
    x, *rest = tensors
    return [x.cuda().bfloat16().requires_grad_()] + [t.cuda().requires_grad_() for t in rest]


def test_feed_forward_with_dropout_vs_float64():
    from modeling_utils import autograd as ag

    tensors, dy = _ff_tensors()
    p = 0.1
    M, Fh = tensors[0].shape[0], tensors[1].shape[0]
    ts = [t.double().requires_grad_() for t in tensors]
    h = torch.nn.functional.gelu(ts[0] @ ts[1].t() + ts[2]) * multiplier(M, Fh, p, SEED, SITE)
    want = h @ ts[3].t() + ts[4] + ts[5] * ts[6]
    want.backward(dy.double())
    gs = _ff_gpu(tensors)
    got = ag.FeedForward.apply(*gs, False, p, SEED, SITE)
    got.backward(dy.cuda())
    err = _rel(got.detach().cpu(), want.detach())
    print(f"FeedForward p={p}: output rel L2 {err:.2e}")
    assert err < 2e-2
    for name, a, b in zip(("dx", "dw1", "db1", "dw2", "db2", "dres", "drs"), gs, ts):
        err = _rel(a.grad.float().cpu(), b.grad)
        print(f"FeedForward p={p}: {name} rel L2 {err:.2e}")
        assert err < 3e-2, name


def test_feed_forward_p_zero_is_the_call_without_the_arguments():
    from modeling_utils import autograd as ag

    tensors, dy = _ff_tensors()
    a, b = _ff_gpu(tensors), _ff_gpu(tensors)
    ya, yb = ag.FeedForward.apply(*a), ag.FeedForward.apply(*b, False, 0.0, SEED, SITE)
    assert torch.equal(_bits(ya), _bits(yb))
    ya.backward(dy.cuda()), yb.backward(dy.cuda())
    for ta, tb in zip(a, b):
        assert torch.equal(_bits(ta.grad), _bits(tb.grad))


# ---- Mlp ----------------------------------------------------------------------------------------------------------------------------------
def _mlp_pair(backend, p=0.1):
    from modeling_utils.models.common import MlpConfig
    from tests.test_gpu_mlp import SHAPES, _fill_mlp_, _stock

    sizes, rows = SHAPES["70-130-65-33"]
    mlp = MlpConfig(hidden_sizes=sizes[1:-1], norm_layer="layer", activation_layer="gelu", dropout=p, dropout_backend=backend).build(sizes[0], sizes[-1])
    _fill_mlp_(mlp, 0)
    oracle = _stock(sizes, True, "gelu", 0.0)
    oracle.load_state_dict(mlp.state_dict())
    return mlp.cuda(), oracle.double(), sizes, rows


def test_mlp_hip_dropout_vs_float64_with_restated_masks():
    from tests.test_gpu_mlp import _x

    p = 0.1
    mlp, oracle, sizes, rows = _mlp_pair("hip", p)
    x, cot = _x(rows, sizes[0]), _x(rows, sizes[-1], seed=2)
    torch.manual_seed(11)
    got = mlp.train()(x.cuda())
    assert (mlp.hip_calls, mlp.stock_calls) == (1, 0)
    torch.manual_seed(11)
    key = int(torch.randint(0, 2**63 - 1, (1,), dtype=torch.int64).item())
    assert mlp.last_dropout_key == key                      # one draw from torch's default CPU generator
    # the stock modules in float64, every nn.Dropout replaced by the restated mask of its site
    want, block = x.double(), 0
    mods = list(oracle)
    for i, m in enumerate(mods):
        if isinstance(m, nn.Dropout):
            site = MLP_OUT_BLOCK if i == len(mods) - 1 else block
            want = want * multiplier(rows, want.shape[1], p, key, site)
            block += 1
        else:
            want = m(want)
    assert block == len(sizes) - 1
    err = _rel(got.detach().cpu(), want.detach())
    print(f"Mlp hip dropout p={p}: forward rel L2 {err:.2e}")
    assert err < 2e-2
    (want * cot.double()).sum().backward()
    (got * cot.cuda()).sum().backward()
    ref = dict(oracle.named_parameters())
    worst = {n: _rel(q.grad.cpu(), ref[n].grad) for n, q in mlp.named_parameters()}
    print(f"Mlp hip dropout p={p}: max gradient rel L2 {max(worst.values()):.2e}")
    assert all(v < 3e-2 for v in worst.values()), worst
    # eval: no dropout, no key drawn
    state = torch.get_rng_state()
    with torch.no_grad():
        assert _rel(mlp.eval()(x.cuda()).cpu(), oracle(x.double())) < 2e-2
    assert torch.equal(state, torch.get_rng_state()) and (mlp.hip_calls, mlp.stock_calls) == (2, 0)


def test_mlp_torch_backend_keeps_the_stock_route():
    from tests.test_gpu_mlp import _x

    mlp, _, sizes, rows = _mlp_pair("torch")
    with torch.no_grad():
        mlp.train()(_x(rows, sizes[0]).cuda())
    assert (mlp.hip_calls, mlp.stock_calls) == (0, 1) and mlp.last_dropout_key is None


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
FDIMS = {"text": (2, 40), "audio": (2, 24), "video": (2, 33)}
V, TOUT, S, B, T = 60, 13, 3, 2, 64
DEPTH = 2


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


def _step(model, batch, seed):
    """One training step under fixed seeds -> (loss, {name: gradient})."""
    from algonauts2025.pl_module import BrainModule
    from modeling_utils.losses import TorchLossConfig

    torch.manual_seed(seed)
    random.seed(seed)
    model.train().zero_grad(set_to_none=True)
    loss = BrainModule(model, TorchLossConfig(name="MSELoss").build(), None, {}).training_step(batch, 0)
    loss.backward()
    return loss.detach().clone(), {n: q.grad.clone() for n, q in model.named_parameters() if q.grad is not None}


def test_eval_ignores_every_dropout(batch):
    plain = _model(contrastive_enabled=True)
    dropped = _model(like=plain, contrastive_enabled=True, ff_dropout=0.2, layer_dropout=0.5, projector_dropout=0.1)
    with torch.no_grad():
        a, b = plain.eval()(batch), dropped.eval()(batch)
        assert torch.equal(_bits(a), _bits(b))
        c = dropped.train()(batch)                          # train mode under no_grad: the fused path, no dropout, no key
        assert torch.equal(_bits(a), _bits(c)) and dropped.last_dropout_key is None and dropped.last_layer_drops is None


def test_training_is_reproducible_from_the_seeds(batch):
    model = _model(contrastive_enabled=True, ff_dropout=0.2, layer_dropout=0.5, projector_dropout=0.1)
    loss_a, grads_a = _step(model, batch, 3)
    key_a = model.last_dropout_key
    loss_b, grads_b = _step(model, batch, 3)
    assert key_a is not None and model.last_dropout_key == key_a
    assert torch.equal(_bits(loss_a), _bits(loss_b)) and grads_a.keys() == grads_b.keys()
    assert all(torch.equal(_bits(grads_a[n]), _bits(grads_b[n])) for n in grads_a)
    loss_c, _ = _step(model, batch, 4)
    assert model.last_dropout_key != key_a and float(loss_c) != float(loss_a)


def test_one_call_per_site_and_the_backward_repeats_them(batch, monkeypatch):
    from algonauts2025.model import SITE_FF, SITE_HEAD, SITE_PROJECTOR
    from algonauts2025.pl_module import BrainModule
    from modeling_utils.losses import TorchLossConfig
    from tribe_hip import ops

    model = _model(contrastive_enabled=True, contrastive_modalities=["video"], ff_dropout=0.2, projector_dropout=0.1).train()
    calls = []
    real = ops.dropout_apply
    monkeypatch.setattr(ops, "dropout_apply", lambda x, p, seed, site, out=None: (calls.append((p, seed, site)), real(x, p, seed, site, out))[1])
    torch.manual_seed(6)
    loss = BrainModule(model, TorchLossConfig(name="MSELoss").build(), None, {}).training_step(batch, 0)
    forward = list(calls)
    calls.clear()
    loss.backward()
    backward = list(calls)
    mlp_sites = lambda kind, m: [(kind << 56) | (m << 16) | j for j in (0, MLP_OUT_BLOCK)]   # noqa: E731
    per_pass = sorted([(SITE_FF << 56) | i for i in range(DEPTH)] + [s for m in range(3) for s in mlp_sites(SITE_PROJECTOR, m)])
    keys = sorted({seed for _, seed, _ in forward}, key=[seed for _, seed, _ in forward].index)
    assert len(keys) == 2 and keys[1] == model.last_dropout_key              # the prediction pass and the contrastive pass: a key each
    assert sorted(site for _, seed, site in forward if seed == keys[0]) == per_pass
    assert sorted(site for _, seed, site in forward if seed == keys[1]) == sorted(per_pass + mlp_sites(SITE_HEAD, 2))
    assert len(set(forward)) == len(forward) == 2 * len(per_pass) + 2
    assert all(p == (0.2 if site >> 56 == SITE_FF else 0.1) for p, _, site in forward)
    assert sorted(backward) == sorted(forward)
    assert getattr(model, "shared_latent_hits", 0) == 0


def test_active_dropout_never_shares_contrastive_latents(batch):
    from algonauts2025.pl_module import BrainModule
    from modeling_utils.losses import TorchLossConfig

    for kw, hits in ((dict(), 1), (dict(ff_dropout=0.1), 0), (dict(layer_dropout=0.5), 0), (dict(projector_dropout=0.1), 0)):
        model = _model(contrastive_enabled=True, modality_dropout=0.0, **kw).train()
        torch.manual_seed(2)
        random.seed(2)
        BrainModule(model, TorchLossConfig(name="MSELoss").build(), None, {}).training_step(batch, 0)
        assert getattr(model, "shared_latent_hits", 0) == hits, kw


def test_zero_settings_leave_the_rng_stream_alone(batch):
    model = _model().train()
    torch.manual_seed(8)
    for _ in FDIMS:
        torch.rand(1)                                       # the modality-dropout draws: all a zero-dropout pass consumes
    want = torch.get_rng_state()
    torch.manual_seed(8)
    model(batch)
    assert torch.equal(torch.get_rng_state(), want) and model.last_dropout_key is None and model.last_layer_drops is None


def _count_calls(monkeypatch, fn):
    counter = []
    real = fn.apply
    monkeypatch.setattr(fn, "apply", lambda *a: (counter.append(a[0]), real(*a))[1])
    return counter


def test_layer_dropout_one_skips_the_whole_encoder(batch, monkeypatch):
    from modeling_utils import autograd as ag
    from tribe_hip import ops

    plain = _model().train()
    forks = _count_calls(monkeypatch, ag.ScaleNormFork)
    plain(batch)
    embedded = forks[0].detach().clone()                    # the encoder's input: the first block's fork
    assert len(forks) == 2 * DEPTH
    forks.clear()
    model = _model(like=plain, layer_dropout=1.0).train()
    x, _, _ = model._latents_autograd(batch.data)
    enc = model.encoder
    assert not forks and model.last_layer_drops == [True] * (2 * DEPTH)
    assert torch.equal(_bits(x), _bits(embedded))
    out = model(batch)
    want = ops.scalenorm(embedded, enc.final_norm.g.detach(), enc.final_norm.gain_scale, enc.final_norm.eps)
    head = ag.VoxelHead.apply(want.view(B, T, -1), model.predictor.weights.detach(), model.predictor.bias.detach(),
                              model.predictor.check_subjects(batch.data["subject_id"]))
    assert torch.equal(_bits(out), _bits(ag.AdaptivePool.apply(head, TOUT)))
    out.sum().backward()
    assert all(q.grad is None for q in enc.layers.parameters())
    assert enc.final_norm.g.grad is not None and all(q.grad is not None for q in model.projectors.parameters())


def test_layer_dropout_follows_python_random(batch, monkeypatch):
    from modeling_utils import autograd as ag

    for seed in range(50):                                  # a seed that keeps some sub-layers and skips others
        random.seed(seed)
        want = [random.random() < 0.5 for _ in range(2 * DEPTH)]
        if 0 < sum(want) < 2 * DEPTH and want[0::2] != want[1::2]:
            break
    model = _model(layer_dropout=0.5, ff_dropout=0.1).train()
    qkv, ff = _count_calls(monkeypatch, ag.QKVLinear), _count_calls(monkeypatch, ag.FeedForward)
    random.seed(seed)
    out = model(batch)
    assert model.last_layer_drops == want
    assert len(qkv) == want[0::2].count(False) and len(ff) == want[1::2].count(False)
    out.sum().backward()
    for i in range(2 * DEPTH):
        got = [q.grad is not None for q in model.encoder.layers[i].parameters()]
        assert got == [not want[i]] * len(got), i


@pytest.mark.parametrize("rows,dim", [(130, 768), (37, 3072), (50, 100)])
def test_scalenorm_gain_gradient_is_reproducible(rows, dim):
    """A seeded dropout run repeats its gradients bit for bit only if every backward kernel does: ScaleNorm's gain gradient is the
    fixed-order sum of tribe_scalenorm_bwd_ordered (register-resident rows at 768 / 3072, the generic kernel at 100)."""
    from modeling_utils import autograd as ag

    g = torch.Generator().manual_seed(rows)
    x, dy, gain = torch.randn(rows, dim, generator=g), torch.randn(rows, dim, generator=g), torch.tensor([1.3])
    xt, gt = x.double().requires_grad_(), gain.double().requires_grad_()
    (xt / xt.norm(dim=-1, keepdim=True).clamp(min=1e-12) * dim**0.5 * gt).backward(dy.double())
    grads = []
    for _ in range(3):
        xg, gg = x.cuda().requires_grad_(), gain.cuda().requires_grad_()
        ag.ScaleNorm.apply(xg, gg, dim**0.5, 1e-12, True).backward(dy.cuda())
        grads.append((xg.grad, gg.grad))
    assert _rel(grads[0][0].cpu(), xt.grad) < 1e-4 and _rel(grads[0][1].cpu(), gt.grad) < 1e-4   # the bounds of test_autograd_blocks_vs_torch
    assert all(torch.equal(_bits(a), _bits(grads[0][0])) and torch.equal(_bits(b), _bits(grads[0][1])) for a, b in grads[1:])
