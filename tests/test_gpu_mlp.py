"""GPU: MlpConfig(hidden_sizes=...).build() on its HIP route and FmriEncoderConfig.projector_hidden_sizes, against stock torch
modules with the same parameters on the CPU (float64 for the MLP alone, the fp32 oracle model for the encoder).

Bounds are the project's (tests/test_gpu_training.py): relative L2 below 2e-2 for outputs, below 3e-2 per gradient tensor.  A CPU
emulation of the route (bf16 rounding of every GEMM operand and inter-layer activation, three seeds, the shapes below) stays at or
below 4.2e-3 forward and 6.3e-3 for the gradients of GELU, ELU and identity; ReLU gradients reach 4e-2 .. 1e-1 because operand
rounding flips pre-activations across zero -- a property of ReLU under bf16 operands, not of a kernel -- so ReLU is checked forward
only here and its backward per element in tests/test_gpu_mlp_kernels.py.

In-place updates reach the next forward through the version-keyed packs (modeling_utils.autograd.PACKS), i.e. through torch's version
counter: the updates below are tracked in-place operations (`with torch.no_grad(): p.mul_(1.5)`, what optimisers and load_state_dict
do).  A write through `p.data` is invisible to that counter by torch's design and to every pack cache of this project with it.
"""

import pytest
import torch
from torch import nn

from oracle import tribe_ref

pytestmark = pytest.mark.gpu

SHAPES = {"200-192-96": ([200, 192, 96], 300), "70-130-65-33": ([70, 130, 65, 33], 37), "2048-1024-512": ([2048, 1024, 512], 300)}
ACTS = {"gelu": nn.GELU, "relu": nn.ReLU, "elu": nn.ELU, None: nn.Identity}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _stock(sizes, norm, act, dropout=0.0):
    """Hand-assembled stock modules in torchvision.ops.MLP's order."""
    layers = []
    for i, o in zip(sizes[:-2], sizes[1:-1]):
        layers.append(nn.Linear(i, o))
        if norm:
            layers.append(nn.LayerNorm(o))
        layers += [ACTS[act](), nn.Dropout(dropout)]
    layers += [nn.Linear(sizes[-2], sizes[-1]), nn.Dropout(dropout)]
    return nn.Sequential(*layers)


def _fill_mlp_(module, seed):
    """Seeded parameters: Linear U(+-1/sqrt(fan_in)), LayerNorm gain N(1, 0.3) and bias N(0, 0.3)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.Linear):
                bound = m.in_features ** -0.5
                m.weight.copy_((torch.rand(m.weight.shape, generator=g) * 2 - 1) * bound)
                m.bias.copy_((torch.rand(m.bias.shape, generator=g) * 2 - 1) * bound)
            elif isinstance(m, nn.LayerNorm):
                m.weight.copy_(1.0 + 0.3 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g))


def _pair(sizes, norm, act, seed=0, dropout=0.0):
    """(Mlp on the GPU, float64 stock oracle on the CPU) with equal parameters."""
    from modeling_utils.models.common import MlpConfig

    mlp = MlpConfig(hidden_sizes=sizes[1:-1], norm_layer="layer" if norm else None, activation_layer=act, dropout=dropout).build(sizes[0], sizes[-1])
    _fill_mlp_(mlp, seed)
    oracle = _stock(sizes, norm, act, dropout)
    oracle.load_state_dict(mlp.state_dict())
    return mlp.cuda(), oracle.double()


def _x(rows, width, seed=1):
    return torch.randn(rows, width, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_mlp_forward_and_gradients(shape, norm, act):
    sizes, rows = SHAPES[shape]
    mlp, oracle = _pair(sizes, norm, act)
    x = _x(rows, sizes[0])
    cot = _x(rows, sizes[-1], seed=2)                       # cotangent of the output
    want = oracle(x.double())
    mlp.train()                                             # dropout == 0: still the HIP route
    got = mlp(x.cuda())
    assert got.dtype == torch.float32 and got.shape == want.shape and (mlp.hip_calls, mlp.stock_calls) == (1, 0)
    err = _rel(got.detach().cpu(), want.detach())
    print(f"{shape} norm={norm} act={act}: forward rel L2 {err:.2e}")
    assert err < 2e-2
    if act == "relu":
        return
    (want * cot.double()).sum().backward()
    (got * cot.cuda()).sum().backward()
    ref_grads = dict(oracle.named_parameters())
    worst = {n: _rel(p.grad.cpu(), ref_grads[n].grad) for n, p in mlp.named_parameters()}
    print(f"{shape} norm={norm} act={act}: max gradient rel L2 {max(worst.values()):.2e}")
    assert all(v < 3e-2 for v in worst.values()), worst


def test_input_gradient():
    sizes, rows = SHAPES["200-192-96"]
    mlp, oracle = _pair(sizes, True, "gelu")
    x = _x(rows, sizes[0])
    xg, xc = x.cuda().requires_grad_(), x.double().requires_grad_()
    cot = _x(rows, sizes[-1], seed=2)
    (mlp(xg) * cot.cuda()).sum().backward()
    (oracle(xc) * cot.double()).sum().backward()
    assert xg.grad.dtype == torch.float32 and _rel(xg.grad.cpu(), xc.grad) < 3e-2
    ref_grads = dict(oracle.named_parameters())
    assert all(_rel(p.grad.cpu(), ref_grads[n].grad) < 3e-2 for n, p in mlp.named_parameters())


def test_dropout_routes():
    sizes, rows = SHAPES["70-130-65-33"]
    mlp, oracle = _pair(sizes, True, "gelu", dropout=0.1)
    x = _x(rows, sizes[0])
    with torch.no_grad():
        got = mlp.eval()(x.cuda())                           # inactive dropout: HIP
        assert (mlp.hip_calls, mlp.stock_calls) == (1, 0)
        assert _rel(got.cpu(), oracle.eval()(x.double())) < 2e-2
        out = mlp.train()(x.cuda())                          # active dropout: the stock modules
        assert (mlp.hip_calls, mlp.stock_calls) == (1, 1) and out.shape == got.shape
        mlp.cpu()(x)                                         # CPU tensors: stock as well
        assert (mlp.hip_calls, mlp.stock_calls) == (1, 2)


def test_in_place_updates_reach_the_next_forward():
    sizes, rows = SHAPES["200-192-96"]
    x = _x(rows, sizes[0])
    # a hidden weight (without a norm, which would undo most of a rescaling, and with one), then a LayerNorm gain
    for norm, names in ((False, ["0.weight"]), (True, ["0.weight", "1.weight"])):
        mlp, oracle = _pair(sizes, norm, "gelu")
        with torch.no_grad():
            assert _rel(mlp(x.cuda()).cpu(), oracle(x.double())) < 2e-2      # packs are built here
            before = oracle(x.double())
            for name in names:
                dict(mlp.named_parameters())[name].mul_(1.5)
                dict(oracle.named_parameters())[name].mul_(1.5)
                want = oracle(x.double())
                if (norm, name) != (True, "0.weight"):
                    assert _rel(want, before) > 1e-1                         # a stale pack would miss the bound below
                assert _rel(mlp(x.cuda()).cpu(), want) < 2e-2, (norm, name)
                before = want
            fresh, _ = _pair(sizes, norm, "gelu", seed=5)                    # load_state_dict writes in place as well
            mlp.load_state_dict(fresh.state_dict())
            oracle.load_state_dict(fresh.state_dict())
            assert _rel(mlp(x.cuda()).cpu(), oracle(x.double())) < 2e-2


def test_bf16_and_3d_inputs():
    sizes, _ = SHAPES["70-130-65-33"]
    mlp, _ = _pair(sizes, True, "gelu")
    x = torch.randn(3, 13, sizes[0], generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        flat = mlp(x.reshape(39, -1))
        assert torch.equal(mlp(x), flat.view(3, 13, -1))
        # the f32 input is rounded to bf16 (nearest even) as the first GEMM's operand: handing that rounding in changes nothing
        y16 = mlp(x.bfloat16())
        assert y16.dtype == torch.float32 and torch.equal(y16, mlp(x.bfloat16().float()))
        assert torch.equal(y16, mlp(x))


# ---- the encoder with projector_hidden_sizes ----------------------------------------------------------------------------------------
FDIMS = {"text": (2, 96), "audio": (2, 80), "video": (1, 72)}
V, TOUT, S, B, T = 50, 10, 4, 3, 40
HIDDEN_SIZES = [160, 100]


def _models(fdims=FDIMS, agg="cat", modality_dropout=0.0, contrastive=True):
    """(HIP model on the GPU, fp32 oracle) whose projectors and contrastive head are [in, 160, 100, out] LayerNorm / GELU MLPs with the
    same weights: the oracle applies its projectors as plain modules, so stock nn.Sequential ones are swapped in."""
    from algonauts2025.model import FmriEncoderConfig

    ref = tribe_ref.FmriEncoderRef(fdims, V, TOUT, S, feature_aggregation=agg, contrastive_modalities=["video"] if contrastive else [],
                                   dims=tribe_ref.EncoderDims(hidden=768, depth=2, heads=2))
    with torch.no_grad():
        tribe_ref.fill_params_(ref, seed=3)
    for i, (group, width) in enumerate(((ref.projectors, None), (ref.contrastive_heads, 768))):
        for j, m in enumerate(list(group)):
            lin = group[m]
            group[m] = _stock([lin.in_features] + HIDDEN_SIZES + [lin.out_features], True, "gelu")
            _fill_mlp_(group[m], 10 * i + j)
    model = FmriEncoderConfig(hidden=768, depth=2, heads=2, n_subjects=S, projector_hidden_sizes=HIDDEN_SIZES, contrastive_enabled=contrastive,
                              feature_aggregation=agg, modality_dropout=modality_dropout).build(fdims, V, TOUT)
    model.load_state_dict(ref.state_dict())
    return model.cuda(), ref


def _batch(data, **extra):
    from data_utils.dataloader import SegmentData

    return SegmentData(data={**{k: v.cuda() for k, v in data.items()}, **{k: v.cuda() for k, v in extra.items()}}, segments=[None] * B)


@pytest.mark.parametrize("agg", ["cat", "sum"])
def test_model_inference(agg):
    model, ref = _models(agg=agg)
    model.eval(), ref.eval()
    data = tribe_ref.synthetic_batch(B, T, FDIMS, S, seed=1)
    with torch.no_grad():
        want, want_nce = ref(data), ref.compute_contrastive_loss(data)["video"]
        got = model(_batch(data)).cpu()
        nce = model.compute_contrastive_loss(_batch(data))["video"]
    assert got.shape == (B, V, TOUT) and _rel(got, want) < 2e-2
    assert abs(float(nce) - float(want_nce)) < 2e-2 * abs(float(want_nce))
    with torch.no_grad():
        assert _rel(model.aggregate_features(_batch(data)).cpu(), ref.aggregate_features(data)) < 2e-2


def test_model_inference_missing_modality():
    fdims = {"text": (2, 96), "audio": None, "video": (1, 72)}
    model, ref = _models(fdims=fdims)
    model.eval(), ref.eval()
    data = tribe_ref.synthetic_batch(B, T, fdims, S, seed=1)
    with torch.no_grad():
        assert _rel(model(_batch(data)).cpu(), ref(data)) < 2e-2


def test_model_inference_modality_dropout():
    p = 0.5
    for seed in range(50):                                   # a seed whose draw drops some modalities, not all (CPU RNG only)
        torch.manual_seed(seed)
        dropped = [m for m in FDIMS if torch.rand(1).item() < p]
        if 0 < len(dropped) < len(FDIMS):
            break
    model, ref = _models(modality_dropout=p)
    model.train(), ref.eval()
    data = tribe_ref.synthetic_batch(B, T, FDIMS, S, seed=1)
    with torch.no_grad():
        x = ref.transformer_forward(ref.aggregate_features(data, dropped=dropped), data["subject_id"])
        want = tribe_ref.adaptive_avg_pool1d(ref.predictor(x.transpose(1, 2), data["subject_id"]), TOUT)
        torch.manual_seed(seed)
        got = model(_batch(data)).cpu()                      # no grad: the inference route, with the training-mode draw
    assert _rel(got, want) < 2e-2


@pytest.mark.parametrize("contrastive", [False, True])
def test_model_training_step_and_adam(contrastive):
    from algonauts2025.pl_module import BrainModule
    from modeling_utils.losses import TorchLossConfig
    from modeling_utils.optim import HipAdam

    model, ref = _models(contrastive=contrastive)
    model.train(), ref.train()
    data = tribe_ref.synthetic_batch(B, T, FDIMS, S, seed=4)
    fmri = torch.randn(B, V, TOUT, generator=torch.Generator().manual_seed(9))
    loss_ref, *_ = tribe_ref.run_step(ref(data), fmri, data["subject_id"])
    if contrastive:
        loss_ref = loss_ref + 0.1 * ref.compute_contrastive_loss(data)["video"]
    opt_ref, opt = torch.optim.Adam(ref.parameters(), lr=1e-3), HipAdam(model.parameters(), lr=1e-3)
    loss_ref.backward()
    loss = BrainModule(model, TorchLossConfig(name="MSELoss").build(), None, {}).training_step(_batch(data, fmri=fmri), 0)
    assert abs(float(loss.detach()) - float(loss_ref.detach())) < 1e-2 * float(loss_ref.detach())
    loss.backward()
    ref_grads = dict(ref.named_parameters())
    trunk = {n: _rel(p.grad.cpu(), ref_grads[n].grad) for n, p in model.named_parameters() if n.startswith(("projectors.", "contrastive_heads."))}
    assert len(trunk) == 10 * (4 if contrastive else 3)
    print(f"contrastive={contrastive}: max projector gradient rel L2 {max(trunk.values()):.2e}")
    assert all(v < 3e-2 for v in trunk.values()), {k: v for k, v in trunk.items() if v >= 3e-2}
    opt_ref.step(), opt.step()
    model.eval(), ref.eval()
    data = tribe_ref.synthetic_batch(B, T, FDIMS, S, seed=5)
    with torch.no_grad():
        assert _rel(model(_batch(data)).cpu(), ref(data)) < 2e-2


def test_default_path_is_bit_identical():
    from algonauts2025.model import FmriEncoderConfig

    outs = []
    data = tribe_ref.synthetic_batch(B, T, FDIMS, S, seed=1)
    for kw in ({}, {"projector_hidden_sizes": None}):
        torch.manual_seed(0)
        model = FmriEncoderConfig(hidden=768, depth=2, heads=2, n_subjects=S, **kw).build(FDIMS, V, TOUT).cuda().eval()
        with torch.no_grad():
            outs.append(model(_batch(data)))
    assert torch.equal(outs[0], outs[1])
