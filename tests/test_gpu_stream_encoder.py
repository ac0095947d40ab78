"""GPU: causal encoders streamed step by step (HipEncoder.new_cache / prefill / step, FmriEncoder.stream) against the restated causal oracle
(tests/causal_restatement.py), with the cases and helpers of tests/test_gpu_causal_encoder.py: dim 768, depth 2, B 2, the q and out
projections scaled by ATTN_GAIN.

Three routes must each give the causal oracle's rows within the project's 2e-2 relative L2: `step` over all T positions; `prefill` of the
first T0 = T * 4 // 7 followed by steps; `prefill` of all T.  Power: the same steps differ from the NON-causal oracle by more than ten
times the bound, and a stream whose cache is reset() at T0 (it forgets the past and restarts at position 0) differs from the oracle beyond T0
by more than ten times the bound.

Model level: FmriEncoder(causal=True).stream(...) pushed step by step against `model.eval()(batch, pool_outputs=False)`'s columns and
against the causal tribe_ref oracle (un-pooled), _model_case's shapes (T = 64), with and without subject_embedding, feature_aggregation
`cat` and `sum`."""

import copy
import functools

import pytest
import torch

from oracle import tribe_ref, xt_encoder
from tests.causal_restatement import make_causal
from tests.test_gpu_causal_encoder import ATTN_GAIN, BOUND, CASES, DEPTH, DIM, FDIMS, TOUT, B, S, T, V, _encoder_case, _hip_encoder, _rel

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _plain_oracle(heads, T_, rotary):
    """The NON-causal oracle's output on _encoder_case's parameters and input: computed once, never modified."""
    state, x, *_ = _encoder_case(heads, T_, rotary)
    ref = xt_encoder.Encoder(dim=DIM, depth=DEPTH, heads=heads, attn_dim_head=DIM // heads, rotary_pos_emb=rotary).eval()
    ref.load_state_dict(state)
    with torch.no_grad():
        return ref(x)


def _steps(enc, cache, x, first, last):
    return torch.stack([enc.step(x[:, t], cache) for t in range(first, last)], dim=1)


@pytest.mark.parametrize("heads,T_,rotary", CASES)
def test_three_routes_vs_causal_oracle(heads, T_, rotary):
    state, x, want, t0, *_ = _encoder_case(heads, T_, rotary)
    assert ATTN_GAIN > 1 and t0 == T_ * 4 // 7
    enc = _hip_encoder(heads, rotary, state, True)
    xg = x.cuda()
    with torch.no_grad():
        cache = enc.new_cache(B, T_ + 3)
        stepped = _steps(enc, cache, xg, 0, T_).cpu()
        assert cache.pos == T_
        cache.reset()
        head = enc.prefill(xg[:, :t0], cache)
        assert cache.pos == t0 and head.shape == (B, t0, DIM)
        mixed = torch.cat([head, _steps(enc, cache, xg, t0, T_)], dim=1).cpu()
        assert cache.pos == T_
        tight = enc.new_cache(B, T_)                                                  # capacity exactly T: the last slot is used
        whole = enc.prefill(xg, tight).cpu()
        assert tight.pos == T_
        # a stream that forgets the past at T0
        cache.reset()
        _steps(enc, cache, xg, 0, t0)
        cache.reset()
        forgot = _steps(enc, cache, xg, t0, T_).cpu()
    errs = {"step": _rel(stepped, want), "prefill + step": _rel(mixed, want), "prefill": _rel(whole, want)}
    tail = {"step": _rel(stepped[:, t0:], want[:, t0:]), "prefill + step": _rel(mixed[:, t0:], want[:, t0:])}
    power = _rel(stepped, _plain_oracle(heads, T_, rotary))
    reset_power = _rel(forgot, want[:, t0:])
    print(f"heads={heads} T={T_} rotary={rotary}: vs causal oracle {errs}; rows >= T0 alone {tail}; steps vs NON-causal oracle {power:.2e}; "
          f"reset at T0={t0} vs oracle beyond T0 {reset_power:.2e}")
    assert max(errs.values()) < BOUND and max(tail.values()) < BOUND
    assert power > 10 * BOUND
    assert reset_power > 10 * BOUND


def test_step_is_deterministic_and_past_max_len_raises():
    heads, T_, rotary = CASES[0]
    state, x, *_ = _encoder_case(heads, T_, rotary)
    enc = _hip_encoder(heads, rotary, state, True)
    xg = x.cuda()
    with torch.no_grad():
        a_cache, b_cache = enc.new_cache(B, 9), enc.new_cache(B, 9)
        a = _steps(enc, a_cache, xg, 0, 9)
        b = _steps(enc, b_cache, xg, 0, 9)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(a_cache.k.view(torch.int16), b_cache.k.view(torch.int16)) and torch.equal(a_cache.v.view(torch.int16), b_cache.v.view(torch.int16))
        with pytest.raises(ValueError, match="run past max_len=9"):
            enc.step(xg[:, 9], a_cache)
        with pytest.raises(ValueError, match="x is on cpu, the cache on cuda"):
            enc.step(x[:, 0], b_cache)


# ---- the model --------------------------------------------------------------------------------------------------------------------------
VARIANTS = [(False, "cat"), (True, "cat"), (False, "sum"), (True, "sum")]


@functools.lru_cache(maxsize=None)
def _variant_case(subject_embedding, aggregation):
    """(state_dict, data, the causal oracle's un-pooled output [B, V, T]) -- _model_case's shapes, draws and seeds."""
    ref = tribe_ref.FmriEncoderRef(FDIMS, V, TOUT, S, feature_aggregation=aggregation, subject_embedding=subject_embedding,
                                   dims=tribe_ref.EncoderDims(hidden=768, depth=DEPTH, heads=4)).eval()
    with torch.no_grad():
        tribe_ref.fill_params_(ref, seed=2)
    state = copy.deepcopy(ref.state_dict())
    data = tribe_ref.synthetic_batch(B, T, FDIMS, S, seed=4)
    make_causal(ref.encoder)
    with torch.no_grad():
        return state, data, ref(data, pool_outputs=False)


@pytest.mark.parametrize("subject_embedding,aggregation", VARIANTS)
def test_model_stream_vs_eval_forward_and_causal_oracle(subject_embedding, aggregation):
    from algonauts2025.model import FmriEncoderConfig
    from data_utils.dataloader import SegmentData

    state, data, want = _variant_case(subject_embedding, aggregation)
    model = FmriEncoderConfig(n_subjects=S, hidden=768, depth=DEPTH, heads=4, causal=True, subject_embedding=subject_embedding,
                              feature_aggregation=aggregation).build(FDIMS, V, TOUT)
    model.load_state_dict(state)
    model = model.cuda().eval()
    gpu = {k: v.cuda() for k, v in data.items()}
    with torch.no_grad():
        full = model(SegmentData(data=gpu, segments=[None] * B), pool_outputs=False).float().cpu()
    assert full.shape == (B, V, T)

    def at(t0, t1):
        return {k: (v if k == "subject_id" else v[..., t0:t1].contiguous()) for k, v in gpu.items()}

    stream = model.stream(B, max_len=T)
    cols = []
    for t in range(T):
        out = stream.push(at(t, t + 1))
        assert out.shape == (B, V) and out.dtype == torch.float32 and stream.pos == t + 1
        cols.append(out)
    pushed = torch.stack(cols, dim=2).cpu()
    stream.reset()
    t0 = T * 4 // 7
    head = stream.prefill(at(0, t0))
    assert head.shape == (B, V, t0) and stream.pos == t0
    mixed = torch.cat([head] + [stream.push(at(t, t + 1))[:, :, None] for t in range(t0, T)], dim=2).cpu()
    errs = {"push vs eval forward": _rel(pushed, full), "push vs oracle": _rel(pushed, want), "prefill + push vs oracle": _rel(mixed, want),
            "eval forward vs oracle": _rel(full, want)}
    print(f"subject_embedding={subject_embedding} {aggregation}: {errs}")
    assert max(errs.values()) < BOUND
    with pytest.raises(ValueError, match="run past max_len"):
        stream.push(at(0, 1))
