"""GPU: blocks of positions appended to the cache of a streamed causal encoder (HipEncoder.extend, EncoderStream.push_block) against the
restated causal oracle (tests/causal_restatement.py), with the cases and helpers of tests/test_gpu_causal_encoder.py: dim 768, depth 2, B 2,
the q and out projections scaled by ATTN_GAIN.

Three schedules must each give the causal oracle's rows, and HipEncoder.forward's, within the project's 2e-2 relative L2: prefill(T0),
extend(k1), step, extend(k2); extend alone from an empty cache; extend(k = 1) at every position.  After cache.reset() the same schedule
reproduces its bits.  Power: the NON-causal module differs from the causal oracle by more than ten times the bound.

Model level: FmriEncoder(causal=True).stream(...).push_block after a prefill against `model.eval()(batch, pool_outputs=False)`'s columns and
the causal tribe_ref oracle (un-pooled), with and without a subject embedding, feature_aggregation `cat` and `sum`."""

import pytest
import torch

from tests.test_gpu_causal_encoder import ATTN_GAIN, BOUND, CASES, DEPTH, DIM, FDIMS, TOUT, B, S, T, V, _encoder_case, _hip_encoder, _rel
from tests.test_gpu_stream_encoder import VARIANTS, _variant_case

pytestmark = pytest.mark.gpu


def _mixed(enc, cache, x, T_):
    """prefill(T0), extend(k1), step, extend(k2): T0 = T * 4 // 7, k1 crosses a 16-row wave, k2 takes what is left."""
    t0 = T_ * 4 // 7
    k1 = 17
    parts = [enc.prefill(x[:, :t0], cache), enc.extend(x[:, t0:t0 + k1], cache), enc.step(x[:, t0 + k1], cache)[:, None]]
    assert cache.pos == t0 + k1 + 1
    parts.append(enc.extend(x[:, t0 + k1 + 1:], cache))
    return torch.cat(parts, dim=1)


def _alone(enc, cache, x, T_):
    return enc.extend(x, cache)


def _ones(enc, cache, x, T_):
    return torch.cat([enc.extend(x[:, t:t + 1], cache) for t in range(T_)], dim=1)


SCHEDULES = {"prefill + extend + step + extend": _mixed, "extend alone": _alone, "extend(k=1) repeatedly": _ones}


@pytest.mark.parametrize("heads,T_,rotary", CASES)
def test_schedules_vs_causal_oracle_and_forward(heads, T_, rotary):
    state, x, want, *_ = _encoder_case(heads, T_, rotary)
    assert ATTN_GAIN > 1
    enc = _hip_encoder(heads, rotary, state, True)
    xg = x.cuda()
    with torch.no_grad():
        forward = enc(xg).cpu()
        plain = _hip_encoder(heads, rotary, state, False)(xg).cpu()
        cache = enc.new_cache(B, T_)                                                  # capacity exactly T: the last slot is used
        for name, schedule in SCHEDULES.items():
            cache.reset()
            got = schedule(enc, cache, xg, T_)
            assert cache.pos == T_ and got.shape == (B, T_, DIM) and got.dtype == torch.float32
            cache.reset()
            again = schedule(enc, cache, xg, T_)
            assert torch.equal(got.view(torch.int32), again.view(torch.int32)), f"{name}: the same schedule after reset() differs"
            errs = _rel(got.cpu(), want), _rel(got.cpu(), forward)
            print(f"heads={heads} T={T_} rotary={rotary} {name}: vs causal oracle {errs[0]:.2e}, vs HipEncoder.forward {errs[1]:.2e}")
            assert max(errs) < BOUND, name
        with pytest.raises(ValueError, match=f"run past max_len={T_}"):
            enc.extend(xg[:, :1], cache)
    power = _rel(plain, want)
    print(f"heads={heads} T={T_} rotary={rotary}: non-causal module vs causal oracle {power:.2e}")
    assert power > 10 * BOUND


# ---- the model --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subject_embedding,aggregation", VARIANTS)
def test_model_push_block_vs_eval_forward_and_causal_oracle(subject_embedding, aggregation):
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
    t0 = T * 4 // 7
    edges = [t0, t0 + 1, t0 + 18, T]                                                # after the prefill: blocks of 1, 17 and the rest
    parts = [stream.prefill(at(0, t0))]
    for lo, hi in zip(edges[:-1], edges[1:]):
        out = stream.push_block(at(lo, hi))
        assert out.shape == (B, V, hi - lo) and out.dtype == torch.float32 and stream.pos == hi
        parts.append(out)
    blocks = torch.cat(parts, dim=2).cpu()
    stream.reset()
    whole = stream.push_block(at(0, T)).cpu()                                         # pos = 0: a prefill through this route
    errs = {"prefill + push_block vs eval forward": _rel(blocks, full), "prefill + push_block vs oracle": _rel(blocks, want),
            "push_block alone vs oracle": _rel(whole, want), "eval forward vs oracle": _rel(full, want)}
    print(f"subject_embedding={subject_embedding} {aggregation}: {errs}")
    assert max(errs.values()) < BOUND
    with pytest.raises(ValueError, match="run past max_len"):
        stream.push_block(at(0, 1))
