"""GPU: independent timelines in one KV cache (HipEncoder.new_slots / step_slots / extend_slots, FmriEncoder.stream(independent=True))
against the restated causal oracle, with the cases and helpers of tests/test_gpu_causal_encoder.py: dim 768, depth 2, the q and out
projections scaled by ATTN_GAIN, BOUND = 2e-2 relative L2.  The oracle is causal, so the rows of a shorter timeline are a prefix of its rows
on the full input.

Staggered run, three slots: slot 0 follows x[0] from call 0 for 40 steps, is reset and follows x[1] from its position 0; slot 1 is inactive
for 5 calls and then follows x[1]; slot 2 starts at call 11 on x[0], takes its first 16 positions as one extend_slots block and then steps.
Every slot's rows are within BOUND of the oracle rows of its own timeline.  Power: without the reset the refilled timeline differs from the
oracle by more than 10 * BOUND (the reset check of tests/test_gpu_stream_encoder.py applied to one slot).

Bit equality: with all slots active from position 0 the slot entry points give the outputs and caches of `step` / `extend`.  Inactive slots:
output rows exactly zero, cache runs and positions unchanged.  Two identical schedules give equal bits.

Model: _model_case's shapes (T = 64), with and without subject_embedding, `cat` and `sum`: a two-slot stream whose slot 1 starts 9 calls late
and which pushes one block of 8 in the middle, each slot against `model.eval()(batch, pool_outputs=False)`'s columns of its own timeline.
Power: the uniform EncoderStream can start a timeline late only by pushing it at the positional rows of the global call index (9 steps of
zero features first); its first outputs for that timeline differ from the columns by more than 10 * BOUND."""

import pytest
import torch

from tests.test_gpu_causal_encoder import BOUND, CASES, DIM, FDIMS, TOUT, B, S, T, V, _encoder_case, _hip_encoder, _rel
from tests.test_gpu_stream_encoder import VARIANTS, _variant_case

pytestmark = pytest.mark.gpu

CALLS, FIRST_LEN, LATE, START2, BLOCK2 = 60, 40, 5, 11, 16


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _staggered(enc, xg, max_len, reset=True):
    """The schedule of the module docstring; returns (slots, {(slot, timeline): rows [n, DIM]}, every output [B=3, DIM] of the step calls)."""
    slots = enc.new_slots(3, max_len)
    zeros = torch.zeros(DIM, device="cuda")
    rows = {(0, 0): [], (0, 1): [], (1, 1): [], (2, 0): []}
    outs = []
    for call in range(CALLS):
        if call == FIRST_LEN and reset:
            slots.reset([0])
        line0 = 0 if call < FIRST_LEN else 1
        t0 = call if call < FIRST_LEN else call - FIRST_LEN                            # slot 0's step within its timeline
        active = [True, call >= LATE, call > START2]
        if call == START2:                                                            # slot 2's first 16 positions at once, alone
            block = torch.zeros(3, BLOCK2, DIM, device="cuda")
            block[2] = xg[0, :BLOCK2]
            before = list(slots.positions)
            y = enc.extend_slots(block, slots, active=[2])
            assert slots.positions == before[:2] + [BLOCK2]
            assert bool((y[:2] == 0).all())
            rows[(2, 0)].extend(y[2])
        x = torch.stack([xg[line0, t0], xg[1, call - LATE] if active[1] else zeros,
                         xg[0, BLOCK2 + call - START2 - 1] if active[2] else zeros])
        y = enc.step_slots(x, slots, active=active if call % 2 else [b for b in range(3) if active[b]])   # mask and indices alike
        outs.append(y)
        rows[(0, line0)].append(y[0])
        if active[1]:
            rows[(1, 1)].append(y[1])
        if active[2]:
            rows[(2, 0)].append(y[2])
        for b in range(3):
            if not active[b]:
                assert bool((_bits(y[b]) == 0).all()), (call, b, "the row of an inactive slot is not zero")
    return slots, {key: torch.stack(val).cpu() for key, val in rows.items()}, torch.stack(outs)


@pytest.mark.parametrize("heads,T_,rotary", [CASES[0], CASES[2]])
def test_staggered_slots_vs_causal_oracle(heads, T_, rotary):
    state, x, want, *_ = _encoder_case(heads, T_, rotary)
    enc = _hip_encoder(heads, rotary, state, True)
    xg = x.cuda()
    with torch.no_grad():
        slots, rows, _ = _staggered(enc, xg, T_)
        _, kept, _ = _staggered(enc, xg, T_, reset=False)
    assert slots.positions == [CALLS - FIRST_LEN, CALLS - LATE, BLOCK2 + CALLS - START2 - 1]
    assert {key: len(val) for key, val in rows.items()} == {(0, 0): FIRST_LEN, (0, 1): CALLS - FIRST_LEN, (1, 1): CALLS - LATE,
                                                            (2, 0): BLOCK2 + CALLS - START2 - 1}
    errs = {key: _rel(val, want[key[1], : len(val)]) for key, val in rows.items()}
    power = _rel(kept[(0, 1)], want[1, : CALLS - FIRST_LEN])
    print(f"heads={heads} T={T_} rotary={rotary}: (slot, timeline) vs the causal oracle's rows of that timeline {errs}; "
          f"slot 0 refilled without a reset {power:.2e}")
    assert max(errs.values()) < BOUND
    assert power > 10 * BOUND


def test_two_identical_schedules_give_equal_bits():
    heads, T_, rotary = CASES[0]
    state, x, *_ = _encoder_case(heads, T_, rotary)
    enc = _hip_encoder(heads, rotary, state, True)
    with torch.no_grad():
        a_slots, _, a = _staggered(enc, x.cuda(), T_)
        b_slots, _, b = _staggered(enc, x.cuda(), T_)
    assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(a_slots.k), _bits(b_slots.k)) and torch.equal(_bits(a_slots.v), _bits(b_slots.v))


@pytest.mark.parametrize("heads,T_,rotary", [CASES[0], CASES[2]])
def test_all_slots_active_gives_the_bits_of_step_and_extend(heads, T_, rotary):
    state, x, *_ = _encoder_case(heads, T_, rotary)
    enc = _hip_encoder(heads, rotary, state, True)
    xg = x.cuda()
    with torch.no_grad():
        cache, slots = enc.new_cache(B, 12), enc.new_slots(B, 12)
        for t in range(9):
            want, got = enc.step(xg[:, t], cache), enc.step_slots(xg[:, t], slots)
            assert torch.equal(_bits(got), _bits(want)), t
        assert slots.positions == [9] * B and cache.pos == 9
        assert torch.equal(_bits(slots.k), _bits(cache.k)) and torch.equal(_bits(slots.v), _bits(cache.v))
        cache, slots = enc.new_cache(B, 12), enc.new_slots(B, 12)
        for t in (0, 5):
            want, got = enc.extend(xg[:, t:t + 5], cache), enc.extend_slots(xg[:, t:t + 5], slots)
            assert torch.equal(_bits(got), _bits(want)), t
        assert slots.positions == [10] * B and cache.pos == 10
        assert torch.equal(_bits(slots.k), _bits(cache.k)) and torch.equal(_bits(slots.v), _bits(cache.v))


def test_step_slots_gives_the_bits_of_step_on_a_filled_cache_at_dim_head_384():
    """dim_head 384, B = 16 at position 255 of caches filled with random keys and values: the decode attention runs split over workgroups
    (4 splits here) and through the combine kernel, which the nine steps from an empty cache above never reach."""
    heads, T_, rotary = CASES[0]
    state, *_ = _encoder_case(heads, T_, rotary)
    enc = _hip_encoder(heads, rotary, state, True)
    assert enc.dim_head == 384
    nb, pos = 16, 255
    g = torch.Generator(device="cuda").manual_seed(3)
    with torch.no_grad():
        cache, slots = enc.new_cache(nb, pos + 1), enc.new_slots(nb, pos + 1)
        cache.k.copy_(torch.randn(cache.k.shape, generator=g, device="cuda"))
        cache.v.copy_(torch.randn(cache.v.shape, generator=g, device="cuda"))
        slots.k.copy_(cache.k)
        slots.v.copy_(cache.v)
        cache.pos, slots.positions = pos, [pos] * nb
        x = torch.randn(nb, DIM, generator=g, device="cuda")
        want, got = enc.step(x, cache), enc.step_slots(x, slots)
    from tribe_hip import ops

    assert ops.attention_decode_splits(nb, heads, pos + 1) > 1
    differ = int((_bits(got) != _bits(want)).sum())
    print(f"step_slots vs step at B={nb}, pos={pos}, dim_head 384: {differ} of {got.numel()} outputs differ")
    assert differ == 0
    assert torch.equal(_bits(slots.k), _bits(cache.k)) and torch.equal(_bits(slots.v), _bits(cache.v))


def test_inactive_slots_are_left_alone():
    heads, T_, rotary = CASES[0]
    state, x, *_ = _encoder_case(heads, T_, rotary)
    enc = _hip_encoder(heads, rotary, state, True)
    xg = torch.cat([x, x.flip(0)])[:3].cuda()                                         # three timelines
    with torch.no_grad():
        slots = enc.new_slots(3, 24)
        enc.extend_slots(xg[:, :4], slots)
        enc.step_slots(xg[:, 4], slots, active=[1])                                   # positions 4, 5, 4
        k0, v0 = slots.k.clone(), slots.v.clone()
        y = enc.step_slots(xg[:, 5], slots, active=[0, 2])
        assert slots.positions == [5, 5, 5]
        assert bool((_bits(y[1]) == 0).all()) and bool((y[0] != 0).any()) and bool((y[2] != 0).any())
        assert torch.equal(_bits(slots.k[:, 1]), _bits(k0[:, 1])) and torch.equal(_bits(slots.v[:, 1]), _bits(v0[:, 1]))
        assert not torch.equal(_bits(slots.k[:, 0]), _bits(k0[:, 0])) and not torch.equal(_bits(slots.v[:, 2]), _bits(v0[:, 2]))
        k0, v0 = slots.k.clone(), slots.v.clone()
        y = enc.extend_slots(xg[:, 6:13], slots, active=[False, True, False])
        assert slots.positions == [5, 12, 5] and y.shape == (3, 7, DIM)
        assert bool((_bits(y[0]) == 0).all()) and bool((_bits(y[2]) == 0).all()) and bool((y[1] != 0).any())
        for b in (0, 2):
            assert torch.equal(_bits(slots.k[:, b]), _bits(k0[:, b])) and torch.equal(_bits(slots.v[:, b]), _bits(v0[:, b]))
        # whatever an inactive slot's input row holds, it reaches nothing: not the other rows, not its own cache run
        k0, v0 = slots.k.clone(), slots.v.clone()
        dirty = xg[:, 13].clone()
        dirty[1] = float("nan")
        a = enc.step_slots(dirty, slots, active=[0, 2])
        assert bool(torch.isfinite(a).all()) and torch.equal(_bits(slots.k[:, 1]), _bits(k0[:, 1]))
        with pytest.raises(ValueError, match=r"slot 1: 12 positions filled \+ 13 would run past max_len=24"):
            enc.extend_slots(xg[:, :13], slots)
        with pytest.raises(ValueError, match="x is on cpu, the slots on cuda"):
            enc.step_slots(x[:, 0].repeat(2, 1)[:3], slots)


# ---- the model --------------------------------------------------------------------------------------------------------------------------
LATE_MODEL, BLOCK_AT, BLOCK_K = 9, 20, 8


@pytest.mark.parametrize("subject_embedding,aggregation", VARIANTS)
def test_slot_stream_vs_eval_forward_of_each_timeline(subject_embedding, aggregation):
    from algonauts2025.model import FmriEncoderConfig
    from data_utils.dataloader import SegmentData

    state, data, _ = _variant_case(subject_embedding, aggregation)
    model = FmriEncoderConfig(n_subjects=S, hidden=768, depth=2, heads=4, causal=True, subject_embedding=subject_embedding,
                              feature_aggregation=aggregation).build(FDIMS, V, TOUT)
    model.load_state_dict(state)
    model = model.cuda().eval()
    gpu = {k: v.cuda() for k, v in data.items()}
    with torch.no_grad():
        full = model(SegmentData(data=gpu, segments=[None] * B), pool_outputs=False).float().cpu()
    assert full.shape == (B, V, T)

    def at(starts, k):
        """Steps starts[b] .. starts[b] + k - 1 of timeline b for every slot; None: the slot takes no part (zero features)."""
        batch = {"subject_id": gpu["subject_id"]}
        for name, v in gpu.items():
            if name != "subject_id":
                batch[name] = torch.stack([torch.zeros_like(v[b, ..., :k]) if s is None else v[b, ..., s:s + k] for b, s in enumerate(starts)])
        return batch

    stream = model.stream(B, T, independent=True)
    cols = [[], []]
    call = 0
    while stream.positions[0] < T:
        p0, p1 = stream.positions
        late = call < LATE_MODEL
        k = BLOCK_K if call == BLOCK_AT else 1
        batch = at([p0, None if late else p1], k)
        active = [0] if late else None
        out = stream.push_block(batch, active)[:, :, :] if k > 1 else stream.push(batch, active)[:, :, None]
        assert out.shape == (B, V, k) and out.dtype == torch.float32
        assert stream.positions == [p0 + k, p1 if late else p1 + k]
        cols[0].append(out[0])
        if late:
            assert bool((out[1] == 0).all()), "the row of an inactive slot is not zero"
        else:
            cols[1].append(out[1])
        call += 1
    n1 = T - LATE_MODEL
    assert call == T - BLOCK_K + 1 and stream.positions == [T, n1]
    got = [torch.cat(c, dim=1).cpu() for c in cols]
    errs = {"slot 0": _rel(got[0], full[0]), "slot 1 (late)": _rel(got[1], full[1, :, :n1])}

    # the same late start through the uniform stream: 9 calls of zero features for timeline 1, then its steps at the global call index
    uniform = model.stream(B, T)
    first = []
    for call in range(BLOCK_AT):
        out = uniform.push(at([call, None if call < LATE_MODEL else call - LATE_MODEL], 1))
        if call >= LATE_MODEL:
            first.append(out[1])
    first = torch.stack(first, dim=1).cpu()
    power = _rel(first, full[1, :, : first.shape[1]])
    head = _rel(got[1][:, : first.shape[1]], full[1, :, : first.shape[1]])
    print(f"subject_embedding={subject_embedding} {aggregation}: slots vs eval forward {errs}; the late timeline's first {first.shape[1]} "
          f"outputs: slots {head:.2e}, uniform stream at the global call index {power:.2e}")
    assert max(errs.values()) < BOUND and head < BOUND
    assert power > 10 * BOUND
    stream.reset([0])
    assert stream.positions == [0, n1]
    with pytest.raises(ValueError, match=rf"slot 1: {n1} steps seen \+ {BLOCK_K + 2} would run past max_len={T}"):
        stream.push_block(at([0, 0], BLOCK_K + 2))
