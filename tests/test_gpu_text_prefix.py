"""GPU: one Llama forward per run of nested word contexts -- `ops.window_mean` (tribe_window_mean_fwd) per element against float64,
`HipLlamaModel.forward_windows` (tribe_llama_windows_fwd) against the fp32 `transformers` model run once per word on that word's own
context, and `LLAMA3p2(share_prefixes=True)` end to end against the per-word route's oracle."""

import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import extractors_ref  # noqa: E402

PAD = 7


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the window-mean kernel
# ---------------------------------------------------------------------------------------------------------------------------
def _window_list(B, T, W):
    """(row, start, len) x W.  The 37-window list holds: length 1, length T, a start at 0, an end at T, two overlapping windows on one
    row, two equal windows, an empty one, windows that need clamping (start < 0, end > T, start > T, negative length) and rows outside
    [0, B) -- then random ones up to W."""
    if W == 1:
        return [(B - 1, 1, min(3, T - 1))]
    wins = [(0, T // 2, 1), (B - 1, 0, T), (0, 0, 2), (1, T - 3, 3), (1, 1, 4), (1, 3, 4), (0, 2, 3), (0, 2, 3), (1, 4, 0),
            (0, -2, 5), (1, T - 2, 9), (0, T + 3, 2), (1, 2, -1), (B, 0, 2), (-1, 1, 2), (0, T, 1), (0, T - 1, 1)]
    g = torch.Generator().manual_seed(B * 1000 + T)
    while len(wins) < W:
        s = int(torch.randint(0, T, (1,), generator=g))
        wins.append((int(torch.randint(0, B, (1,), generator=g)), s, int(torch.randint(1, min(T - s, 40) + 1, (1,), generator=g))))
    return wins


@functools.lru_cache(maxsize=None)
def _window_case(B, T, dim, W):
    """x, the window list and, per window, the float64 mean, the clamped row count n and mean_t |x| -- computed once per case"""
    g = torch.Generator().manual_seed(dim + W)
    x = torch.randn(B * T, dim, generator=g) * 3 + 0.5
    wins = _window_list(B, T, W)
    x64 = x.double().view(B, T, dim)
    want, count, scale = torch.zeros(W, dim, dtype=torch.float64), [], torch.zeros(W, dim, dtype=torch.float64)
    for w, (b, s, n) in enumerate(wins):
        s = min(max(s, 0), T)
        n = min(n, T - s) if 0 <= b < B else 0
        count.append(max(n, 0))
        if n > 0:
            want[w] = x64[b, s:s + n].mean(0)
            scale[w] = x64[b, s:s + n].abs().mean(0)
    return x, wins, want, count, scale


@pytest.mark.parametrize("W", [1, 37])
@pytest.mark.parametrize("B,T,dim", [(3, 7, 64), (2, 300, 1408), (2, 50, 30)], ids=["small", "column-blocks", "scalar"])
def test_window_mean_per_element_vs_float64(B, T, dim, W):
    """|got - want| <= (n + 1) * 2^-24 * mean_t |x[t, c]| for a window of n rows: the float32 bound on a sum of n terms in any order
    ((n - 1) roundings, each at most 2^-24 of the running sum <= sum |x|) plus one division."""
    from tribe_hip import ops

    x, wins, want, count, scale = _window_case(B, T, dim, W)
    row, start, length = (torch.tensor(v, dtype=torch.int64).cuda() for v in zip(*wins))
    xg = x.cuda()
    got = ops.window_mean(xg, B, T, row, start, length)
    assert got.shape == (W, dim) and got.dtype == torch.float32
    again = ops.window_mean(xg, B, T, row, start, length)
    got, again = got.cpu(), again.cpu()
    assert torch.equal(got, again), "two launches on the same input differ"
    assert W == 1 or 0 in count
    for w, n in enumerate(count):
        if n == 0:
            assert bool((got[w] == 0).all()), f"window {w} {wins[w]} is empty: must be exactly zero"
            continue
        err = (got[w].double() - want[w]).abs()
        bound = (n + 1) * 2.0 ** -24 * scale[w]
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"window {w} {wins[w]}: n={n} max err / bound = {worst:.3f}")
        assert bool((err <= bound).all()), f"window {w} {wins[w]}: max err / bound = {worst:.3f}"
    if W > 1:
        assert torch.equal(got[6], got[7])   # the two equal windows


def test_window_mean_refuses_bad_arguments():
    from tribe_hip import ops

    x = torch.zeros(6, 8, device="cuda")
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ops.window_mean(x, 2, 4, one, one, one)               # x does not hold B * T rows
    with pytest.raises(ValueError):
        ops.window_mean(x, 2, 3, one, one, one[:0])           # window arrays of different lengths


# ---------------------------------------------------------------------------------------------------------------------------
# 2. / 3. / 5. the forward with a window list
# ---------------------------------------------------------------------------------------------------------------------------
def _llama(layers=3, hidden=256, heads=4, kv=2, head_dim=64, inter=512, vocab=300):
    from transformers import LlamaConfig, LlamaModel

    cfg = LlamaConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers,
                      num_attention_heads=heads, num_key_value_heads=kv, head_dim=head_dim, max_position_embeddings=16384,
                      rms_norm_eps=1e-5, tie_word_embeddings=True,
                      rope_parameters={"rope_type": "llama3", "rope_theta": 500000.0, "factor": 32.0, "low_freq_factor": 1.0,
                                       "high_freq_factor": 4.0, "original_max_position_embeddings": 8192})
    torch.manual_seed(0)
    return cfg, LlamaModel(cfg).eval()


@functools.lru_cache(maxsize=None)
def _models(shape):
    """(config, fp32 transformers model, HipLlamaModel) -- 'wide': the real Llama-3.2-3B widths on 2 layers"""
    from data_utils.features.text import HipLlamaModel

    cfg, hf = _llama() if shape == "tiny" else _llama(layers=2, hidden=3072, heads=24, kv=8, head_dim=128, inter=8192, vocab=512)
    return cfg, hf, HipLlamaModel(cfg, hf.state_dict())


def _per_word_reference(hf, row, ends, words, T):
    """What the reference computes for each word: the model over the word's OWN context (row[:end]), right padded to T, then the mean of
    the last len(word) real positions.  One oracle call per word.  Returns the per-word [n_states, dim] arrays and the per-word rows."""
    from data_utils.features.text import word_pool_windows

    want, ids = [], torch.full((len(words), T), PAD, dtype=torch.long)
    for j, (end, word) in enumerate(zip(ends, words)):
        ids[j, :end] = row[:end]
        want.append(extractors_ref.llama_word_states(hf, ids[j:j + 1], (ids[j:j + 1] != PAD).long(), [word], PAD)[0])
    start, length = word_pool_windows(ids, words, PAD)
    return want, ids, start, length


def _check_states(got, want, what):
    """the project's bounds for pooled Llama states (tests/test_gpu_extractors.py): bf16 embedding table, bf16 GEMM operands"""
    worst = 0.0
    for j, w in enumerate(want):
        assert got[:, j].shape == w.shape
        np.testing.assert_allclose(got[0, j], w[0], rtol=0, atol=4e-3 * np.abs(w[0]).max() + 1e-6)
        err = _rel(got[:, j], w)
        worst = max(worst, err)
        assert err < 1.5e-2, f"{what} word {j}: relative L2 error {err:.2e}"
    print(f"{what}: largest relative L2 error vs transformers {worst:.3e}")


@pytest.mark.parametrize("shape", ["tiny", "wide"])
def test_forward_windows_vs_transformers_per_word(shape):
    """Row 0: 45 tokens, six words whose windows end across the row; row 1: 3 tokens and a word longer than its context."""
    cfg, hf, model = _models(shape)
    g = torch.Generator().manual_seed(11)
    T = 45
    ids = torch.randint(8, cfg.vocab_size, (2, T), generator=g)
    ids[1, 3:] = PAD
    ends0, words0 = [5, 12, 20, 31, 40, 45], ["abc", "a", "sevench", "hello", "extraordinarily", "word"]
    want0, _, start0, len0 = _per_word_reference(hf, ids[0], ends0, words0, T)
    want1, _, start1, len1 = _per_word_reference(hf, ids[1], [3], ["toolongword"], T)
    assert (start0 + len0).tolist() == ends0 and start1.tolist() == [0] and len1.tolist() == [3]
    win_row = torch.tensor([0] * 6 + [1])
    got = model.forward_windows(ids, win_row, torch.cat([start0, start1]), torch.cat([len0, len1]), fp8=False).cpu().numpy()
    assert got.shape == (cfg.num_hidden_layers + 1, 7, cfg.hidden_size)
    _check_states(got, want0 + want1, f"forward_windows[{shape}]")


def test_forward_windows_is_causal_across_attention_tiles():
    """One row of 300 tokens; windows end at 63, 64, 65, 128, 129, 299 and 300: a state pooled from the long row must be the state of
    the prefix run alone, whichever attention tile the position falls into."""
    cfg, hf, model = _models("tiny")
    g = torch.Generator().manual_seed(12)
    T = 300
    row = torch.randint(8, cfg.vocab_size, (T,), generator=g)
    ends, words = [63, 64, 65, 128, 129, 299, 300], ["four", "a", "spanning", "abc", "twelve_chars", "hello", "extraordinarily"]
    want, prefix_ids, start, length = _per_word_reference(hf, row, ends, words, T)
    assert (start + length).tolist() == ends
    shared = model.forward_windows(row[None], torch.zeros(len(ends), dtype=torch.int64), start, length, fp8=False).cpu().numpy()
    _check_states(shared, want, "forward_windows[300 tokens]")
    per_word = model.forward_pooled(prefix_ids, start, length, fp8=False).cpu().numpy()
    _check_states(per_word, want, "forward_pooled[per prefix]")
    dist = max(_rel(shared[:, j], per_word[:, j]) for j in range(len(ends)))
    print(f"shared vs per-word route: largest relative L2 distance {dist:.3e}")   # recorded, not a gate


def test_forward_windows_takes_the_fp8_route_of_forward_pooled():
    """The same forward (same ids, same shape), pooled by the two kernels: window w of forward_windows against the one window per row of
    forward_pooled, on the bf16 and on the e4m3 route.  Both average the same n <= 5 float32 rows, each within (n + 1) * 2^-24 *
    mean |x| of the exact mean per element, i.e. within ~1e-6 of each other relative to the vector's norm; 1e-4 leaves room for
    cancellation in the mean and is far below any difference in what is pooled (O(1))."""
    cfg, hf, model = _models("wide")
    g = torch.Generator().manual_seed(13)
    ids = torch.randint(8, cfg.vocab_size, (2, 45), generator=g)
    ids[1, 3:] = PAD
    start, length = torch.tensor([40, 0]), torch.tensor([5, 3])
    rows = torch.tensor([0, 1])
    with pytest.raises(ValueError):
        model.forward_windows(ids, rows, start, length, fp8=True)    # before calibration, as forward_pooled
    try:
        bf16 = model.forward_windows(ids, rows, start, length).cpu().numpy()
        assert _rel(bf16, model.forward_pooled(ids, start, length).cpu().numpy()) < 1e-4
        model.enable_fp8(ids)
        fp8 = model.forward_windows(ids, rows, start, length).cpu().numpy()          # fp8 by default once enabled
        assert _rel(fp8, model.forward_pooled(ids, start, length).cpu().numpy()) < 1e-4
        assert not np.array_equal(fp8, bf16)
        assert np.array_equal(model.forward_windows(ids, rows, start, length, fp8=False).cpu().numpy(), bf16)
    finally:
        model.fp8_layers = None   # the model is shared with the other tests of this file


def test_forward_windows_validates_on_the_host_before_any_launch(monkeypatch):
    cfg, hf, model = _models("tiny")

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(model, "_launch", no_launch)
    ids = torch.randint(8, cfg.vocab_size, (2, 10), generator=torch.Generator().manual_seed(1))
    for row, start, length in (([2], [0], [1]), ([-1], [0], [1]), ([0], [8], [3]), ([0], [-1], [2]), ([0], [0], [-1]), ([0, 1], [0], [1]),
                               ([], [], [])):
        with pytest.raises(ValueError):
            model.forward_windows(ids, row, start, length)
    bad = ids.clone()
    bad[0, 0] = cfg.vocab_size
    with pytest.raises(ValueError):
        model.forward_windows(bad, [0], [0], [1])
    with pytest.raises(AssertionError, match="launched"):
        model.forward_windows(ids, [1], [7], [3])    # a window that ends exactly at T is fine


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the plugin
# ---------------------------------------------------------------------------------------------------------------------------
class _Tok:
    """Whitespace 'tokenizer' with the call signature the plugin uses (ids from a fixed table, right padding)."""

    eos_token_id = PAD
    pad_token = "<eos>"

    def __init__(self, vocab):
        self.vocab = vocab

    def __call__(self, texts, add_special_tokens=False, return_tensors="pt", padding=True, truncation=True):
        rows = [[8 + (sum(map(ord, w)) % (self.vocab - 8)) for w in t.split()] for t in texts]
        n = max(len(r) for r in rows)
        ids = torch.full((len(rows), n), self.eos_token_id, dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r)
        return {"input_ids": ids, "attention_mask": (ids != self.eos_token_id).long()}


def _counted(model):
    """wrap forward_windows / forward_pooled of one model instance; returns the log of (name, rows, windows)"""
    calls = []
    fw, fp = model.forward_windows, model.forward_pooled

    def forward_windows(ids, row, start, length, *a, **k):
        calls.append(("windows", tuple(ids.shape), len(row)))
        return fw(ids, row, start, length, *a, **k)

    def forward_pooled(ids, start, length, *a, **k):
        calls.append(("pooled", tuple(ids.shape), len(start)))
        return fp(ids, start, length, *a, **k)

    model.forward_windows, model.forward_pooled = forward_windows, forward_pooled
    return calls


def test_plugin_share_prefixes_end_to_end():
    from data_utils.events import Word
    from data_utils.features.text import HipLlamaModel, LLAMA3p2

    cfg, hf, _ = _models("tiny")
    tok = _Tok(cfg.vocab_size)
    sentence = "the quick brown fox jumps over the lazy dog again and again".split()
    second = "a second timeline starts".split()
    stream = "one two three four five six seven eight nine".split()
    pairs = [(w, " ".join(sentence[:i + 1])) for i, w in enumerate(sentence)]              # a nested 12-word sentence
    pairs += [(w, " ".join(second[:i + 1])) for i, w in enumerate(second)]                 # a second timeline
    pairs += [pairs[-1]]                                                                   # a repeated word (same context)
    pairs += [("orphan", "")]                                                              # an empty context
    pairs += [(w, " ".join(stream[max(0, i - 4):i + 1])) for i, w in enumerate(stream)]    # a 5-word cap: 5 nested, then 4 sliding
    words, contexts = [w for w, _ in pairs], [c for _, c in pairs]
    empty = contexts.index("")
    n_groups = 1 + 1 + 1 + 4    # the sentence; the second timeline with its repeat and the empty context; the run up to the cap; 4 slides

    enc = tok(contexts)
    want = extractors_ref.llama_word_states(hf, enc["input_ids"], enc["attention_mask"], words, PAD)   # NaN for the empty context

    shared = LLAMA3p2(device="cuda", share_prefixes=True, batch_size=4).attach(HipLlamaModel(cfg, hf.state_dict()), tok)
    calls = _counted(shared._model)
    got = list(shared.extract(words, contexts))
    assert calls == [("windows", (4, 12), 12 + 6 + 5 + 1), ("windows", (3, 5), 3)]
    assert len(calls) == math.ceil(n_groups / 4)
    assert len(got) == len(words) and all(g.shape == (cfg.num_hidden_layers + 1, cfg.hidden_size) for g in got)
    worst = max(_rel(g, w) for j, (g, w) in enumerate(zip(got, want)) if j != empty)
    print(f"share_prefixes vs oracle: largest relative L2 error {worst:.3e}")
    assert worst < 3e-2

    default = LLAMA3p2(device="cuda", batch_size=4).attach(HipLlamaModel(cfg, hf.state_dict()), tok)
    default_calls = _counted(default._model)
    base = list(default.extract(words, contexts))
    assert [c[0] for c in default_calls] == ["pooled"] * math.ceil(len(words) / 4)          # the default route is the per-word one
    assert len(base) == len(got)
    assert not base[empty].any() and not got[empty].any()                                  # zeros for the empty context on both routes
    print(f"share_prefixes vs per-word route: largest relative L2 distance "
          f"{max(_rel(g, b) for j, (g, b) in enumerate(zip(got, base)) if j != empty):.3e}")

    # the nested sentence alone: ONE forward over its longest context where the per-word route takes ceil(12 / 4) = 3
    del calls[:]
    alone = list(shared.extract(words[:12], contexts[:12]))
    assert calls == [("windows", (1, 12), 12)]
    assert all(np.array_equal(a, g) or _rel(a, g) < 3e-2 for a, g in zip(alone, got[:12]))

    # through the plugin surface: one array per Word event, in order (the repeated item is served from the item cache)
    events = [Word(start=1.0 + 0.5 * i, duration=0.3, text=w, context=c, timeline="t") for i, (w, c) in enumerate(pairs)]
    served = list(shared._get_data(events))
    assert len(served) == len(events)
    assert all(np.array_equal(s, g) for j, (s, g) in enumerate(zip(served, got)) if j != empty) or \
        max(_rel(s, g) for j, (s, g) in enumerate(zip(served, got)) if j != empty) < 3e-2
