"""Words/s of the Llama text extractor with one forward per word and with one forward per run of nested contexts
(`LLAMA3p2(share_prefixes=True)`), on one MI355X: the real Llama-3.2-3B widths and depth 28, random weights, a synthetic timeline.

The timeline has 2048 words; contexts follow the reference's AddContextToWords rule (the words so far, cut to the last cap + 1 = 1025
words).  So the first 1025 contexts nest -- each is a prefix of the next -- and the remaining 1023 slide: every one drops its first word
and is no prefix of its successor.  Sharing applies to the nested part only; the sliding part still costs one forward per word, and
the two parts are timed separately.  A third input holds contexts of which no two nest, which shows what the grouping costs when it
cannot help.  Times are host clocks around whole `extract` calls (tokenising, grouping, launches, the copy of the pooled states) that
end in a device synchronise; each route runs once after a warm-up on a sample of the same input.

GPU box: python scripts/llama_prefix_bench.py [--words 2048] [--cap 1024] [--out profiles/llama_prefix_bench.txt]"""
import argparse
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "algonauts-2025_amd"))
sys.path.insert(0, str(ROOT / "scripts"))


class WordTokenizer:
    """Whitespace tokenizer with the call signature the plugin uses: a word is one token, every third word two (about the 1.3 tokens
    per word of English under the Llama tokenizer); ids from a hash of the word; right padding with the eos id."""

    eos_token_id = 7
    pad_token = "<eos>"

    def __init__(self, vocab: int):
        self.vocab = vocab

    def _ids(self, word: str) -> list[int]:
        h = int(word[1:])
        first = 8 + (h * 2654435761) % (self.vocab - 8)
        return [first] if h % 3 else [first, 8 + (h * 40503 + 17) % (self.vocab - 8)]

    def __call__(self, texts, add_special_tokens=False, return_tensors="pt", padding=True, truncation=True):
        rows = [[t for w in text.split() for t in self._ids(w)] for text in texts]
        ids = torch.full((len(rows), max(1, max(len(r) for r in rows))), self.eos_token_id, dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r, dtype=torch.long)
        return {"input_ids": ids, "attention_mask": (ids != self.eos_token_id).long()}


def timeline(n_words: int, cap: int, first: int = 0) -> tuple[list[str], list[str]]:
    """words w<k> and their contexts by the AddContextToWords rule (enhancers.py:386-388: the text up to the word, last cap + 1 words)"""
    words = [f"w{first + i}" for i in range(n_words)]
    return words, [" ".join(words[max(0, i - cap):i + 1]) for i in range(n_words)]


def counted(model):
    calls = {"forward_pooled": 0, "forward_windows": 0}
    for name in calls:
        fn = getattr(model, name)

        def wrapper(*a, _fn=fn, _name=name, **k):
            calls[_name] += 1
            return _fn(*a, **k)

        setattr(model, name, wrapper)
    return calls


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--words", type=int, default=2048)
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "llama_prefix_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("llama_prefix_bench: needs a GPU (rates are not measured on a CPU)")

    from data_utils.features.text import LLAMA3p2, prefix_groups
    from extractor_bench import build_llama

    model, vocab = build_llama()
    tok = WordTokenizer(vocab)
    calls = counted(model)
    routes = {name: LLAMA3p2(device="cuda", share_prefixes=shared).attach(model, tok) for name, shared in (("per-word", False), ("shared", True))}
    batch = routes["shared"].batch_size
    lines: list[str] = []

    def say(text: str) -> None:
        print(text, flush=True)
        lines.append(text)

    def run(route: str, words: list[str], contexts: list[str]) -> tuple[float, int, list[np.ndarray]]:
        before = sum(calls.values())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = list(routes[route].extract(words, contexts))
        torch.cuda.synchronize()
        return time.perf_counter() - t0, sum(calls.values()) - before, out

    words, contexts = timeline(args.words, args.cap)
    n_nested = min(args.words, args.cap + 1)
    # no two contexts nest: every context is a 256-word text of its own
    lone = [[f"w{10_000 + 1000 * i + k}" for k in range(256)] for i in range(256)]
    inputs = {
        f"nested part (words 0..{n_nested - 1}, each context a prefix of the next)": (words[:n_nested], contexts[:n_nested]),
        f"sliding part (words {n_nested}..{args.words - 1}, contexts of {args.cap + 1} words, none a prefix of the next)": (words[n_nested:], contexts[n_nested:]),
        "no two contexts nest (256 contexts of 256 words)": ([t[-1] for t in lone], [" ".join(t) for t in lone]),
    }
    say(f"Llama-3.2-3B widths, depth {model.depth}, random weights; {torch.cuda.get_device_name(0)}; batch_size {batch}; "
        f"{args.words}-word timeline, context cap {args.cap} words")
    for title, (w, c) in inputs.items():
        if not w:
            continue
        rows = [r[:int((r != tok.eos_token_id).sum())].tolist() for r in (tok([x])["input_ids"][0] for x in c)]
        groups = prefix_groups(rows)
        say(f"\n{title}: {len(w)} words, {sum(map(len, rows))} context tokens, {len(groups)} group(s)")
        say(f"  forwards by count: per-word ceil({len(w)} / {batch}) = {math.ceil(len(w) / batch)}, shared ceil({len(groups)} / {batch}) = "
            f"{math.ceil(len(groups) / batch)}")
        sample = slice(None, None, max(1, len(w) // 16))
        for route in routes:   # warm-up: code objects, workspaces, rope tables
            run(route, w[sample], c[sample])
        result = {}
        for route in routes:
            dt, n_fwd, out = run(route, w, c)
            result[route] = out
            say(f"  {route:9s}: {dt:8.3f} s  {len(w) / dt:9.1f} words/s  {n_fwd} forward(s)")
        dist = max(float(np.linalg.norm(a.astype(np.float64) - b) / (np.linalg.norm(b.astype(np.float64)) + 1e-30))
                   for a, b in zip(result["shared"], result["per-word"]))
        say(f"  largest relative L2 distance between the two routes' per-word states: {dist:.3e}")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
