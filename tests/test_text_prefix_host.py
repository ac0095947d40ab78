"""CPU (no GPU): the host side of `LLAMA3p2(share_prefixes=True)` -- how contexts are grouped into runs of nested token rows
(`prefix_groups`), that a member's pooling window addresses its group's longest row unchanged, and that the new C entry points are
declared, bound and hidden from the plugin's uids."""

import ctypes
import re
from pathlib import Path

import torch

from data_utils.features.text import LLAMA3p2, prefix_groups, word_pool_windows

ROOT = Path(__file__).resolve().parent.parent
PAD = 7


def _nested(n, first=10):
    """contexts of one timeline below the cap: row i is row i - 1 plus one token"""
    return [list(range(first, first + i + 1)) for i in range(n)]


def _check_cover(rows, groups):
    """every input in exactly one group, in input order; every member a prefix of its group's longest row"""
    assert [m for _, members in groups for m in members] == list(range(len(rows)))
    for longest, members in groups:
        assert len(longest) == max(len(rows[m]) for m in members)
        for m in members:
            assert longest[:len(rows[m])] == list(rows[m])


def test_a_nested_run_is_one_group():
    rows = _nested(12)
    groups = prefix_groups(rows)
    assert groups == [(rows[-1], list(range(12)))]
    _check_cover(rows, groups)


def test_one_different_token_or_a_new_timeline_breaks_the_group():
    rows = _nested(5)
    changed = rows[4][:]
    changed[2] = 999                                   # same length as the longest, one token differs
    other = _nested(3, first=500)                      # a second timeline starts over with one word
    rows = rows + [changed] + other
    groups = prefix_groups(rows)
    assert [members for _, members in groups] == [[0, 1, 2, 3, 4], [5], [6, 7, 8]]
    assert groups[1][0] == changed and groups[2][0] == other[-1]
    _check_cover(rows, groups)


def test_a_sliding_window_breaks_it_at_every_word():
    cap = 5
    stream = list(range(100, 120))
    rows = [stream[max(0, i + 1 - cap):i + 1] for i in range(len(stream))]   # the context rule with a cap of 5 tokens
    groups = prefix_groups(rows)
    assert [members for _, members in groups] == [list(range(cap))] + [[i] for i in range(cap, len(stream))]
    _check_cover(rows, groups)


def test_repeats_shorter_and_empty_contexts_join():
    rows = [[10], [10, 11], [10, 11], [10, 11, 12], [10], [], [10, 11, 12, 13], [], [20]]
    groups = prefix_groups(rows)
    assert groups == [([10, 11, 12, 13], [0, 1, 2, 3, 4, 5, 6, 7]), ([20], [8])]
    _check_cover(rows, groups)
    # an empty context first: it opens a group that the next context extends
    assert prefix_groups([[], [5, 6], []]) == [([5, 6], [0, 1, 2])]
    assert prefix_groups([[], []]) == [([], [0, 1])]
    assert prefix_groups([]) == []
    # tensors and tuples are rows too
    assert prefix_groups([torch.tensor([3, 4]), (3, 4, 5)]) == [([3, 4, 5], [0, 1])]


def test_window_positions_are_those_of_the_per_word_rows():
    """word_pool_windows on the padded per-word batch gives (start, len) per word; the shared route pools the same positions of the
    group's longest row.  Covers a word longer than its context and a zero-length word (both take the whole context)."""
    rows = _nested(6) + [[], [10, 11]]
    words = ["a", "toolongword", "abc", "", "ab", "abcdef", "x", "abc"]
    T = max(len(r) for r in rows)
    ids = torch.full((len(rows), T), PAD, dtype=torch.long)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = torch.tensor(r, dtype=torch.long)
    start, length = word_pool_windows(ids, words, PAD)
    assert start.tolist() == [0, 0, 0, 0, 3, 0, 0, 0] and length.tolist() == [1, 2, 3, 4, 2, 6, 0, 2]
    (longest, members), = prefix_groups([ids[i, :int(start[i] + length[i])].tolist() for i in range(len(rows))])
    assert members == list(range(len(rows))) and longest == rows[5]
    for m in members:
        s, n = int(start[m]), int(length[m])
        assert s + n == len(rows[m]) <= len(longest)
        assert longest[s:s + n] == ids[m, s:s + n].tolist()   # the same tokens at the same positions


def test_header_declares_the_entry_points_and_the_binding_carries_them():
    from tribe_hip import _lib

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tribe_hip.h").read_text(), flags=re.S)
    for name in ("tribe_window_mean_fwd", "tribe_llama_windows_workspace_bytes", "tribe_llama_windows_fwd"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/tribe_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    assert re.search(r"#define TRIBE_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5
    vp, i64, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t
    desc = ctypes.POINTER(_lib.LlamaDesc)
    assert _lib.SIGNATURES["tribe_window_mean_fwd"] == (ctypes.c_int, [vp, i64, i64, i64, vp, vp, vp, i64, vp, i64, vp])
    assert _lib.SIGNATURES["tribe_llama_windows_workspace_bytes"] == (sz, [desc])
    assert _lib.SIGNATURES["tribe_llama_windows_fwd"] == (ctypes.c_int, [desc, vp, vp, vp, i64, vp, vp, sz, vp])
    handle = _lib.lib()
    assert handle.tribe_version() == 5
    # argument errors come back before any launch
    assert handle.tribe_window_mean_fwd(None, 1, 1, 4, None, None, None, 1, None, 4, None) < 0
    assert handle.tribe_llama_windows_fwd(None, None, None, None, 1, None, None, 0, None) < 0
    assert handle.tribe_llama_windows_workspace_bytes(None) == 0


def test_share_prefixes_is_a_schedule_not_a_result():
    feat = LLAMA3p2(share_prefixes=True, device="cpu")
    assert feat.share_prefixes is True and LLAMA3p2(device="cpu").share_prefixes is False
    assert {"device", "share_prefixes"} <= set(LLAMA3p2._exclude_from_cls_uid())
    assert {"device", "share_prefixes", "layers", "layer_aggregation"} <= set(feat._exclude_from_cache_uid())
    assert LLAMA3p2(device="cpu")._exclude_from_cache_uid() == ["device", "layers", "layer_aggregation"]   # the reference's list, unset
