"""CPU (no GPU): the GEMM launchers decide what they decided before they were rebuilt around one resolve step (csrc/gemm_plan.cpp).
tests/golden/gemm_plan.npz holds, for a few thousand descriptors, the return code, the error text and every integer of the launch the OLD
tribe_gemm_bf16 / tribe_gemm_fp8 would have made; it was recorded from the commit before the rebuild (tests/golden/make_golden_gemm_plan.py
keeps the recording patch) and is never regenerated from the code under test.  Here every case is replayed through tribe_debug_gemm_plan
-- made-up addresses, nothing is launched -- and must match in every field; and the table must cover the dispatch, so that a thin one
cannot pass."""

import ctypes as C
from functools import lru_cache
from pathlib import Path

import numpy as np

FIXTURE = Path(__file__).resolve().parent / "golden" / "gemm_plan.npz"
KIND_SMALL, KIND_BIG, KIND_RING, KIND_BIG4W = range(4)
N_PAIRS = 12   # TRIBE_GEMM_PAIRS (csrc/gemm_plan.h)

# every TRIBE_REQUIRE of the two entry points, by a piece of its text that no other has
BF16_MESSAGES = [
    "null descriptor", "M, N, K must be positive (got 0 128 64)", "K=96 must be a multiple of 64 (zero-pad K)", "batch counts must be positive", "null operand",
    "lda/ldb/batch strides must be multiples of 8 elements (16-byte rows)", "A/B must be 16-byte aligned", "leading dimension too small",
    "SWIGLU needs an even N and no residual / row adds", "c_dtype must be f32 or bf16", "bias_mode set without bias", "rowadd needs a positive period",
    "gadd needs index and divisor", "gather flags set without gather1", "GELU_BWD needs the saved pre-activation in aux",
    "MUL_AUX needs aux laid out like C (ld_aux == ldc)", "EXP2 / MUL_AUX take a row bias only", "aux is supported for un-batched GEMMs (and for MUL_AUX)",
    "sBias0 belongs to a row bias", "c_bf16 / row_sumsq / row_scale need an un-batched launch with plain operators",
    "c_bf16 / row_sumsq / row_scale need 16-byte aligned operands", "c_bf16 / row_sumsq accompany an f32 C", "bad c_bf16",
    "c_bf16 / row_sumsq / row_scale need N (320) to be a multiple of the tile width 192", "ld_row_sumsq must cover N / 48 slots (tribe_gemm_sumsq_slots)",
    "ld_row_sumsq must cover N / 64 slots (tribe_gemm_sumsq_slots)",
    "trans_ab takes At [K, M] and Bt [K, N] with M and N multiples of 8 and lda >= M, ldb >= N",
    "trans_ab supports the plain epilogue operators and no operand gather", "grid too large", "stream_k takes a plain un-batched f32 product",
    "stream_k needs a 16-byte aligned workspace of 134217728 bytes (tribe_gemm_stream_k_workspace_bytes)",
    "this launch is split over K: stream_k_ws must hold 12582912 bytes (tribe_gemm_stream_k_workspace_bytes)",
]
FP8_MESSAGES = [
    "null descriptor", "M, N, K must be positive (got 128 128 0)", "K=64 must be a multiple of 128 (zero-pad K)", "batch counts must be positive", "null operand",
    "lda/ldb/batch strides must be multiples of 16 elements (16-byte rows)", "A/B must be 16-byte aligned", "leading dimension too small",
    "SWIGLU / GLU need an even N and no residual / row adds", "c_dtype must be f32 or bf16", "bias_mode set without bias", "rowadd needs a positive period",
    "gadd needs index and divisor", "gather flags set without gather1", "the training-only epilogues (aux, GELU_BWD) are bf16-only", "grid too large",
]


@lru_cache(maxsize=None)
def _fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _replay():
    """(expected row, got row, expected text, got text) of every case."""
    from tribe_hip import _lib

    f = _fixture()
    handle = _lib.lib()
    fields = [str(n) for n in f["fields"]]
    n_out = len(f["out_fields"])
    for i in range(len(f["desc"])):
        got = (C.c_int64 * n_out)()
        if f["null"][i]:
            rc = handle.tribe_debug_gemm_plan(None, int(f["fp8"][i]), got, n_out)
        else:
            d = _lib.GemmDesc()
            for name, v in zip(fields, f["desc"][i].tolist()):
                setattr(d, name, v)
            d.alpha = float(f["alpha"][i])
            rc = handle.tribe_debug_gemm_plan(C.byref(d), int(f["fp8"][i]), got, n_out)
        text = handle.tribe_last_error().decode() if rc != 0 else ""
        yield i, f["out"][i].tolist(), [rc] + list(got)[1:], str(f["messages"][f["message_of"][i]]), text


def test_every_recorded_launch_is_resolved_as_before():
    f = _fixture()
    assert "do not regenerate" in str(f["note"])
    names = [str(n) for n in f["out_fields"]]
    bad = []
    for i, want, got, want_text, got_text in _replay():
        if want != got or want_text != got_text:
            diff = {n: (w, g) for n, w, g in zip(names, want, got) if w != g}
            bad.append(f"case {i} (fp8={int(f['fp8'][i])}): {diff} text {want_text!r} -> {got_text!r}")
    assert not bad, f"{len(bad)} of {len(f['desc'])} cases changed (recorded, now):\n" + "\n".join(bad[:20])


def test_workspace_query_reads_the_plan_of_the_launch():
    """tribe_gemm_stream_k_workspace_bytes answers what the launch will demand -- and 0 (not split) for a stream_k request whose
    operators the launch refuses, where it used to name a size for a launch that could not happen."""
    from tribe_hip import _lib

    f = _fixture()
    handle = _lib.lib()
    fields = [str(n) for n in f["fields"]]
    ws_need = f["out"][:, [str(n) for n in f["out_fields"]].index("ws_need")]
    refused_text = "tribe_gemm_bf16: stream_k takes a plain un-batched f32 product"
    asked = refused = 0
    for i in range(len(f["desc"])):
        text = str(f["messages"][f["message_of"][i]])
        if f["fp8"][i] or f["null"][i] or not (f["out"][i, 0] == 0 or text == refused_text):
            continue
        d = _lib.GemmDesc()
        for name, v in zip(fields, f["desc"][i].tolist()):
            setattr(d, name, v)
        d.alpha = float(f["alpha"][i])
        got = handle.tribe_gemm_stream_k_workspace_bytes(C.byref(d))
        assert got == (0 if text == refused_text else ws_need[i]), (i, got)
        asked += got > 0
        refused += text == refused_text
    assert asked > 20 and refused > 5


def test_fixture_covers_the_dispatch():
    f = _fixture()
    col = {str(n): f["out"][:, j] for j, n in enumerate(f["out_fields"])}
    field = {str(n): f["desc"][:, j] for j, n in enumerate(f["fields"])}
    fp8, ok = f["fp8"] == 1, col["rc"] == 0
    bf = ~fp8
    assert len(f["desc"]) >= 2000
    texts = {False: set(), True: set()}
    for i in np.nonzero(~ok)[0]:
        texts[bool(fp8[i])].add(str(f["messages"][f["message_of"][i]]))
    for is_fp8, wanted, who in ((False, BF16_MESSAGES, "tribe_gemm_bf16: "), (True, FP8_MESSAGES, "tribe_gemm_fp8: ")):
        missing = [m for m in wanted if who + m not in texts[is_fp8]]
        assert not missing, f"{who}no case fails with {missing}"
    # every kind, the 8-wave kind with both tile widths; every kernel symbol, the fallbacks of a role kernel to GENERIC included
    kinds = {(int(k), int(b)) for k, b in zip(col["kind"][ok & bf], col["bn"][ok & bf])}
    assert kinds >= {(KIND_SMALL, 128), (KIND_RING, 128), (KIND_BIG, 256), (KIND_BIG, 192), (KIND_BIG4W, 256)}
    assert set(col["pair"][ok & bf].tolist()) == set(range(N_PAIRS)) and set(col["pair"][ok & fp8].tolist()) == {0, 1, 2, 3}
    role_named = np.isin(field["role"], [2, 5, 6, 7]) & ok & bf & (col["kind"] == KIND_BIG) & (field["trans_ab"] == 0)
    for role, dtype_pair in ((2, 0), (5, 1), (6, 0), (7, 1)):   # QKV, out-proj, FF1, FF2 -> the GENERIC symbol of the role's dtype
        assert np.any(role_named & (field["role"] == role) & (col["pair"] == dtype_pair) & (col["epilogue_path"] == 0))
    assert set(col["epilogue_path"][ok & bf].tolist()) == {0, 1, 2}
    # split-K with 2 and 8 shares, and a request that is declined; stream-K split and declined -- with the remainders above half a round
    nt_request = ok & bf & (field["stream_k"] == 1) & (field["trans_ab"] == 0)
    assert {2, 8} <= set(col["splits"][nt_request].tolist()) and np.any(nt_request & (col["splits"] == 1) & (col["kind"] == KIND_RING))
    assert np.all(col["ws_need"][nt_request & (col["splits"] > 1)] > 0)
    tn_request = ok & bf & (field["stream_k"] == 1) & (field["trans_ab"] == 1)
    split = tn_request & (col["reduce_grid_x"] > 0)
    assert np.any(split) and np.all(col["sk_second_parts"][split] >= 0) and np.any(col["sk_second_parts"][split] > 0)
    declined = {(int(t), int(k) // 64) for t, k in zip((col["tiles_m"] * col["tiles_n"])[tn_request & ~split], field["K"][tn_request & ~split])}
    assert {(144, 256), (432, 256)} <= declined   # tests/test_abi_and_host.py::test_stream_k_schedule_covers_every_k_step_once
    assert {(576, 256), (64, 256)} <= {(int(t), int(k) // 64) for t, k in zip((col["tiles_m"] * col["tiles_n"])[split], field["K"][split])}
