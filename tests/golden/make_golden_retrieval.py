"""Golden vectors for the retrieval metrics (g14) by EXECUTING the reference's `Rank` / `TopkAcc`.

Run in the build container only (needs the reference checkout, which never travels to the GPU box):

    python tests/golden/make_golden_retrieval.py

modeling_utils/metrics/metrics.py of the reference imports `torchmetrics` (absent here).  It is loaded by file path after an
inert stub is registered: `Metric` is an nn.Module whose `add_state` sets the attribute, `regression.PearsonCorrCoef` a
placeholder base class (OnlinePearsonCorr is not executed).  Everything Rank / TopkAcc compute is the reference's own code.

Only data is written: tests/golden/g14_retrieval.npz.  Labels are stored as integer codes; the tests pass them as `str(code)`,
which is what the reference's `list.index` lookup sees here too.
"""

from __future__ import annotations

import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch
from torch import nn

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")

REDUCTIONS = ("mean", "median", "std")
TOPKS = (1, 5)


def load_reference_metrics() -> types.ModuleType:
    tm = types.ModuleType("torchmetrics")
    reg = types.ModuleType("torchmetrics.regression")

    class Metric(nn.Module):
        def add_state(self, name, default, dist_reduce_fx=None):
            setattr(self, name, default)

    class PearsonCorrCoef(Metric):   # placeholder base of OnlinePearsonCorr, never instantiated here
        pass

    tm.Metric, reg.PearsonCorrCoef, tm.regression = Metric, PearsonCorrCoef, reg
    sys.modules["torchmetrics"], sys.modules["torchmetrics.regression"] = tm, reg
    path = REF / "modeling_utils/modeling_utils/metrics/metrics.py"
    spec = importlib.util.spec_from_file_location("ref_retrieval_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _labels(codes) -> list[str] | None:
    return None if codes is None else [str(int(c)) for c in codes]


def main() -> None:
    ref = load_reference_metrics()
    g = torch.Generator().manual_seed(14)
    out: dict[str, np.ndarray] = {}

    def rnd(*shape):
        return torch.randn(*shape, generator=g)

    cases: dict[str, dict] = {}

    # diagonal from time-means of a [16, 64, 8] pair; target rows 3 and 11 duplicated into 5 and 12 (exact ties after any mean)
    pred = rnd(16, 64, 8)
    target = 0.4 * pred + rnd(16, 64, 8)
    target[5], target[12] = target[3], target[11]
    out["bvt__pred"], out["bvt__target"] = pred.numpy(), target.numpy()
    cases["bvt"] = {"updates": [(pred.mean(-1), target.mean(-1), None, None)], "relative": False}

    # plain [N, V]
    x = rnd(24, 48)
    cases["plain"] = {"updates": [(x, 0.3 * x + rnd(24, 48), None, None)], "relative": False}

    # labelled gallery, M != N, repeated labels (the true row is the first occurrence)
    ylab = np.array([0, 1, 2, 3, 4, 5, 2, 6, 7, 3, 8, 9, 10, 11, 1, 12, 13, 14, 15, 16, 17, 4, 18, 19, 20, 21, 22, 23, 24, 2])
    y = rnd(30, 32)
    xlab = np.array([2, 3, 0, 4, 1, 24, 17, 2, 9, 12])
    first = [int(np.flatnonzero(ylab == c)[0]) for c in xlab]
    x = 0.5 * y[first] + rnd(10, 32)
    cases["labelled"] = {"updates": [(x, y, xlab, ylab)], "relative": False}

    # duplicated gallery rows (exact ties): rows 2, 7 and 9 equal, 4 and 10 equal
    x = rnd(12, 40)
    y = 0.5 * x + rnd(12, 40)
    y[7], y[9], y[10] = y[2], y[2], y[4]
    cases["ties"] = {"updates": [(x, y, None, None)], "relative": False}

    # a NaN query row (rank N // 2)
    x = rnd(10, 32)
    y = 0.5 * x + rnd(10, 32)
    x[4] = float("nan")
    cases["nanrow"] = {"updates": [(x, y, None, None)], "relative": False}

    # a zero-norm target row
    x = rnd(10, 32)
    y = 0.5 * x + rnd(10, 32)
    y[3] = 0.0
    cases["zeronorm"] = {"updates": [(x, y, None, None)], "relative": False}

    # relative ranks, labelled (divides by M)
    y = rnd(20, 24)
    ylab2 = np.arange(20)
    xlab2 = np.array([3, 7, 0, 19, 12, 5, 5, 8])
    x = 0.4 * y[xlab2] + rnd(8, 24)
    cases["relative"] = {"updates": [(x, y, xlab2, ylab2)], "relative": True}

    # three successive updates of sizes 16 / 7 / 16 (the 7-row call has a NaN query: rank 7 // 2)
    ups = []
    for n in (16, 7, 16):
        x = rnd(n, 36)
        y = 0.35 * x + rnd(n, 36)
        if n == 7:
            x[2] = float("nan")
        ups.append((x, y, None, None))
    cases["seq"] = {"updates": ups, "relative": False}

    names = list(cases)
    out["cases"] = np.array(names)
    for name, case in cases.items():
        rel = case["relative"]
        out[f"{name}__n_updates"] = np.array(len(case["updates"]))
        out[f"{name}__relative"] = np.array(rel)
        for i, (x, y, xl, yl) in enumerate(case["updates"]):
            out[f"{name}__x{i}"], out[f"{name}__y{i}"] = x.numpy(), y.numpy()
            if xl is not None:
                out[f"{name}__xl{i}"], out[f"{name}__yl{i}"] = np.asarray(xl), np.asarray(yl)
        results = []
        ranks = None
        for red in REDUCTIONS:
            m = ref.Rank(reduction=red, relative=rel)
            for x, y, xl, yl in case["updates"]:
                m.update(x, y, _labels(xl), _labels(yl))
            results.append(float(m.compute()))
            ranks = m.ranks.clone() if ranks is None else ranks
            assert torch.equal(ranks, m.ranks)
        if not rel:   # TopkAcc has no relative form
            for k in TOPKS:
                m = ref.TopkAcc(topk=k)
                for x, y, xl, yl in case["updates"]:
                    m.update(x, y, _labels(xl), _labels(yl))
                assert torch.equal(m.ranks, ranks)
                results.append(float(m.compute()))
        out[f"{name}__ranks"] = ranks.numpy().astype(np.float32)
        out[f"{name}__compute"] = np.array(results, dtype=np.float64)   # mean, median, std[, top1, top5]

    # _compute_sim for the four norm kinds (N != M, one zero row on each side)
    x, y = rnd(6, 20), rnd(9, 20)
    x[1], y[4] = 0.0, 0.0
    out["sim__xin"], out["sim__yin"] = x.numpy(), y.numpy()
    for kind in (None, "x", "y", "xy"):
        out[f"sim__{kind}"] = ref.Rank._compute_sim(x, y, norm_kind=kind).numpy()

    np.savez_compressed(HERE / "g14_retrieval.npz", **out)
    print({k: v for k, v in out.items() if k.endswith("__ranks") or k.endswith("__compute")})


if __name__ == "__main__":
    main()
