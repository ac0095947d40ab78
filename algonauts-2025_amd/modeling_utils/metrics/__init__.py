"""Metric registry (mirror of /root/reference/modeling_utils/modeling_utils/metrics/__init__.py)."""
import typing as tp

import pydantic

from .base import (BaseMetricConfig, GroupedMetric, GroupedMetricConfig, MultidimPearsonCorrCoef,  # noqa: F401
                   MultidimPearsonCorrCoefConfig, OnlinePearsonCorr, TorchMetricConfig)
from .bootstrap import BootstrapPearsonCorrCoef, BootstrapPearsonCorrCoefConfig, BootstrapResult  # noqa: F401
from .metrics import OnlinePearsonCorrConfig, Rank, RankConfig, TopkAcc, TopkAccConfig  # noqa: F401
from .rank_corr import MultidimSpearmanCorrCoef, MultidimSpearmanCorrCoefConfig  # noqa: F401
from .regression import ExplainedVariance, MeanAbsoluteError, MeanSquaredError, R2Score  # noqa: F401

MetricConfig = tp.Annotated[tp.Union[MultidimPearsonCorrCoefConfig, GroupedMetricConfig, OnlinePearsonCorrConfig, RankConfig,
                                     TopkAccConfig, TorchMetricConfig, MultidimSpearmanCorrCoefConfig, BootstrapPearsonCorrCoefConfig],
                            pydantic.Field(discriminator="name")]
