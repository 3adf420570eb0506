"""blueice_amd: the binned-likelihood hot path of blueice, MI355X-native.

Top-level names follow the reference's `blueice/__init__.py` (likelihood, model, source, exceptions).
"""
from .exceptions import *  # noqa: F401,F403
from .model import Model  # noqa: F401
from .priors import GaussianPrior  # noqa: F401
from .source import Source, HistogramPdfSource, DensityEstimatingSource, MonteCarloSource  # noqa: F401
from .likelihood import (LogLikelihoodBase, BinnedLogLikelihood, UnbinnedLogLikelihood,  # noqa: F401
                         LogLikelihoodSum, LogLikelihoodReParam, LogAncillaryLikelihood, toy_seed)
from .grid import grid_scan, GridResult  # noqa: F401
from .coarse import CoarseBinning  # noqa: F401
from .source_wise import SourceWiseBinnedLogLikelihood  # noqa: F401
from .source_wise_unbinned import (SourceWiseUnbinnedLogLikelihood, sourcewise_event_toys, sourcewise_event_toys_points,  # noqa: F401
                                   sourcewise_simulated_events)

__version__ = '0.1.0'
