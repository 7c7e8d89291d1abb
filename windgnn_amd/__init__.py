"""windgnn_amd: MI355X-native (gfx950 HIP) implementation of WindGNN's GCN+GRU hot path behind
the reference's own nn.Module API.  See DESIGN.md / INTEGRATION.md."""
from .evaluate import Evaluator  # noqa: F401
from .modules import GCN_GRU, GraphConvLayer  # noqa: F401
from .streaming import StreamingForecaster  # noqa: F401
from .ensemble import Ensemble, EnsembleForecast, PerMember  # noqa: F401
from .transfer import adopt_convs  # noqa: F401

__all__ = ["Ensemble", "EnsembleForecast", "Evaluator", "GCN_GRU", "GraphConvLayer", "PerMember", "StreamingForecaster", "adopt_convs"]
