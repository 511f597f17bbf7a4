"""Per-model explainers (mirror of the `Explain*` classes of models/gridTDmodel.py / models/aoamodel.py / models/adaptiveattention.py)."""
from .adaatt import AdaAttEngine, ExplainAdaptiveAttention  # noqa: F401
from .adaatt_grad import (AdaAttGradEngine, ExplainAdaptiveGradCam, ExplainAdaptiveGradient, ExplainAdaptiveGuidedGradCam,  # noqa: F401
                          ExplainiAdaptiveGuidedGradient)
