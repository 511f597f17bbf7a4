"""Per-model explainers (mirror of the `Explain*` classes of models/gridTDmodel.py / models/aoamodel.py / models/adaptiveattention.py)."""
from .adaatt import AdaAttEngine, ExplainAdaptiveAttention  # noqa: F401
from .adaatt_grad import (AdaAttGradEngine, ExplainAdaptiveGradCam, ExplainAdaptiveGradient, ExplainAdaptiveGuidedGradCam,  # noqa: F401
                          ExplainiAdaptiveGuidedGradient)
from . import ablation  # noqa: F401
from .beam import beam_search_batch, caption_batch  # noqa: F401
from .ablation import image_ablation, word_ablation, word_prob  # noqa: F401
