"""Per-model explainers (mirror of the `Explain*` classes of models/gridTDmodel.py / models/aoamodel.py / models/adaptiveattention.py)."""
from .adaatt import AdaAttEngine, ExplainAdaptiveAttention  # noqa: F401
from .adaatt_grad import (AdaAttGradEngine, ExplainAdaptiveGradCam, ExplainAdaptiveGradient, ExplainAdaptiveGuidedGradCam,  # noqa: F401
                          ExplainiAdaptiveGuidedGradient)
from . import ablation, attention, experiments  # noqa: F401
from .beam import beam_search_batch, caption_batch, diverse_beam_search_batch, diverse_captions_batch  # noqa: F401
from .ablation import image_ablation, word_ablation, word_prob  # noqa: F401
from .attention import attention_maps, gradcam_maps, one_minus_beta  # noqa: F401
from .experiments import bbox_correctness, tpfp_statistics  # noqa: F401
