"""unimm_amd -- MI355X-native (gfx950) implementation of the UniMM-UL forward/backward hot path.

Drop-in surface (same names / signatures as the reference):
    from unimm_amd import VisualDialogEncoder, BertForMultiModalPreTraining, BertConfig
"""
from . import reward
from .config import BertConfig
from .modeling import BertForMultiModalPreTraining, VisualDialogEncoder
from .policy import DistillObjective, PolicyObjective, PreferenceObjective, PreferenceTargets, frozen_reference
from .scoring import SharedContext

__version__ = "0.1.0"
__all__ = ["BertConfig", "BertForMultiModalPreTraining", "VisualDialogEncoder", "SharedContext", "PolicyObjective",
           "frozen_reference", "PreferenceObjective", "PreferenceTargets", "DistillObjective", "reward"]
