"""`cvap.model` surface: model registry + builder (cvap/model/__init__.py:12-26)."""
from ..registry import Registry
from .helper import *  # noqa: F401,F403
from .cvalp import CVALP
from .siamese_va import CVASP
from .classifier import ASClassifier, ESClassifier

VAL_MODELS_REGISTRY = Registry("VAL_MODELS")
VAL_MODELS_REGISTRY.__doc__ = "Registry for vision-audio-language models."
VAL_MODELS_REGISTRY.register(CVALP)
VAL_MODELS_REGISTRY.register(CVASP)
VAL_MODELS_REGISTRY.register(ESClassifier)
VAL_MODELS_REGISTRY.register(ASClassifier)


def build_main_model(cfg, echo, **kwargs):
    return VAL_MODELS_REGISTRY.get(cfg.worker)(cfg, echo)
