from .callback import Callback, EvaluationCallback, SaveCheckpointCallback
from .configurable import ConfigurableMixin
from .learning_rate import LearningRateBase
from .module import ERModule
from .dataloader import ERDataLoader, ERDataset
from .transform_base import Transform, MultiTransform

__all__ = ['ERModule', 'ConfigurableMixin', 'ERDataLoader', 'ERDataset', 'Callback', 'SaveCheckpointCallback',
           'EvaluationCallback', 'LearningRateBase', 'Transform', 'MultiTransform']
