from .scene import SceneStitcher, scene_inference
from .sliding_window import sliding_window, sliding_window_inference

__all__ = ['sliding_window', 'sliding_window_inference', 'SceneStitcher', 'scene_inference']
