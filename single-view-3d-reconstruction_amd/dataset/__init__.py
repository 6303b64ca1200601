from .implicit_dataset import DeviceSampleLoader, ImplicitDataset  # noqa: F401
from .scene_net_data import scene_net_data  # noqa: F401
from .scenes_dataset import ScenesDataset  # noqa: F401
