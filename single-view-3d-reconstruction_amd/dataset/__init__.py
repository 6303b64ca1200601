from .implicit_dataset import DeviceSampleLoader, ImplicitDataset  # noqa: F401
from .scene_net_data import scene_net_data  # noqa: F401
