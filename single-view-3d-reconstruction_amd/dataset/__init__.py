from .implicit_dataset import BatchedSampleLoader, DeviceSampleLoader, ImplicitDataset  # noqa: F401
from .scene_net_data import DeviceSceneLoader, scene_net_data  # noqa: F401
from .scenes_dataset import ScenesDataset  # noqa: F401
