from .ifnet import IFNet, IFNetFeatureExtractor, IFNetFeatureExtractor128, evaluate_network_on_grid, evaluate_network_on_grid_device, \
    evaluate_network_on_grid_sparse, implicit_to_mesh, make_3d_grid  # noqa: F401
from .projection import project  # noqa: F401
from .unet import UNetMini, Unet  # noqa: F401
