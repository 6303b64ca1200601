from .trainer_ifnet import ImplicitRefinementTrainer, bce_with_logits_sum_mean  # noqa: F401
from .trainer_scene_net import SceneNetTrainer, default_hparams, use_pretrained_unet  # noqa: F401
from .trainer_unet import DepthRegressorTrainer, train_unet  # noqa: F401
from .checkpoint import load_checkpoint, save_checkpoint  # noqa: F401
