from .trainer_ifnet import ImplicitRefinementTrainer, bce_with_logits_sum_mean, train_implicit_refinement  # noqa: F401
from .trainer_scene_net import SceneNetTrainer, default_hparams, run_scene_net_test, train_scene_net, use_pretrained_unet  # noqa: F401
from .trainer_unet import DepthRegressorTrainer, train_unet  # noqa: F401
from .checkpoint import TopKCheckpoints, load_checkpoint, save_checkpoint  # noqa: F401
from .fit import shard_batches  # noqa: F401
