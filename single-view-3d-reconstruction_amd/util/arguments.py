"""Mirror of the reference's util/arguments.py: the command-line flags of the three training entry points, their defaults
and the post-processing of :48-62, one for one.

``parse_arguments(argv=None, timestamp=True)``: `argv` as for argparse (None = the process's own).  The reference prefixes
the experiment name with the wall clock (``%d%m%H%M_``); ``timestamp=False`` leaves the name as given, so that a caller (a
test, a script that names its own runs) gets a reproducible directory.  The reference parses once at import time into a
module-level `args`; nothing is parsed here before the call."""
import argparse
from datetime import datetime
from pathlib import Path
from random import randint


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--num_workers', type=int, default=0, help='num workers')
    parser.add_argument('--gpu', type=int, nargs='+', default=0, help='gpus')
    parser.add_argument('--sanity_steps', type=int, default=2, help='validation batches run before training')
    parser.add_argument('--resume', type=str, default=None, help='resume checkpoint')
    parser.add_argument('--splitsdir', type=str, default='overfit', help='splits directory')
    parser.add_argument('--datasetdir', type=str, help='datasetdir', default='data')
    parser.add_argument('--val_check_percent', type=float, default=0.5, help='percentage of val checked')
    parser.add_argument('--val_check_interval', type=float, default=0.25, help='check val every fraction of epoch')
    parser.add_argument('--max_epoch', type=int, default=100, help='number of epochs to train for')
    parser.add_argument('--save_epoch', type=int, default=1, help='save every nth epoch')
    parser.add_argument('--lr', type=float, default=0.0001, help='learning rate')
    parser.add_argument('--batch_size', type=int, default=16, help='batch size')
    parser.add_argument('--experiment', type=str, default='scenes_net', help='experiment directory')
    parser.add_argument('--seed', type=int, default=-1, help='random seed')
    parser.add_argument('--W', type=int, default=256)
    parser.add_argument('--sigma', nargs='+', type=float, default=[1.5], help='point_extent')
    parser.add_argument('--kernel_size', nargs='+', type=int, default=[3, 3, 3], help='kernel size for voxelization')
    parser.add_argument('--num_points', type=int, default=2048)
    parser.add_argument('--net_res', type=int, default=128, help='Architecture of the Network and number of features')
    parser.add_argument('--inf_res', type=int, default=1, help='Multiple of inference resolution per training grid resolution')
    parser.add_argument('--precision', type=int, default=32, help='float32 or float16 network precision')
    parser.add_argument('--profiler', type=str, default=None, help='Profiler: None, simple or Advanced')
    parser.add_argument('--version', type=str, default=None, help='version for logs name')
    parser.add_argument('--resize_input', dest='resize_input', action='store_true', help='Square pad and resize the rgb image input')
    parser.add_argument('--pretrain_unet', default=None, help='use a pretrained Unet')
    parser.add_argument('--visualize', dest='visualize', action='store_true', help='Output visualizations every validation')
    parser.add_argument('--min_z', type=float, default=0.1953997164964676,
                        help='minimum depth value for the dataset. Used during normalization of predicted depth.')
    # (the data's largest depth is 24.6, but very few pixels exceed 7)
    parser.add_argument('--max_z', type=float, default=7.0,
                        help='maximum depth value for the dataset. Used during normalization of predicted depth.')
    parser.add_argument('--scale_factor', type=int, default=1, help='Down scale the voxel grid input.')
    parser.add_argument('--subsample_points', type=int, default=0, help='Use n points from projected pointclouds instead of all')
    parser.add_argument('--skip_unet', dest='skip_unet', action='store_true', help='Skips Unet and uses GT depth instead')
    parser.add_argument('--no_depth_sup', dest='no_depth_sup', action='store_true', help='Disables depth supervision')
    parser.add_argument('--test', type=str, default=None, help='load and test from model-checkpoint')
    return parser


def post_process(args, timestamp=True):
    """arguments.py:48-62, on a parsed namespace."""
    if len(args.kernel_size) == 1:
        args.kernel_size = args.kernel_size * 3
    if len(args.sigma) == 1:
        args.sigma = args.sigma * 3
    if args.seed == -1:
        args.seed = randint(0, 999)
    if args.val_check_interval > 1:
        args.val_check_interval = int(args.val_check_interval)
    if timestamp:
        args.experiment = f"{datetime.now().strftime('%d%m%H%M')}_{args.experiment}"
    if args.resume is not None:
        args.experiment = Path(args.resume).parents[0].name
    return args


def parse_arguments(argv=None, timestamp=True):
    return post_process(build_parser().parse_args(argv), timestamp)
