"""Host-side mirror of the reference's util package: the mesh output of util/visualize.py and the mesh metrics of
util/evaluate.py (``from svr_amd.util import eval_mesh, eval_pointcloud, distance_p2p, sample_surface``)."""
_EVALUATE = ("distance_p2p", "eval_mesh", "eval_pointcloud", "sample_surface")
__all__ = list(_EVALUATE)


def __getattr__(name):          # resolved on first use: `python -m svr_amd.util.evaluate` must not find itself imported
    if name in _EVALUATE:
        from . import evaluate
        return getattr(evaluate, name)
    raise AttributeError(name)
