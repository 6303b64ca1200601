"""CPU: when may the |max| word remembered on a gradient tensor (ops.amax_of, attribute `_svr_amax`) be reused?  The decision
is ops.amax_cached -- host only, so it runs here on CPU tensors with a stand-in word.  A stale word is a silently wrong scale
of the "f16x3s" backward kernels (inf / NaN when the tensor grew, lost bits when it shrank); the kernels' side of this is
tests/test_gpu_amax_lifecycle.py."""
import pytest
import torch

import svr_amd  # noqa: F401
from svr_amd import ops


def _word(ring=None, serial=0):
    w = torch.zeros(1, dtype=torch.int32)
    if ring is not None:
        w._svr_ring, w._svr_serial = ring, serial
    return w


def _cached(n=24):
    t = torch.arange(n, dtype=torch.float32).reshape(4, n // 4) + 1.0
    w = _word()
    ops.amax_remember(t, w)
    assert ops.amax_cached(t) is w
    return t, w


def test_unchanged_tensor_hits():
    t, w = _cached()
    assert ops.amax_cached(t) is w and ops.amax_cached(t) is w       # as often as asked
    _ = t * 2.0, t.sum(), t.clone(), t.t().contiguous()              # out-of-place work does not touch it
    assert ops.amax_cached(t) is w


INPLACE = {
    "copy_": lambda t: t.copy_(torch.ones_like(t)),
    "mul_": lambda t: t.mul_(1024.0),
    "add_": lambda t: t.add_(torch.ones_like(t)),                    # autograd's accumulation of a second contribution
    "slice_assignment": lambda t: t.__setitem__(slice(None), torch.ones_like(t)),
    "one_element": lambda t: t.__setitem__((1, 2), 7.0),
    "foreach_mul_": lambda t: torch._foreach_mul_([t], 2.0 ** -40),
    "zero_": lambda t: t.zero_(),
    "view_flat": lambda t: t.view(-1).__setitem__(slice(3, 5), 9.0),
    "view_row": lambda t: t[1].mul_(3.0),
    "view_columns": lambda t: t[:, :2].zero_(),
}


@pytest.mark.parametrize("name", sorted(INPLACE))
def test_in_place_change_misses(name):
    """Every in-place op torch knows of moves the version counter, also through a view of the tensor (views share it)."""
    t, _ = _cached()
    INPLACE[name](t)
    assert ops.amax_cached(t) is None


def test_storage_change_misses():
    t, _ = _cached()
    t.data = torch.ones(4, 6)
    assert ops.amax_cached(t) is None
    t, _ = _cached()
    t.set_(torch.ones(4, 6))
    assert ops.amax_cached(t) is None


def test_another_tensor_object_of_the_same_memory_has_no_word():
    t, _ = _cached()
    assert ops.amax_cached(t[:, :4]) is None and ops.amax_cached(t.view(-1)) is None and ops.amax_cached(t.detach()) is None


def test_ring_age_misses():
    """A word of the ring is recycled after N // 2 - 8 more were handed out (_AmaxSlots.fresh)."""
    limit = ops._AmaxSlots.N // 2 - 8
    ring = {"serial": 100}
    t = torch.ones(8)
    w = _word(ring, 100)
    ops.amax_remember(t, w)
    assert ops.amax_cached(t) is w
    ring["serial"] = 100 + limit - 1
    assert ops.amax_cached(t) is w
    ring["serial"] = 100 + limit
    assert ops.amax_cached(t) is None


def test_force_and_forget_miss():
    t, w = _cached()
    assert ops.amax_cached(t, force=True) is None
    assert ops.amax_cached(t) is w                                   # (force asks once, it does not forget)
    ops.amax_forget(t)
    assert ops.amax_cached(t) is None and not hasattr(t, "_svr_amax") and not hasattr(t, "_svr_amax_stamp")
    ops.amax_forget(t)                                               # nothing there: fine
    ops.amax_forget(None)


def test_a_word_without_a_stamp_is_not_trusted():
    t = torch.ones(8)
    t._svr_amax = _word()
    assert ops.amax_cached(t) is None


def test_what_the_stamp_cannot_see():
    """Documented limit (amax_of's docstring): a write through `t.data` moves neither the counter nor the
    address, so the word survives it; the remedy is amax_forget / amax_of(t, force=True)."""
    t, w = _cached()
    t.data.mul_(1024.0)
    assert ops.amax_cached(t) is w
    assert ops.amax_cached(t, force=True) is None
    ops.amax_forget(t)
    assert ops.amax_cached(t) is None


def test_inference_tensors_are_never_reused():
    with torch.inference_mode():
        t = torch.ones(8)
    ops.amax_remember(t, _word())
    assert ops.amax_cached(t) is None
