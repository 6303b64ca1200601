"""GPU: ops.rgb_preprocess (csrc/rgb_preprocess.hip) against the host chain of dataset/scene_net_data.py run through Pillow:
``square_pad(image).resize((W, W), Image.BILINEAR)`` byte for byte, ``rgb_transform(image, W, resize_input)`` bit for bit."""
import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

# (H, W) -> Wout: upscale with an even pad; odd pad difference (the padded image is 7 x 8, not square) on either axis;
# upscale without a pad; the dataset's shape; scale 2.5 (6-7 taps); ~87 taps (the runtime tap loop); both passes skipped
SHAPES = [((7, 5), 8), ((5, 8), 3), ((8, 5), 3), ((33, 33), 256), ((240, 320), 256), ((480, 640), 256), ((300, 300), 7),
          ((256, 256), 256)]
CASES = [(hw, w, 3) for hw, w in SHAPES] + [((7, 5), 8, 1), ((240, 320), 256, 1)]


def _pixels(hw, bands, seed):
    return np.random.default_rng(seed).integers(0, 256, hw + (bands,), dtype=np.uint8)


def _image(a):
    return Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a)


def _host(a, W, resize_input=True, flip=False):
    """-> (resized bytes (Ho, Wo, C), rgb_transform's float tensor) of one (H, W, C) array, all on the host."""
    import importlib
    from svr_amd.dataset import scene_net_data
    # the module under the name it was first imported by: importing it as svr_amd.dataset.scene_net_data would rebind the
    # package attribute `scene_net_data` from the class to the module for every test that runs afterwards
    host = importlib.import_module(scene_net_data.__module__)
    rgb_transform, square_pad = host.rgb_transform, host.square_pad
    image = _image(a)
    if flip:
        image = image.transpose(Image.FLIP_LEFT_RIGHT)
    u8 = np.asarray(square_pad(image).resize((W, W), Image.BILINEAR) if resize_input else image, dtype=np.uint8)
    return u8.reshape(u8.shape[0], u8.shape[1], a.shape[2]), rgb_transform(image, W, resize_input)


def _same(got_f, got_u8, want_u8, want_f):
    assert got_u8.dtype == torch.uint8 and got_f.dtype == torch.float32
    assert tuple(got_u8.shape) == want_u8.shape and np.array_equal(got_u8.cpu().numpy(), want_u8)
    assert torch.equal(got_f.cpu(), want_f)


@pytest.mark.parametrize("hw,W,bands", CASES, ids=[f"{h}x{w}-{W}-c{c}" for (h, w), W, c in CASES])
def test_resize_matches_pillow_and_rgb_transform(hw, W, bands):
    import svr_amd  # noqa: F401
    from svr_amd import ops
    a = _pixels(hw, bands, seed=hw[0] * 7 + hw[1] + W + bands)
    f, u8 = ops.rgb_preprocess(torch.from_numpy(a)[None].cuda(), W=W, return_u8=True)
    assert tuple(f.shape) == (1, bands, W, W)
    _same(f[0], u8[0], *_host(a, W))


def test_batch_of_three_different_images():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    a = np.stack([_pixels((240, 320), 3, seed=40 + i) for i in range(3)])
    f, u8 = ops.rgb_preprocess(torch.from_numpy(a).cuda(), W=256, return_u8=True)
    assert tuple(f.shape) == (3, 3, 256, 256)
    for i in range(3):
        _same(f[i], u8[i], *_host(a[i], 256))
    assert torch.equal(ops.rgb_preprocess(torch.from_numpy(a).cuda(), W=256), f)         # the float output alone


@pytest.mark.parametrize("hw,W", [((7, 5), 8), ((240, 320), 256)])
def test_flip_is_flip_left_right_before_the_pad(hw, W):
    import svr_amd  # noqa: F401
    from svr_amd import ops
    a = _pixels(hw, 3, seed=91 + W)
    f, u8 = ops.rgb_preprocess(torch.from_numpy(a)[None].cuda(), W=W, flip=True, return_u8=True)
    _same(f[0], u8[0], *_host(a, W, flip=True))
    assert not torch.equal(f, ops.rgb_preprocess(torch.from_numpy(a)[None].cuda(), W=W))


@pytest.mark.parametrize("flip", [False, True])
def test_without_resize_only_layout_and_normalisation(flip):
    import svr_amd  # noqa: F401
    from svr_amd import ops
    a = _pixels((240, 320), 3, seed=5)
    f, u8 = ops.rgb_preprocess(torch.from_numpy(a)[None].cuda(), W=256, resize_input=False, flip=flip, return_u8=True)
    assert tuple(f.shape) == (1, 3, 240, 320)
    _same(f[0], u8[0], *_host(a, 256, resize_input=False, flip=flip))


def test_pad_without_resize_on_either_axis():
    """(6, 8) -> 8: the pad makes it 8 x 8 and both passes are skipped; (6, 8) -> 4 after (8, 6) -> 4: cached tables are per
    (in, out), not per call."""
    import svr_amd  # noqa: F401
    from svr_amd import ops
    for hw, W in (((6, 8), 8), ((6, 8), 4), ((8, 6), 4)):
        a = _pixels(hw, 3, seed=hw[0] + W)
        f, u8 = ops.rgb_preprocess(torch.from_numpy(a)[None].cuda(), W=W, return_u8=True)
        _same(f[0], u8[0], *_host(a, W))


def test_refuses_cpu_tensors_four_bands_and_other_dtypes():
    import svr_amd  # noqa: F401
    from svr_amd import ops
    a = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.rgb_preprocess(a)
    with pytest.raises(ValueError):
        ops.rgb_preprocess(torch.zeros(1, 8, 8, 4, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError):
        ops.rgb_preprocess(a.cuda().float())
    with pytest.raises(ValueError):
        ops.rgb_preprocess(a.cuda()[0])
