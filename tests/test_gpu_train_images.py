"""Training images on the device: every kernel of csrc/surs_train_image.hip and the whole surs_train_images chain against the
_host twins, bit for bit (tests/test_train_images_host.py holds the twins against Pillow), and TrainDataset(images="device")."""
import random

import numpy as np
import pytest
import torch

import mesh_ref as mr
import train_data_common as tdc
from surs_amd import _lib, data, native, prng

pytestmark = pytest.mark.gpu

T = native.IMAGE_TILE      # the side of a resample and of a blur tile
G = native.JITTER_GROUP_PIXELS


def noise(tag, h, w, c=3):
    a = (prng.uniform01("gpu_train_images_" + tag, 1, h * w * c) * 256.0).astype(np.uint8)
    return a.reshape((h, w, c) if c > 1 else (h, w))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(native.require_gpu())


def same(t, a):
    return np.array_equal(t.cpu().numpy(), a)


# ---------------------------------------------------------------- resample, nearest
RESAMPLE = [((53, 37), (47, 33), _lib.FILTER_BILINEAR), ((53, 37), (66, 46), _lib.FILTER_BILINEAR), ((76, 76), (95, 95), _lib.FILTER_BILINEAR),
            ((76, 76), (76, 76), _lib.FILTER_BILINEAR), ((60, 45), (T - 1, T + 1), _lib.FILTER_BILINEAR),
            ((60, 45), (T + 1, 2 * T + 1), _lib.FILTER_BILINEAR), ((60, 45), (2 * T + 1, T - 1), _lib.FILTER_BILINEAR),
            ((64, 64), (32, 32), _lib.FILTER_BICUBIC), ((34, 66), (17, 33), _lib.FILTER_BICUBIC), ((2, 2), (1, 1), _lib.FILTER_BICUBIC),
            ((2 * T + 2, 4 * T - 2), (T + 1, 2 * T - 1), _lib.FILTER_BICUBIC)]


@pytest.mark.parametrize("src,size,filter", RESAMPLE)
def test_resample_and_nearest(src, size, filter):
    img, mask = noise("rs", *src), noise("rs_mask", *src, c=1)
    d_img, d_mask = dev(img), dev(mask)
    for window in (None, (size[1] // 3, size[0] // 3, size[1], size[0])):
        want = native.image_resample(img, size, filter=filter, window=window, host=True)
        got = native.image_resample(d_img, size, filter=filter, window=window)
        assert same(got, want), window
        assert same(native.image_resample(d_img, size, filter=filter, window=window), want)      # the same bits again
        assert same(native.image_nearest(d_mask, size, window=window), native.image_nearest(mask, size, window=window, host=True)), window


@pytest.mark.parametrize("flip", [False, True])
def test_geometry(flip):
    img, mask = noise("geo", 64, 64), noise("geo_mask", 64, 64, c=1)
    for window in ((13, 13, 64, 64), (19, 19, 64, 64), (-5, 40, 64, 64)):
        kw = dict(window=window, pad=6, flip=flip)
        assert same(native.image_resample(dev(img), (95, 95), **kw), native.image_resample(img, (95, 95), host=True, **kw))
        assert same(native.image_nearest(dev(mask), (95, 95), **kw), native.image_nearest(mask, (95, 95), host=True, **kw))


# ---------------------------------------------------------------- colour jitter
@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0), (1, 0, 3, 2)])
@pytest.mark.parametrize("size", [(17, 33), (33, 47), (200, 300)])      # one workgroup; two; 59 partial sums
def test_jitter(order, size):
    img = noise("jit", *size)
    assert (size[0] * size[1] > G) == (size != (17, 33))
    for jitter in ((order, 1.3, 0.8, 1.4, -0.07), (order, None, 1.2, None, 0.3), (order, 0.6, None, 0.5, None)):
        want = native.image_jitter(img, jitter, host=True)
        assert same(native.image_jitter(dev(img), jitter), want), jitter
        assert same(native.image_jitter(dev(img), jitter), want)


@pytest.fixture(scope="module")
def all_triples():
    g = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([g & 255, (g >> 8) & 255, g >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.mark.parametrize("jitter", [((0, 1, 2, 3), None, None, None, 0.1), ((2, 0, 1, 3), 1.3, 0.7, 1.5, -0.3), ((1, 3, 2, 0), 0.9, 1.4, 0.5, 0.5)])
def test_jitter_on_every_colour(all_triples, jitter):
    """Every RGB triple through the hue op's conversions and the blends; 16384 partial sums of L in front of the contrast."""
    assert same(native.image_jitter(dev(all_triples), jitter), native.image_jitter(all_triples, jitter, host=True))


# ---------------------------------------------------------------- blur
@pytest.mark.parametrize("size", [(64, 64), (40, 5), (5, 40), (T - 1, T + 1), (2 * T + 1, T - 1), (T + 1, 2 * T + 1)])
@pytest.mark.parametrize("radius", [0, 0.3, 1.0, 2.0, 4.0, 21.0])      # (21: a box radius of 20 per pass, the halo's limit)
def test_blur(size, radius):
    img = noise("blur", *size)
    want = native.image_blur(img, radius, host=True)
    assert same(native.image_blur(dev(img), radius), want)
    assert same(native.image_blur(dev(img), radius), want)


# ---------------------------------------------------------------- the whole chain
CHAIN = [dict(src=(64, 64), pad=6, flip=True, full=(95, 95), window=(19, 13, 64, 64), jitter=((3, 1, 0, 2), 1.3, 0.8, 1.4, -0.07), blur=1.7),
         dict(src=(64, 64), pad=6, flip=False, full=(68, 68), window=(-1, 5, 64, 64), jitter=((0, 1, 2, 3), None, None, None, None), blur=0.0),
         dict(src=(50, 70), pad=5, flip=True, full=(66, 88), window=(3, 2, 2 * T + 2, 2 * T - 2), jitter=((1, 0, 3, 2), None, 1.2, 0.7, None), blur=0.4),
         dict(src=(64, 64), augment=False), dict(src=(2 * T + 2, 2 * T - 2), augment=False)]


@pytest.mark.parametrize("case", CHAIN)
def test_train_images(case):
    case = dict(case)
    src = case.pop("src")
    plan = native.train_image_plan(src, **case)
    rgb, mask = noise("chain", *src), noise("chain_mask", *src, c=1)
    hr, lr = native.train_images(plan, rgb, mask, host=True)
    d_rgb, d_mask = dev(rgb), dev(mask)
    for _ in range(2):
        got_hr, got_lr = native.train_images(plan, d_rgb, d_mask)
        assert same(got_hr, hr) and same(got_lr, lr)
    assert hr.shape == plan.size + (3,) and lr.shape == (plan.size[0] // 2, plan.size[1] // 2, 3)


# ---------------------------------------------------------------- the dataset
def item(ds, seed=4):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return ds[0]


def test_train_dataset_device(tmp_path):
    import common
    from surs_amd import model, options, weights
    N, size = 256, 128
    param = dict(ortho_ratio=1.0, scale=0.5, center=np.array([0.0, 100.0, 0.0]), R=np.eye(3))
    root = tdc.make_dataroot(tmp_path, mr.torus(24, 12), mr.torus(12, 6), size=size, param=param)
    more = ["--random_flip", "--random_scale", "--random_trans", "--aug_blur", "2", "--aug_bri", "0.2", "--aug_con", "0.3", "--aug_sat", "0.4",
            "--aug_hue", "0.1"]
    opt = tdc.opt(root, size=size, n=N, more=more)
    on_dev, on_cpu = item(data.TrainDataset(opt, "train", seed=3, images="device")), item(data.TrainDataset(opt, "train", seed=3, images="cpu"))
    for k in ("img_HR", "img_LR"):
        assert on_dev[k].is_cuda and not on_cpu[k].is_cuda and on_dev[k].dtype == torch.float32
        assert on_dev[k].permute(0, 2, 3, 1).is_contiguous()      # NHWC in memory, as DeviceInputStage gives it
        assert torch.equal(on_dev[k].cpu(), on_cpu[k]), k
    assert tuple(on_dev["img_HR"].shape) == (1, 3, size, size) and tuple(on_dev["img_LR"].shape) == (1, 3, size // 2, size // 2)
    assert float(on_dev["img_HR"].abs().max()) > 0
    for k in ("calib", "extrinsic"):
        assert not on_dev[k].is_cuda and torch.equal(on_dev[k], on_cpu[k]), k
    # the samples do not depend on the image path
    blur_only = tdc.opt(root, size=size, n=N, more=more[:5])
    default, device = item(data.TrainDataset(blur_only, "train", seed=3)), item(data.TrainDataset(blur_only, "train", seed=3, images="device"))
    for k in ("samples_HR", "samples_LR", "labels_HR", "labels_disp"):
        assert torch.equal(default[k], device[k]) and torch.equal(default[k], on_dev[k]), k
    for k in ("img_HR", "img_LR", "calib", "extrinsic"):
        assert torch.equal(default[k], device[k].cpu()), k
    # the test phase: the half-size pair only
    test_default, test_device = item(data.TrainDataset(blur_only, "test")), item(data.TrainDataset(opt, "test", images="device"))
    assert torch.equal(test_default["img_HR"], test_device["img_HR"].cpu()) and torch.equal(test_default["img_LR"], test_device["img_LR"].cpu())

    # net.forward takes the device images as they are
    fopt = options.BaseOptions().parse(common.FLAGS)
    net = model.SuRSNet(fopt).to(device=native.require_gpu())
    net.load_state_dict(weights.synthetic_state_dict(fopt, seed=0))
    net.eval()
    d = native.require_gpu()
    res_hr, error, res_lr = net.forward(on_dev["img_LR"], on_dev["img_HR"], on_dev["samples_LR"][None], on_dev["samples_HR"][None],
                                        on_dev["calib"].to(d), labels_lr=on_dev["labels_disp"][None], labels_hr=on_dev["labels_HR"][None])
    ref_hr, ref_error, ref_lr = net.forward(on_cpu["img_LR"].contiguous().to(d), on_cpu["img_HR"].contiguous().to(d), on_dev["samples_LR"][None],
                                            on_dev["samples_HR"][None], on_dev["calib"].to(d), labels_lr=on_dev["labels_disp"][None],
                                            labels_hr=on_dev["labels_HR"][None])
    assert bool(torch.isfinite(error)) and float(error) > 0
    assert torch.equal(error, ref_error) and torch.equal(res_hr, ref_hr) and torch.equal(res_lr, ref_lr)
