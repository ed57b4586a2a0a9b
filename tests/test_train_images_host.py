"""Training images without a device: the host twins of csrc/surs_train_image.hip (the kernels' arithmetic, csrc/surs_train_image.h)
against the installed Pillow, byte for byte, stage by stage; data.jitter_params against torchvision's draw sequence; and
TrainDataset(images="cpu") against the PIL path of images=None and against a PIL restatement of the colour jitter."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

import mesh_ref as mr
import train_data_common as tdc
from surs_amd import _lib, data, native, prng


def noise(tag, h, w, c=3):
    a = (prng.uniform01("train_images_" + tag, 1, h * w * c) * 256.0).astype(np.uint8)
    return a.reshape((h, w, c) if c > 1 else (h, w))


def ragged_mask(h, w):
    """255 inside a rectangle whose edges are no multiples of any scale used here."""
    m = np.zeros((h, w), np.uint8)
    m[h // 7 + 1: h - h // 5, w // 6 + 1: w - w // 9 - 1] = 255
    return m


def windows(w, h):
    """The whole image, and a crop window that starts inside and ends outside it."""
    return (None, (w // 3, h // 3, w, h))


def crop(im, window):
    return im if window is None else im.crop((window[0], window[1], window[0] + window[2], window[1] + window[3]))


# ---------------------------------------------------------------- resample and nearest
@pytest.mark.parametrize("size", [(53, 37), (76, 76)])
@pytest.mark.parametrize("s", [0.9, 1.0, 1.1, 1.25])
def test_bilinear_and_nearest(size, s):
    h, w = size
    img, mask = noise("bil%d" % h, h, w), ragged_mask(h, w)
    nw, nh = int(s * w), int(s * h)
    for window in windows(nw, nh):
        ref = np.asarray(crop(Image.fromarray(img).resize((nw, nh), Image.BILINEAR), window))
        assert np.array_equal(native.image_resample(img, (nh, nw), window=window, host=True), ref), (s, window)
        ref = np.asarray(crop(Image.fromarray(mask).resize((nw, nh), Image.NEAREST), window))
        assert np.array_equal(native.image_nearest(mask, (nh, nw), window=window, host=True), ref), (s, window)


@pytest.mark.parametrize("size", [(64, 64), (34, 66), (2, 2)])
def test_bicubic_half(size):
    h, w = size
    img, mask = noise("bic%d" % h, h, w), ragged_mask(h, w)
    for window in windows(w // 2, h // 2):
        ref = np.asarray(crop(Image.fromarray(img).resize((w // 2, h // 2), Image.BICUBIC), window))
        got = native.image_resample(img, (h // 2, w // 2), filter=_lib.FILTER_BICUBIC, window=window, host=True)
        assert np.array_equal(got, ref), window
        ref = np.asarray(crop(Image.fromarray(mask).resize((w // 2, h // 2), Image.NEAREST), window))
        assert np.array_equal(native.image_nearest(mask, (h // 2, w // 2), window=window, host=True), ref), window


def test_resample_refuses_a_reduction_its_tile_cannot_hold():
    with pytest.raises(_lib.SursError, match="source pixels"):
        native.image_resample(noise("big", 8, 400), (8, 100), filter=_lib.FILTER_BICUBIC, host=True)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("d", [-3, 3])
def test_geometry(flip, d):
    """get_render's PIL sequence: expand by 6, flip, resize 76 -> 95 (scale 1.25), crop 64 x 64 at dx = dy = d."""
    img, mask = noise("geo", 64, 64), ragged_mask(64, 64)
    render, m = ImageOps.expand(Image.fromarray(img), 6, fill=0), ImageOps.expand(Image.fromarray(mask), 6, fill=0)
    if flip:
        render, m = render.transpose(Image.FLIP_LEFT_RIGHT), m.transpose(Image.FLIP_LEFT_RIGHT)
    w = h = int(1.25 * 76)
    render, m = render.resize((w, h), Image.BILINEAR), m.resize((w, h), Image.NEAREST)
    x1 = y1 = int(round((w - 64) / 2.)) + d
    window = (x1, y1, 64, 64)
    assert np.array_equal(native.image_resample(img, (h, w), window=window, pad=6, flip=flip, host=True), np.asarray(crop(render, window)))
    assert np.array_equal(native.image_nearest(mask, (h, w), window=window, pad=6, flip=flip, host=True), np.asarray(crop(m, window)))


# ---------------------------------------------------------------- colour jitter
ENHANCERS = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)


def one_op(k, f):
    vals = [None] * 4
    vals[k] = f
    return ((0, 1, 2, 3),) + tuple(vals)


def pil_hue(im, h):
    hh, ss, vv = im.convert("HSV").split()
    a = ((np.asarray(hh, np.int32) + (int(h * 255) & 255)) & 255).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(a, "L"), ss, vv)).convert("RGB")


def pil_jitter(im, jitter):
    """torchvision's ColorJitter.forward with drawn parameters, on a PIL image."""
    order, vals = jitter[0], jitter[1:]
    for k in order:
        if vals[k] is None:
            continue
        im = pil_hue(im, vals[k]) if k == 3 else ENHANCERS[k](im).enhance(vals[k])
    return im


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("f", [0, 0.3, 1, 1.7])
def test_blend_ops(k, f):
    for img in (noise("blend", 17, 33), np.zeros((17, 33, 3), np.uint8), np.full((17, 33, 3), 255, np.uint8)):
        ref = np.asarray(ENHANCERS[k](Image.fromarray(img)).enhance(f))
        assert np.array_equal(native.image_jitter(img, one_op(k, f), host=True), ref)


@pytest.mark.parametrize("ones", [999, 1000, 1001])
def test_contrast_mean_beside_a_half(ones):
    """2000 grey pixels of 100 and 101: the mean of L is 100.4995, 100.5 or 100.5005, and int(mean + 0.5) is 100, 101, 101."""
    g = np.full(2000, 100, np.uint8)
    g[:ones] = 101
    img = np.ascontiguousarray(np.repeat(g.reshape(40, 50, 1), 3, 2))
    assert abs(np.asarray(Image.fromarray(img).convert("L"), np.float64).mean() - 100.5) <= 1e-3
    outs = []
    for f in (0.3, 1.7):
        ref = np.asarray(ImageEnhance.Contrast(Image.fromarray(img)).enhance(f))
        outs.append(native.image_jitter(img, one_op(1, f), host=True))
        assert np.array_equal(outs[-1], ref)
    # f = 0.3 leaves mean + 0.3 (x - mean): 100 -> 100 either way, 101 -> (uint8)100.3 or 101
    assert int(outs[0].max()) == (100 if ones == 999 else 101)


def all_triples():
    g = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([g & 255, (g >> 8) & 255, g >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_hsv_exhaustive():
    px = all_triples()
    assert np.array_equal(native.image_hsv_host(px), np.asarray(Image.fromarray(px).convert("HSV")))
    back = Image.merge("HSV", [Image.fromarray(np.ascontiguousarray(px[..., c]), "L") for c in range(3)]).convert("RGB")
    assert np.array_equal(native.image_hsv_host(px, inverse=True), np.asarray(back))


@pytest.mark.parametrize("h", [-0.5, -0.1, 0.1, 0.5])
def test_hue(h):
    img = noise("hue", 17, 33)
    assert np.array_equal(native.image_jitter(img, one_op(3, h), host=True), np.asarray(pil_hue(Image.fromarray(img), h)))


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 1, 0, 2), (2, 3, 1, 0), (1, 0, 3, 2)])
def test_jitter_chain(order):
    """All four ops in an order: the contrast mean is taken from the image as the ops in front of it leave it."""
    img = noise("chain", 33, 47)
    jitter = (order, 1.3, 0.8, 1.4, -0.07)
    assert np.array_equal(native.image_jitter(img, jitter, host=True), np.asarray(pil_jitter(Image.fromarray(img), jitter)))
    jitter = (order, None, 1.2, None, 0.3)
    assert np.array_equal(native.image_jitter(img, jitter, host=True), np.asarray(pil_jitter(Image.fromarray(img), jitter)))


# ---------------------------------------------------------------- blur
@pytest.mark.parametrize("size", [(64, 64), (40, 5), (5, 40)])
@pytest.mark.parametrize("radius", [0, 0.3, 1.0, 2.0, 4.0])
def test_blur(size, radius):
    img = noise("blur%d" % size[0], *size)
    ref = np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius)))
    assert np.array_equal(native.image_blur(img, radius, host=True), ref)


def test_blur_refuses_a_radius_its_halo_cannot_hold():
    with pytest.raises(_lib.SursError, match="box radius"):
        native.image_blur(noise("blur_big", 8, 8), 40.0, host=True)


# ---------------------------------------------------------------- the draws
AMOUNTS = [(0.2, 0.3, 0.4, 0.1), (0.5, 0.5, 0.5, 0.5), (0.2, 0.0, 0.0, 0.1), (0.0, 0.3, 0.4, 0.0), (0.0, 0.0, 0.25, 0.05),
           (0.0, 0.0, 0.0, 0.0)]


def jitter_opt(root, amounts, more=()):
    flags = []
    for k, a in zip(data.JITTER_OPTIONS, amounts):
        flags += ["--" + k, repr(a)]
    return tdc.opt(root, more=flags + list(more))


@pytest.mark.parametrize("amounts", AMOUNTS)
@pytest.mark.parametrize("seed", [0, 7])
def test_jitter_params(amounts, seed):
    torch.manual_seed(seed)
    got = data.jitter_params(jitter_opt("unused", amounts))
    torch.manual_seed(seed)
    fn_idx = torch.randperm(4)
    b, c, s, h = amounts
    want = [None if b == 0 else float(torch.empty(1).uniform_(max(0, 1 - b), 1 + b)),
            None if c == 0 else float(torch.empty(1).uniform_(max(0, 1 - c), 1 + c)),
            None if s == 0 else float(torch.empty(1).uniform_(max(0, 1 - s), 1 + s)),
            None if h == 0 else float(torch.empty(1).uniform_(-h, h))]
    assert got == (tuple(int(i) for i in fn_idx),) + tuple(want)
    after = torch.rand(1)
    torch.manual_seed(seed)
    data.jitter_params(jitter_opt("unused", amounts))
    assert torch.equal(torch.rand(1), after)      # and nothing else was drawn


def test_jitter_params_refuses_amounts_outside_the_convention():
    with pytest.raises(ValueError, match="aug_hue"):
        data.jitter_params(jitter_opt("unused", (0.1, 0.1, 0.1, 0.6)))


# ---------------------------------------------------------------- the dataset
@pytest.fixture(scope="module")
def dataroot(tmp_path_factory):
    return tdc.make_dataroot(tmp_path_factory.mktemp("train_images_root"), mr.torus(8, 6), mr.torus(6, 4), size=64)


def render(ds, subject="alpha", seed=11):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return ds.get_render(subject, num_views=1)


VARIANTS = {"plain": ((), "train"), "flip": (("--random_flip",), "train"), "scale_trans": (("--random_scale", "--random_trans"), "train"),
            "blur": (("--aug_blur", "2"), "train"), "all": (("--random_flip", "--random_scale", "--random_trans", "--aug_blur", "3"), "train"),
            "test": (("--random_flip", "--random_scale", "--random_trans", "--aug_blur", "2"), "test")}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("seed", [11, 13])      # (np.random.rand() > 0.5 under seed 13, not under seed 11: both flip branches)
def test_dataset_cpu_equals_pil_path(dataroot, variant, seed):
    more, phase = VARIANTS[variant]
    subject = "alpha" if phase == "train" else "beta"
    ref = render(data.TrainDataset(tdc.opt(dataroot, more=more), phase), subject, seed)
    state = (random.getstate(), np.random.get_state()[1].copy())
    got = render(data.TrainDataset(tdc.opt(dataroot, more=more), phase, images="cpu"), subject, seed)
    assert sorted(got) == sorted(ref)
    for k in ref:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), k
    assert random.getstate() == state[0] and np.array_equal(np.random.get_state()[1], state[1])      # the same draws
    assert got["img_HR"].permute(0, 2, 3, 1).is_contiguous() and got["img_LR"].permute(0, 2, 3, 1).is_contiguous()      # NHWC in memory


def test_flip_seeds_cover_both_branches():
    np.random.seed(11)
    a = np.random.rand()
    np.random.seed(13)
    assert a <= 0.5 < np.random.rand()


def tensors(render_hr, mask_hr):
    """Lines 276-284 of data.TrainDataset.get_render."""
    pair = []
    for mask, img in ((mask_hr.resize([x // 2 for x in mask_hr.size], Image.NEAREST), render_hr.resize([x // 2 for x in render_hr.size], Image.BICUBIC)),
                      (mask_hr, render_hr)):
        m = data.TrainDataset._to_tensor(mask)
        r = (data.TrainDataset._to_tensor(img) - np.float32(0.5)) / np.float32(0.5)
        pair.append(torch.from_numpy(np.ascontiguousarray(m * r))[None])
    return pair


@pytest.mark.parametrize("amounts", AMOUNTS[:5])
def test_dataset_jitter_against_pil(dataroot, amounts):
    """Jitter on, then blur: with no flip, scale or translation the crop is the decoded image itself."""
    opt = jitter_opt(dataroot, amounts, more=["--aug_blur", "2"])
    with pytest.raises(NotImplementedError):
        data.TrainDataset(opt, "train")
    got = render(data.TrainDataset(opt, "train", images="cpu"), seed=5)
    torch.manual_seed(5)
    jitter = data.jitter_params(opt)
    np.random.seed(5)
    radius = np.random.uniform(0, 2.0)
    img = Image.open(os.path.join(dataroot, "RENDER", "alpha", "0_0_00.png")).convert("RGB")
    mask = Image.open(os.path.join(dataroot, "MASK", "alpha", "0_0_00.png")).convert("L")
    img = pil_jitter(img, jitter).filter(ImageFilter.GaussianBlur(radius))
    lr, hr = tensors(img, mask)
    assert torch.equal(got["img_HR"], hr) and torch.equal(got["img_LR"], lr)
    plain = render(data.TrainDataset(tdc.opt(dataroot, more=["--aug_blur", "2"]), "train"), seed=5)
    assert not torch.equal(got["img_HR"], plain["img_HR"]) and torch.equal(got["calib"], plain["calib"])


def test_images_argument(dataroot):
    with pytest.raises(ValueError, match="images"):
        data.TrainDataset(tdc.opt(dataroot), "train", images="gpu")
