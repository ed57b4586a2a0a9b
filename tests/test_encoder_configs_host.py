"""Host side of the encoder options --norm batch and --scale: the key list against the reference's (tests/golden/state_dict_keys_bn.json,
tools/gen_golden_encoder_configs.py), strict loading, the BatchNorm fold, the refusals at construction and the size rules."""
import json
import os

import numpy as np
import pytest
import torch

import common
from surs_amd import encoder, model, options, weights


def _opt(*extra):
    return options.BaseOptions().parse(common.FLAGS + list(extra))


def test_batchnorm_key_list_equals_the_references(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "state_dict_keys_bn.json")))
    spec = weights.state_dict_spec(_opt("--norm", "batch"))
    assert len(ref) == len(spec) == 1036
    assert [k for k, _, _ in ref] == [k for k, _, _ in spec]                       # names, in the reference's order
    assert [tuple(s) for _, s, _ in ref] == [tuple(s) for _, s, _ in spec]
    sd = weights.synthetic_state_dict(_opt("--norm", "batch"))
    assert [d for _, _, d in ref] == [str(sd[k].dtype) for k, _, _ in ref]          # float32, num_batches_tracked int64
    assert sum(k.endswith("num_batches_tracked") for k in sd) == 161
    # the alias of bn4 inside `downsample` carries the same arrays
    assert sd["image_filter_hr.conv2.downsample.0.running_var"] is sd["image_filter_hr.conv2.bn4.running_var"]


def test_groupnorm_key_list_is_unchanged(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "state_dict_keys.json")))
    for opt in (_opt(), _opt("--norm", "group"), _opt("--scale", "4")):
        spec = weights.state_dict_spec(opt)
        assert [(k, tuple(s)) for k, s in ref] == [(k, tuple(s)) for k, s, _ in spec]


def test_strict_load_of_batchnorm_state_dicts():
    net = model.SuRSNet(_opt("--norm", "batch"))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.synthetic_state_dict(_opt("--norm", "batch"), seed=3).items()}
    sd["image_filter_lr.bn_end1.num_batches_tracked"] = torch.tensor(77)
    net.load_state_dict(sd)
    back = net.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) and back[k].dtype == sd[k].dtype for k in sd)
    assert back["image_filter_lr.bn_end1.num_batches_tracked"].dtype == torch.int64
    less = dict(sd)
    del less["image_filter_lr.m1.b2_2.bn2.running_var"]
    with pytest.raises(RuntimeError, match=r"missing \['image_filter_lr.m1.b2_2.bn2.running_var'\]"):
        net.load_state_dict(less)
    group = {k: torch.from_numpy(v) for k, v in common.state_dict().items()}
    with pytest.raises(RuntimeError, match="missing .*running_mean"):
        net.load_state_dict(group)
    with pytest.raises(RuntimeError, match="unexpected .*running_mean"):
        model.SuRSNet(_opt()).load_state_dict(sd)


def test_batchnorm_fold_is_the_float64_formula(golden_dir):
    """Sites with the reference's calibrated statistics (running_var down to 1e-6: eps matters)."""
    gold = np.load(os.path.join(golden_dir, "encoder_bn_h64_stats.npz"))
    sd = weights.synthetic_state_dict(_opt("--norm", "batch"))
    for site in ("image_filter_lr.conv2.bn1", "image_filter_lr.m0.b2_plus_1.bn3", "image_filter_lr.m2.b3_2.bn2", "image_filter_lr.bn_end2"):
        w, b = sd[site + ".weight"], sd[site + ".bias"]
        m, v = gold["stat:" + site + ".running_mean"], gold["stat:" + site + ".running_var"]
        sc, sh = weights.fold_batchnorm(w, b, m, v)
        want_sc = w.astype(np.float64) / np.sqrt(v.astype(np.float64) + 1e-5)
        want_sh = b.astype(np.float64) - m.astype(np.float64) * want_sc
        assert sc.dtype == sh.dtype == np.float32
        assert np.array_equal(sc, want_sc.astype(np.float32)) and np.array_equal(sh, want_sh.astype(np.float32))
        x = np.linspace(-2, 2, 7)[:, None]
        ref = (x - m) / np.sqrt(v.astype(np.float64) + 1e-5) * w + b          # BatchNorm2d in eval mode
        assert np.abs(x * sc + sh - ref).max() <= 1e-6 * np.abs(ref).max()
    assert float(min(gold[k].min() for k in gold.files if k.endswith("running_var"))) < 1e-5   # (the fixture does exercise eps)


@pytest.mark.parametrize("extra,words", [(("--norm", "instance"), "'group' and 'batch'"), (("--scale", "0"), "integer in 1..4"),
                                         (("--scale", "5"), "integer in 1..4"), (("--scale", "-2"), "integer in 1..4")])
def test_unsupported_values_are_refused_at_construction(extra, words):
    with pytest.raises(ValueError, match=words):
        model.SuRSNet(_opt(*extra))


def test_supported_values_construct():
    for extra in (("--norm", "batch"), ("--scale", "1"), ("--scale", "3"), ("--norm", "batch", "--scale", "4")):
        model.SuRSNet(_opt(*extra))
    with pytest.raises(ValueError, match="integer in 1..4"):
        encoder.check_scale(2.5)


def test_size_rules_are_stated_on_the_enlarged_image():
    # factor 2: the accepted sizes and the words of old
    encoder.check_image_size(36, 64, 2)
    with pytest.raises(ValueError, match=r"multiples of 4 \(three stride-2 stages\), got 66x64"):
        encoder.check_image_size(66, 64, 2)
    # other factors: both sizes and the factor in the message
    for h, w, s in ((32, 32, 4), (30, 32, 4), (64, 8, 3), (128, 136, 1), (2, 2, 4)):
        encoder.check_image_size(h, w, s)
    with pytest.raises(ValueError, match="input image 31x32 enlarged by the factor 4 is 124x128: .* multiples of 8"):
        encoder.check_image_size(31, 32, 4)
    with pytest.raises(ValueError, match="input image 64x66 enlarged by the factor 3 is 192x198"):
        encoder.check_image_size(64, 66, 3)
    with pytest.raises(ValueError, match="input image 126x128 enlarged by the factor 1 is 126x128"):
        encoder.check_image_size(126, 128, 1)
    # feature_lr = a quarter of the enlarged image, halved hg_depth times
    encoder.check_feature_lr_size(48, 48, 2, 3)
    with pytest.raises(ValueError, match="feature_lr size must be a multiple of 2\\^hg_depth$"):
        encoder.check_feature_lr_size(18, 16, 2, 2)
    with pytest.raises(ValueError, match="multiple of 2\\^hg_depth = 4: got 6x8, a quarter of the enlarged image of 24x32 .factor 4: an input image of 6x8"):
        encoder.check_feature_lr_size(6, 8, 2, 4)
