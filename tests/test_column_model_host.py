"""tests/column_model.py is checked before it judges a kernel (no GPU, no product code):
  * with every rounding switched off it IS the classifier: `dense` equals grad_common.mlp_forward on point_rows, `restated` equals
    `dense` (the identity of test_oracle_restatement.py, through the model's own code);
  * its bf16 conversion is torch.bfloat16's;
  * the bound of tests/test_gpu_column_model.py separates wrong models: four perturbed float64 models - (a) truncating 16-bit
    conversion of the activations, (b) one layer-0 channel's contribution missing over ten voxels, (c) the depth feature one voxel
    off in the ragged tile, (d) b1 through a 16-bit rounding - each break it against the unperturbed model, in the mean, the
    max or the median, on the gain-1 case of grid S (tests/column_bits.py), for both models and both precisions."""
import numpy as np
import pytest
import torch

import column_bits as cb
import column_model as cm
import common
import grad_common as gc
from surs_amd import weights

_cache = {}


def s_case(gain=1):
    """(mlp state dict with layer 0's depth column x gain, geometry closure) of grid S: column_bits' 2 x 8 x 296."""
    sd = {k: np.array(v, copy=True) for k, v in common.state_dict().items() if k.startswith("mlp_")}
    for m in ("mlp_lr.", "mlp_hr."):
        sd[m + "conv0.weight"][:, 320] *= float(gain)
    fl, fh = weights.body_features(32, 128)
    cols = [(cb.I0 + i, j) for i in range(cb.PLANES) for j in range(cb.RY)]
    return sd, lambda R: cm.sweep_geometry(R, cb.matrix(), common.CALIB, cols, cb.RZ, cb.ZMUL, cb.ZDIV, fl, fh)


def model(fn, prec, acc=np.float64, order="asc"):
    key = (fn.__name__, prec, acc, order)
    if key not in _cache:
        sd, geom = s_case()
        _cache[key] = fn(sd, prec, geom, acc=acc, order=order)
    return _cache[key]


def test_rounding_off_the_model_is_the_classifier():
    sd, geom = s_case()
    off = cm.Rounding("bf16", on=False)
    d = cm.dense(sd, "bf16", geom, rounding=False)
    r = cm.restated(sd, "bf16", geom, rounding=False)
    # the same voxels as points, through grad_common's restatement
    mat = cb.matrix().reshape(3, 4)
    idx = np.array([(cb.I0 + i, j, k, 1.0) for i in range(cb.PLANES) for j in range(cb.RY) for k in range(cb.RZ)], np.float64).T
    pts = mat @ idx
    cal4 = np.asarray(common.CALIB, np.float64)
    fl, fh = weights.body_features(32, 128)
    rows, mask, _ = gc.point_rows(fl, fh, pts, cal4)
    assert off.f(np.float64(1.0) / 3.0) == 1.0 / 3.0 and mask.all()
    (Wl, bl), (Wh, bh) = gc._layers(sd, "mlp_lr."), gc._layers(sd, "mlp_hr.")
    lg_l = gc.mlp_forward(Wl, bl, set(cm.RES), rows)[0]
    q = mask * cm.sigmoid(lg_l)
    lg_h = gc.mlp_forward(Wh, bh, set(cm.RES), np.concatenate([rows, q[None]]))[0]
    for tag, want in (("lr", lg_l), ("hr", lg_h)):
        want = want.reshape(cb.PLANES * cb.RY, cb.RZ)
        top = np.abs(want).max()
        e_dense = np.abs(d["logit_" + tag] - want).max() / top
        e_rest = np.abs(r["logit_" + tag] - d["logit_" + tag]).max() / top
        print("rounding off, %s: dense vs mlp_forward %.2e, restated vs dense %.2e (of the largest logit %.3f)" % (tag, e_dense, e_rest, top))
        assert e_dense <= 1e-12 and e_rest <= 1e-9


def test_bf16_conversion_is_torch_bfloat16():
    rng = np.random.RandomState(16)
    bits = rng.randint(0, 2 ** 32, 10 ** 6, dtype=np.uint64).astype(np.uint32)
    bits[:20000] = (bits[:20000] & np.uint32(0xffff0000)) | np.uint32(0x8000)          # ties: to even, both parities of bit 16
    bits[20000:40000] &= np.uint32(0x807fffff)                                         # fp32 denormals (bf16's too)
    bits[40000:40008] = np.array([0x7f7fffff, 0xff7fffff, 0x7f7f0000, 0x7f7f8000, 0x7f7f7fff, 0x00000000, 0x80000000, 0x00008000],
                                 np.uint32)                                            # the largest finite values, zeros, the smallest tie
    x = bits.view(np.float32)
    x = x[np.isfinite(x)]
    assert x.size > 990000
    got = cm.bf16_round(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isinf(cm.bf16_round(np.array([np.finfo(np.float32).max], np.float32))[0])
    # and the wrong conversion of perturbation (a) is a different one
    assert (cm.bf16_truncate(x).view(np.uint32) != got.view(np.uint32)).mean() > 0.4


def _ratios(ref, forms, pert):
    """(dev mean / e mean, dev max / e max, dev median / its bound, the statistics that break their bound) per classifier."""
    out = {}
    for tag in ("lr", "hr"):
        sel = np.broadcast_to((ref["mask"] > 0)[:, None], ref["logit_" + tag].shape)
        bound, e = cm.bounds(ref, forms, tag, sel)
        dev = np.abs(pert["logit_" + tag] - ref["logit_" + tag])[sel]
        out[tag] = (dev.mean() / e.mean(), dev.max() / e.max(), np.median(dev) / bound["median"], cm.breaks(dev, bound))
    return out


@pytest.mark.parametrize("fn", [cm.restated, cm.dense], ids=["restated", "dense"])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_the_bound_separates_wrong_models(fn, prec):
    sd, geom = s_case()
    ref = model(fn, prec)
    forms = [model(fn, prec, np.float32, o) for o in ("asc", "desc")]
    for tag in ("lr", "hr"):
        assert np.abs(ref["logit_" + tag]).max() < cm.SAT                # no voxel of this case is saturated
        assert not _ratios(ref, forms, forms[0])[tag][3]                 # and the bound holds for what it has to let through
    # (b): the channel with the largest activation over voxels 100 .. 109 of column 3 (the contribution of a channel that is
    # nearly zero there is nearly nothing, and nothing can notice its absence)
    act = cm.layer0_lr(sd, prec, geom)[:, 3, 100:110]
    ch = int(np.argmax(act.min(1)))
    perts = {"a truncated activations": {"trunc_act": True},
             "b channel %d missing over 10 voxels" % ch: {"drop": (ch, 3, slice(100, 110))},
             "c depth one voxel off in the ragged tile": {"zshift": 256},
             "d b1 through 16 bits": {"b1_16": True}}
    for name, pert in perts.items():
        got = _ratios(ref, forms, fn(sd, prec, geom, pert=pert))
        print("%s %s, (%s): lr mean %.1fx max %.1fx of e_model, median %.1fx of its bound, breaks %s; hr mean %.1fx max %.1fx, median %.1fx, "
              "breaks %s" % ((fn.__name__, prec, name) + got["lr"] + got["hr"]))
        assert got["lr"][3], (name, got)
