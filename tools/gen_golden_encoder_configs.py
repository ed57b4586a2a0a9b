"""Golden vectors for encoders trained with --norm batch or with another --scale, from the upstream reference itself on CPU
(tools/ref_harness.py; build-container only, as tools/gen_golden.py).

    python tools/gen_golden_encoder_configs.py [keys] [bn] [scale] [recon]

keys  -> tests/golden/state_dict_keys_bn.json: the reference's state-dict keys for --norm batch (name, shape, dtype).
bn    -> tests/golden/encoder_bn_h64.npz + encoder_bn_h64_stats.npz: the reference's --norm batch encoder on synthetic_image(64, seed=1).
         The running statistics come from the reference, not from a formula: the project's synthetic weights (strict=False: they hold
         no running statistics), every BatchNorm's momentum set to 1, ONE train-mode forward on the calibration image
         synthetic_image(64, seed=7), then eval().  The statistics file holds them (and the hourglass taps).
scale -> tests/golden/encoder_scale{4_h32,3_h64,1_h128}.npz: the reference's GroupNorm encoder with --scale 4 on a 32 x 32 input, --scale 3
         on 64 x 64 and --scale 1 on 128 x 128.
recon -> tests/golden/recon_bn_scale4_r32.npz: --norm batch --scale 4 end to end on a 32 x 32 input: the dense eval_grid volumes at
         R = 32 (calibration and bounds of gen_golden_shapes.gen_recon), with the running statistics (calibrated by one train-mode pass
         of this very model on the 32 x 32 calibration image).

No committed file may exceed 1 MiB, so every map is stored as a strided sub-sample (the stride is in the file) together with the
per-channel means (float64 sums) and abs-maxima of the WHOLE map.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_harness as rh  # noqa: E402
from gen_golden import CALIB, FLAGS, GOLD  # noqa: E402
from surs_amd import options, weights  # noqa: E402

CALIBRATION_SEED = 7


def make_net(extra):
    """The reference net for FLAGS + extra with the project's synthetic weights (running statistics, if any, at their defaults)."""
    net = rh.build_net(rh.parse_opt(FLAGS + extra))
    group = [a for a in extra if a not in ("--norm", "batch")]   # (the synthetic conv / affine weights do not depend on --norm)
    sd = weights.synthetic_state_dict(options.BaseOptions().parse(FLAGS + group), seed=0)
    missing, unexpected = net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.rsplit(".", 1)[1] in ("running_mean", "running_var", "num_batches_tracked") for k in missing)
    return net


def encode(net, img):
    with torch.no_grad(), rh.quiet():
        img_sr, f_lr, f_hr = net.super_res(torch.from_numpy(img.copy()))
        net.filter_hr(f_hr)
        net.filter_lr(f_lr)
    return img_sr, f_lr, f_hr


def calibrate(net, h):
    """Running statistics = the batch statistics of ONE train-mode forward on the calibration image (momentum 1)."""
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.momentum = 1.0
    net.train()
    encode(net, weights.synthetic_image(h, seed=CALIBRATION_SEED))
    net.eval()
    stats = {k: v.numpy().copy() for k, v in net.state_dict().items()
             if k.rsplit(".", 1)[1] in ("running_mean", "running_var", "num_batches_tracked")}
    var = np.concatenate([v.ravel() for k, v in stats.items() if k.endswith("running_var")])
    print("calibrated %d BatchNorm modules, %d floats, running_var %.3g .. %.3g" %
          (len(bns), sum(v.size for k, v in stats.items() if not k.endswith("tracked")), var.min(), var.max()))
    return stats


def _put(out, name, a, step):
    a = np.asarray(a)
    out[name] = np.ascontiguousarray(a[..., ::step, ::step])
    out[name + "_step"] = np.array(step)
    out[name + "_shape"] = np.array(a.shape)
    out[name + "_mean"] = a.astype(np.float64).mean((1, 2))
    out[name + "_absmax"] = np.abs(a).max((1, 2))


def run_encoder(net, img, steps, taps_step=None):
    """steps: (img_sr, feature_lr, feature_hr, im_feat_lr, im_feat_hr) sub-sampling strides."""
    taps, hooks = {}, []
    if taps_step:
        def tap(name, mod):
            hooks.append(mod.register_forward_hook(lambda m, i, o, name=name: taps.__setitem__(name, o.detach()[0].numpy().copy())))
        tap("conv2", net.image_filter_lr.conv2)
        for i in range(3):
            tap("hg%d" % i, getattr(net.image_filter_lr, "m%d" % i))
            tap("out%d" % i, getattr(net.image_filter_lr, "l%d" % i))
    img_sr, f_lr, f_hr = encode(net, img)
    for h in hooks:
        h.remove()
    out = {}
    for name, a, st in zip(("img_sr", "feature_lr", "feature_hr", "im_feat_lr", "im_feat_hr"),
                           (img_sr[0], f_lr[0], f_hr[0], net.im_feat_list_lr[-1][0], net.im_feat_list_hr[0][0]), steps):
        _put(out, name, a.numpy(), st)
    tp = {}
    for k, v in taps.items():
        _put(tp, "tap_" + k, v, taps_step)
    for k in ("img_sr", "feature_lr", "feature_hr", "im_feat_lr", "im_feat_hr"):
        print("   %-11s %s max-abs %.3g" % (k, tuple(int(v) for v in out[k + "_shape"]), float(out[k + "_absmax"].max())))
    return out, tp


def _save(name, out):
    path = os.path.join(GOLD, name)
    np.savez_compressed(path, **out)
    n = os.path.getsize(path)
    print("%s: %d bytes" % (name, n))
    assert n < (1 << 20), "a committed file must stay below 1 MiB"


def gen_keys():
    net = rh.build_net(rh.parse_opt(FLAGS + ["--norm", "batch"]))
    keys = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net.state_dict().items()]
    with open(os.path.join(GOLD, "state_dict_keys_bn.json"), "w") as f:
        json.dump(keys, f)
    print("keys", len(keys))


def gen_bn():
    net = make_net(["--norm", "batch"])
    stats = calibrate(net, 64)
    out, taps = run_encoder(net, weights.synthetic_image(64, seed=1), (2, 2, 8, 2, 8), taps_step=4)
    _save("encoder_bn_h64.npz", out)
    _save("encoder_bn_h64_stats.npz", dict(taps, calibration_seed=np.array(CALIBRATION_SEED), **{"stat:" + k: v for k, v in stats.items()}))


def gen_scale():
    for s, h, steps in ((4, 32, (2, 2, 8, 2, 8)), (3, 64, (3, 3, 12, 3, 12)), (1, 128, (2, 2, 8, 2, 8))):
        net = make_net(["--scale", str(s)])
        print("--scale %d on %dx%d" % (s, h, h))
        out, _ = run_encoder(net, weights.synthetic_image(h, seed=1), steps)
        out["scale"], out["input_size"] = np.array(s), np.array(h)
        _save("encoder_scale%d_h%d.npz" % (s, h), out)


def gen_recon():
    ns = rh.load_reference()
    net = make_net(["--norm", "batch", "--scale", "4"])
    stats = calibrate(net, 32)
    encode(net, weights.synthetic_image(32, seed=1))
    calib = torch.from_numpy(CALIB[None].copy())
    R = 32
    coords, mat = ns.sdf.create_grid(R, R, R, np.array([-0.5] * 3), np.array([0.5] * 3))

    def eval_func(points):   # lib/mesh_util.py:20-28
        samples = torch.from_numpy(np.expand_dims(points, axis=0)).float()
        net.query_mr(samples, calib)
        net.query_sr(samples, calib)
        phr, plr = net.get_preds()
        return phr[0][0].detach().numpy(), plr[0][0].detach().numpy()

    with torch.no_grad(), rh.quiet():
        dh, dl = ns.sdf.eval_grid(coords, eval_func, num_samples=50000)
    for k, v in (("dense hr", dh), ("dense lr", dl)):
        print("%-9s range %.3f..%.3f, mean %.3f, > 0.5: %.3f" % (k, v.min(), v.max(), v.mean(), float((v > 0.5).mean())))
    _save("recon_bn_scale4_r32.npz", dict(dense_hr=dh.astype(np.float32), dense_lr=dl.astype(np.float32),
                                          calibration_seed=np.array(CALIBRATION_SEED), **{"stat:" + k: v for k, v in stats.items()}))


if __name__ == "__main__":
    todo = sys.argv[1:] or ["keys", "bn", "scale", "recon"]
    for name in todo:
        {"keys": gen_keys, "bn": gen_bn, "scale": gen_scale, "recon": gen_recon}[name]()
