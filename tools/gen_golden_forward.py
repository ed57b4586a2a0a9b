"""Generate tests/golden/forward_h64.npz by running the reference's SuRSNet.forward on the CPU.

Build container only, through tools/ref_harness.py.  The released shape and s1 (the 512-wide pair of tests/test_gpu_mlp_shapes.py),
in train mode (three stacks) and eval mode (one): per-stack predictions, the four loss terms, the total, img_SR; the inputs come
from seeds (tests/forward_common.py), so only the reference's outputs, the seeds and the flags are stored.

    python tools/gen_golden_forward.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ref_harness as rh  # noqa: E402
import forward_common as fc  # noqa: E402
from surs_amd import options, weights  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    torch.set_num_threads(8)
    x = fc.inputs()
    T = lambda k: torch.from_numpy(x[k].copy())
    out = dict(meta=np.array(json.dumps(dict(
        B=fc.B, H=fc.H, N=fc.N, image_seeds=[1 + b for b in range(fc.B)], images_hr=["img_hr", 7],
        points_hr_seeds=[30 + b for b in range(fc.B)], points_lr_seeds=[40 + b for b in range(fc.B)], labels=["lab_hr", "lab_lr", 1],
        weights_seed=0, loss_weights=list(fc.LOSS_WEIGHTS), flags={n: fc.flags(n) for n in fc.SHAPES}))))
    for name in fc.SHAPES:
        opt_ref = rh.parse_opt(fc.flags(name))
        net = rh.build_net(opt_ref)
        sd = weights.synthetic_state_dict(options.BaseOptions().parse(fc.flags(name)), seed=0)
        net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        for mode in fc.MODES:
            net.train(mode == "train")
            with torch.no_grad(), rh.quiet():
                res_hr, err, res_lr = net.forward(T("images_lr"), T("images_hr"), T("points_lr"), T("points_hr"), T("calibs"),
                                                  labels_lr=T("labels_lr"), labels_hr=T("labels_hr"))
                terms = [net.get_error_lr(), net.get_error_hr(), net.get_errorSR(net.im_SR, T("images_hr")), net.get_error_disp_1()]
            tag = "%s_%s_" % (name, mode)
            out[tag + "pred_lr"] = np.stack([p[:, 0].numpy() for p in net.intermediate_preds_list_lr])   # [S,B,N]
            out[tag + "pred_hr"] = np.stack([p[:, 0].numpy() for p in net.intermediate_preds_list_hr])
            out[tag + "terms"] = np.array([float(t) for t in terms], np.float32)
            out[tag + "total"] = np.float32(err.item())
            assert torch.equal(res_hr, net.intermediate_preds_list_hr[-1]) and torch.equal(res_lr, net.intermediate_preds_list_lr[-1])
            sr = net.im_SR.numpy()
            if "img_sr" in out:   # (the encoder does not depend on the classifiers' shape or on the mode)
                assert np.array_equal(out["img_sr"], sr)
            out["img_sr"] = sr
            e, tot = fc.terms_f64(out[tag + "pred_lr"], out[tag + "pred_hr"], x["labels_lr"], x["labels_hr"], sr, x["images_hr"])
            print(tag, "stacks", len(net.intermediate_preds_list_lr), "total", err.item(), "f64", tot, "diff", abs(err.item() - tot),
                  "term diffs", np.abs(e - out[tag + "terms"]), "outside", float(np.mean(out[tag + "pred_lr"][-1] == 0)), file=sys.__stdout__)
    path = os.path.join(GOLD, "forward_h64.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", file=sys.__stdout__)


if __name__ == "__main__":
    main()
