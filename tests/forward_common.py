"""Inputs and the float64 restatement of the loss for the validation-forward tests (tests/golden/forward_h64.npz,
tools/gen_golden_forward.py): everything comes from seeds, the fixture holds the reference's outputs only."""
import numpy as np

import common
from surs_amd import prng, weights

B, H, N = 2, 64, 3000
LOSS_WEIGHTS = (0.5, 2.0, 0.25, 1.5)      # --mlp1 --mlp2 --srweight --dispweight: all different, so that a swapped weight shows
S1 = ["--mlp_dim_lr", "321", "512", "256", "128", "1", "--mlp_dim_hr", "322", "512", "256", "128", "1",
      "--mlp_res_layers_lr", "1", "2", "3", "--mlp_res_layers_hr", "1", "2", "3"]   # (as tests/test_gpu_mlp_shapes.py)
SHAPES = {"released": [], "s1": S1}
MODES = ("train", "eval")


def flags(name, more=()):
    w = ["--mlp1", "--mlp2", "--srweight", "--dispweight"]
    return common.FLAGS + SHAPES[name] + [x for k, v in zip(w, LOSS_WEIGHTS) for x in (k, str(v))] + list(more)


def inputs():
    """forward()'s arguments as numpy arrays: B images of H x H, N points per image and point set, binary labels."""
    return dict(
        images_lr=np.concatenate([weights.synthetic_image(H, seed=1 + b) for b in range(B)], 0),
        images_hr=prng.uniform("img_hr", 7, (B, 3, 2 * H, 2 * H), -1.0, 1.0).astype(np.float32),
        points_hr=np.stack([weights.synthetic_points(N, seed=30 + b) for b in range(B)]),
        points_lr=np.stack([weights.synthetic_points(N, seed=40 + b) for b in range(B)]),
        calibs=np.stack([common.CALIB] * B),
        labels_hr=(prng.uniform("lab_hr", 1, (B, 1, N), 0.0, 1.0) > 0.5).astype(np.float32),
        labels_lr=(prng.uniform("lab_lr", 1, (B, 1, N), 0.0, 1.0) > 0.5).astype(np.float32),
    )


def terms_f64(pred_lr, pred_hr, labels_lr, labels_hr, img_sr, images_hr, w=LOSS_WEIGHTS):
    """(terms [4], total) in float64 of predictions [S,B,N] and forward()'s label ARGUMENTS: forward hands labels_hr to query_mr -
    the lr predictions are held against them - and labels_lr to query_sr (lib/model/SuRSNet.py:249-250); the displacement term is
    MSE(stored labels_hr - stored labels_lr, preds_hr - preds_lr) = MSE(labels_lr - labels_hr arguments, ...), last stack."""
    pl, ph = np.asarray(pred_lr, np.float64), np.asarray(pred_hr, np.float64)
    for_lr = np.asarray(labels_hr, np.float64).reshape(pl.shape[1:])
    for_hr = np.asarray(labels_lr, np.float64).reshape(ph.shape[1:])
    e = np.array([np.mean([np.mean((p - for_lr) ** 2) for p in pl]),
                  np.mean([np.mean((p - for_hr) ** 2) for p in ph]),
                  np.mean(np.abs(np.asarray(img_sr, np.float64) - np.asarray(images_hr, np.float64))),
                  np.mean(((for_hr - for_lr) - (ph[-1] - pl[-1])) ** 2)])
    return e, float(np.dot(np.asarray(w, np.float64), e))
