"""Inputs, the float64 restatement and the fixture format of the classifier-gradient tests (tests/golden/mlp_grads_*.npz,
tools/gen_golden_grads.py).  Everything on the input side comes from seeds; a fixture holds the kept (kink-safe) point indices, the
reference's float64 gradients and the distance of its own float32 gradients from them.

The arithmetic (written from the formulas, stacks s < S, images b < B, M = B N):
    x_s(p)  = [bilinear sample of lr map s | bilinear sample of the hr map | z_feat] at the orthogonal projection of p
    q_s     = in_img_mr sigmoid(mlp_lr(x_s(points_mr)))            r_s = in_img_sr sigmoid(mlp_hr([x_s(points_sr) | q_s]))
    error   = w1 mean_s MSE(q_s, lab_lr) + w2 mean_s MSE(r_s, lab_hr) + wd MSE(lab_hr - lab_lr, r_{S-1} - q_{S-1})
with lab_lr / lab_hr the labels q / r are held against.  Index i of an image is KINK-SAFE when every hidden pre-activation of both
classifiers on every stack has |z| >= 1e-5 max(1, max |z| of that layer) and no projected x, y lies within 1e-4 of +-1."""
import os
from collections import OrderedDict

import numpy as np

import common
import forward_common as fc
from surs_amd import options, prng, weights

ZMUL, ZDIV = 1024 // 2, 200.0
LOSS_WEIGHTS = (fc.LOSS_WEIGHTS[0], fc.LOSS_WEIGHTS[1], fc.LOSS_WEIGHTS[3])     # mlp1, mlp2, dispweight
N_CAND = 16000
HL, HH = 16, 64
KINK_REL, EDGE = 1e-5, 1e-4
WHOLE, N_SAMPLES = 65536, 2048
FLOOR = 2.0 ** -22
CALIB_B = np.array([[1.7, 0.3, -0.2, 0.05], [0.25, -1.8, 0.15, -0.04], [0.1, 0.2, 1.9, 0.02], [0, 0, 0, 1]], np.float32)


def _dims(tag, dims):
    return ["--mlp_dim_" + tag] + [str(d) for d in dims]


def _res(tag, res):
    return ["--mlp_res_layers_" + tag] + [str(r) for r in res]


_ODD = [1000, 500, 250, 100]
# name -> (flags beyond common.FLAGS, S, B, N kept)
CASES = OrderedDict([
    ("released", ([], 3, 2, 3000)),
    ("odd", (_dims("lr", [321] + _ODD + [1]) + _dims("hr", [322] + _ODD + [1]), 1, 2, 1537)),
    ("res0", (_res("lr", [0, 2]) + _res("hr", [0, 2]), 2, 1, 777)),
    ("nores", (["--no_residual"], 2, 1, 777)),
    ("l1", (_dims("lr", [321, 1]) + _dims("hr", [322, 1]) + ["--no_residual"], 2, 1, 777)),
    ("mixed", (_dims("lr", [321, 512, 256, 128, 1]) + _res("lr", [1, 2, 3]) + _dims("hr", [322] + _ODD + [1]), 2, 1, 777)),
    ("d48", (["--hg_dim", "48"] + _dims("lr", [113] + _ODD + [1]) + _dims("hr", [114] + _ODD + [1]), 2, 1, 777)),
    ("tiny", (_dims("lr", [321, 64, 32, 1]) + _dims("hr", [322, 64, 32, 1]) + _res("lr", [1]) + _res("hr", [1]), 2, 2, 77)),
    ("tiny1", (_dims("lr", [321, 64, 32, 1]) + _dims("hr", [322, 64, 32, 1]) + _res("lr", [1]) + _res("hr", [1]), 2, 2, 1)),
])


def flags(name):
    return common.FLAGS + CASES[name][0]


def opt(name):
    return options.BaseOptions().parse(flags(name))


def fixture_path(golden_dir, name, part=""):
    return os.path.join(golden_dir, "mlp_grads_%s%s.npz" % (name, part))


def load_fixture(golden_dir, name):
    """A case's fixture as one dict: mlp_grads_<name>.npz, joined with mlp_grads_<name>_hr.npz (mlp_hr's quantities) where the
    generator had to split the case to keep every file below 1 MiB."""
    out = dict(np.load(fixture_path(golden_dir, name)))
    if os.path.exists(fixture_path(golden_dir, name, "_hr")):
        out.update(np.load(fixture_path(golden_dir, name, "_hr")))
    return out


def mlp_state(name):
    """The mlp_* entries of weights.synthetic_state_dict for the case's flags, float32 numpy."""
    sd = weights.synthetic_state_dict(opt(name), seed=0)
    return OrderedDict((k, v) for k, v in sd.items() if k.startswith("mlp_"))


def shapes_of(sd):
    """((dims, skip layers) lr, (dims, skip layers) hr) read off the weight tensors: the input width is hg_dim + 65 / + 66 with hg_dim
    a multiple of 16, or twice that with a skip at layer 0; any other skip layer l has dims[l] + dims[0] input channels."""
    out = []
    for m, p in enumerate(("mlp_lr.", "mlp_hr.")):
        L = 0
        while p + "conv%d.weight" % L in sd:
            L += 1
        cin0 = int(sd[p + "conv0.weight"].shape[1])
        c0 = cin0 if (cin0 - 65 - m) % 16 == 0 else cin0 // 2
        dims = [c0] + [int(sd[p + "conv%d.weight" % l].shape[0]) for l in range(L)]
        res = [l for l in range(L) if int(sd[p + "conv%d.weight" % l].shape[1]) == dims[l] + c0]
        assert all(int(sd[p + "conv%d.weight" % l].shape[1]) == dims[l] + (c0 if l in res else 0) for l in range(L)), p
        out.append((tuple(dims), tuple(res)))
    return tuple(out)


def inputs(name):
    """The candidate inputs of a case: lr maps [B][S] (D,16,16), hr maps [B] (64,64,64), candidate points_mr / points_sr [B,3,N_CAND],
    calibrations [B,4,4] of each point set, candidate labels [B,N_CAND] for q (lab_lr) and r (lab_hr)."""
    _, S, B, _ = CASES[name]
    D = opt(name).hg_dim
    tiny = name.startswith("tiny")
    return dict(
        feat_lr=[[prng.uniform("feat_lr", 3 + 7 * b + s, (D, HL, HL), -1.0, 1.0) for s in range(S)] for b in range(B)],
        feat_hr=[prng.uniform("feat_hr", 3 + 7 * b, (64, HH, HH), -1.0, 1.0) for b in range(B)],
        points_mr=np.stack([weights.synthetic_points(N_CAND, seed=30 + b) for b in range(B)]),
        points_sr=np.stack([weights.synthetic_points(N_CAND, seed=40 + b) for b in range(B)]),
        # (tiny: image 1's query_mr on a general calibration, its query_sr on the usual one - a swapped pair shows)
        calib_mr=np.stack([CALIB_B if (tiny and b == 1) else common.CALIB for b in range(B)]),
        calib_sr=np.stack([common.CALIB] * B),
        lab_lr=(prng.uniform("lab_hr", 1, (B, N_CAND), 0.0, 1.0) > 0.5).astype(np.float32),
        lab_hr=(prng.uniform("lab_lr", 1, (B, N_CAND), 0.0, 1.0) > 0.5).astype(np.float32),
    )


def kept(x, keep):
    """The inputs restricted to the kept indices keep [B,N]."""
    take = lambda a: np.stack([a[b][..., keep[b]] for b in range(len(keep))])
    return dict(x, points_mr=take(x["points_mr"]), points_sr=take(x["points_sr"]), lab_lr=take(x["lab_lr"]), lab_hr=take(x["lab_hr"]))


# ------------------------------------------------------------------ the float64 restatement
def project(points, calib):
    p = np.asarray(points, np.float64)
    c = np.asarray(calib, np.float64)
    return c[:3, :3] @ p + c[:3, 3:4]


def bilinear(fm, x, y):
    """[C,N]: grid_sample(align_corners=True, zeros padding) of fm [C,H,W] at x, y in [-1, 1] coordinates."""
    fm = np.asarray(fm, np.float64)
    H, W = fm.shape[1:]
    ix, iy = (x + 1.0) / 2.0 * (W - 1), (y + 1.0) / 2.0 * (H - 1)
    x0, y0 = np.floor(ix), np.floor(iy)
    out = np.zeros((fm.shape[0], x.shape[0]))
    for xx, yy, w in ((x0, y0, (x0 + 1 - ix) * (y0 + 1 - iy)), (x0 + 1, y0, (ix - x0) * (y0 + 1 - iy)),
                      (x0, y0 + 1, (x0 + 1 - ix) * (iy - y0)), (x0 + 1, y0 + 1, (ix - x0) * (iy - y0))):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        xi, yi = np.clip(xx, 0, W - 1).astype(np.int64), np.clip(yy, 0, H - 1).astype(np.int64)
        out += fm[:, yi, xi] * np.where(ok, w, 0.0)
    return out


def point_rows(feat_lr, feat_hr, points, calib):
    """([D + 65, N] input rows, in-image mask [N], (x, y))."""
    xyz = project(points, calib)
    x, y = xyz[0], xyz[1]
    mask = ((x >= -1.0) & (x <= 1.0) & (y >= -1.0) & (y <= 1.0)).astype(np.float64)
    return np.concatenate([bilinear(feat_lr, x, y), bilinear(feat_hr, x, y), xyz[2:3] * ZMUL / ZDIV]), mask, (x, y)


def _layers(sd, p):
    L = 0
    while p + "conv%d.weight" % L in sd:
        L += 1
    return ([np.asarray(sd[p + "conv%d.weight" % l], np.float64).reshape(sd[p + "conv%d.weight" % l].shape[0], -1) for l in range(L)],
            [np.asarray(sd[p + "conv%d.bias" % l], np.float64) for l in range(L)])


def mlp_forward(Ws, bs, res, X):
    """(logits [N], inputs of every layer, pre-activations of every layer)."""
    y, ins, zs = X, [], []
    for l, (W, b) in enumerate(zip(Ws, bs)):
        inp = np.concatenate([y, X]) if l in res else y
        z = W @ inp + b[:, None]
        ins.append(inp)
        zs.append(z)
        y = np.where(z > 0, z, 0.01 * z)
    return zs[-1][0], ins, zs


def mlp_backward(Ws, res, ins, zs, dlogit):
    """(dW list, db list, d error / d X [c0,N]) of d error / d logit [N]."""
    L = len(Ws)
    c0 = ins[0].shape[0] // (2 if 0 in res else 1)
    gW, gb = [None] * L, [None] * L
    dX = np.zeros((c0, dlogit.shape[0]))
    dz = dlogit[None]
    for l in range(L - 1, -1, -1):
        gW[l] = dz @ ins[l].T
        gb[l] = dz.sum(1)
        din = Ws[l].T @ dz
        if l in res:
            dX += din[-c0:]
            din = din[:-c0]
        if l == 0:
            dX += din
        else:
            dz = din * np.where(zs[l - 1] > 0, 1.0, 0.01)
    return gW, gb, dX


def grads_f64(sd, x, loss_weights=LOSS_WEIGHTS):
    """(grads, info) for mlp state dict sd and inputs x (as kept() returns them).  grads: OrderedDict key -> float64 array of the
    parameter's shape, in sd's key order; info: pred_lr / pred_hr [S,B,N], error (the three terms' weighted sum), margin [B,N] (the
    smallest |z| / max(1, layer max |z|) over the hidden units a point meets; inf without hidden layers), edge [B,N] (distance of the
    projected x, y from +-1)."""
    shapes = shapes_of(sd)
    nets = [(_layers(sd, p), set(shapes[m][1])) for m, p in enumerate(("mlp_lr.", "mlp_hr."))]
    B, S = len(x["feat_hr"]), len(x["feat_lr"][0])
    N = x["points_mr"].shape[2]
    M = B * N
    w1, w2, wd = loss_weights
    acc = [[np.zeros_like(W) for W in nets[m][0][0]] for m in range(2)], [[np.zeros_like(b) for b in nets[m][0][1]] for m in range(2)]
    pred = np.zeros((2, S, B, N))
    hidden = [[[] for _ in nets[m][0][0][:-1]] for m in range(2)]     # per classifier and hidden layer: (image, min |z| per point, max |z|)
    edge = np.zeros((B, N))
    error = 0.0
    for b in range(B):
        ll, lh = np.asarray(x["lab_lr"][b], np.float64), np.asarray(x["lab_hr"][b], np.float64)
        for s in range(S):
            (Wl, bl), rl = nets[0]
            (Wh, bh), rh_ = nets[1]
            Xl, mask_mr, xy_mr = point_rows(x["feat_lr"][b][s], x["feat_hr"][b], x["points_mr"][b], x["calib_mr"][b])
            Xs, mask_sr, xy_sr = point_rows(x["feat_lr"][b][s], x["feat_hr"][b], x["points_sr"][b], x["calib_sr"][b])
            edge[b] = np.min([np.abs(np.abs(v) - 1.0) for v in xy_mr + xy_sr], 0)
            lg_l, ins_l, zs_l = mlp_forward(Wl, bl, rl, Xl)
            sg_l = 1.0 / (1.0 + np.exp(-lg_l))
            q = mask_mr * sg_l
            Xh = np.concatenate([Xs, q[None]])
            lg_h, ins_h, zs_h = mlp_forward(Wh, bh, rh_, Xh)
            sg_h = 1.0 / (1.0 + np.exp(-lg_h))
            r = mask_sr * sg_h
            pred[0, s, b], pred[1, s, b] = q, r
            for m, zs in ((0, zs_l), (1, zs_h)):
                for l, z in enumerate(zs[:-1]):
                    hidden[m][l].append((b, np.abs(z).min(0), float(np.abs(z).max())))
            dr = w2 * 2.0 * (r - lh) / (S * M)
            dq = w1 * 2.0 * (q - ll) / (S * M)
            error += w1 * np.sum((q - ll) ** 2) / (S * M) + w2 * np.sum((r - lh) ** 2) / (S * M)
            if s == S - 1:
                d = (r - q) - (lh - ll)
                dr = dr + wd * 2.0 * d / M
                dq = dq - wd * 2.0 * d / M
                error += wd * np.sum(d ** 2) / M
            gW, gb, dX = mlp_backward(Wh, rh_, ins_h, zs_h, dr * mask_sr * sg_h * (1.0 - sg_h))
            for l in range(len(gW)):
                acc[0][1][l] += gW[l]
                acc[1][1][l] += gb[l]
            dq = dq + dX[-1]
            gW, gb, _ = mlp_backward(Wl, rl, ins_l, zs_l, dq * mask_mr * sg_l * (1.0 - sg_l))
            for l in range(len(gW)):
                acc[0][0][l] += gW[l]
                acc[1][0][l] += gb[l]
    margin = np.full((B, N), np.inf)
    for m in range(2):
        for blocks in hidden[m]:
            top = max(1.0, max(t for _, _, t in blocks))
            for b, low, _ in blocks:
                margin[b] = np.minimum(margin[b], low / top)
    grads = OrderedDict()
    for k in sd:
        m = 0 if k.startswith("mlp_lr.") else 1
        l = int(k.split("conv")[1].split(".")[0])
        grads[k] = acc[0][m][l][:, :, None] if k.endswith("weight") else acc[1][m][l]
    return grads, dict(pred_lr=pred[0], pred_hr=pred[1], error=error, margin=margin, edge=edge)


# ------------------------------------------------------------------ the fixture format
def quantities(key, g):
    """What a fixture stores of gradient tensor g: [(name, float64 array)] - the tensor itself below 65 536 elements, else its row
    sums, column sums and 2 048 elements at seeded indices."""
    g = np.asarray(g, np.float64)
    g2 = g.reshape(g.shape[0], -1)
    if g.size < WHOLE:
        return [(key + "|whole", g2.reshape(-1))]
    idx = np.minimum((prng.uniform01("grad_samples_" + key, 5, N_SAMPLES).astype(np.float64) * g.size).astype(np.int64), g.size - 1)
    return [(key + "|rows", g2.sum(1)), (key + "|cols", g2.sum(0)), (key + "|samples", g2.reshape(-1)[idx])]


def compare(gold, grads, factor=8.0, scale=1.0):
    """[(name, deviation relative to the reference's max-abs, bound)] of gradients `grads` against fixture `gold` for every stored
    quantity t: max |g / scale - g64| / max |g64| against factor * max(e_ref(t), 2^-22)."""
    out = []
    for key, g in grads.items():
        for name, got in quantities(key, np.asarray(g, np.float64) / scale):
            ref = gold[name]
            dev = float(np.abs(got - ref).max() / np.abs(ref).max())
            out.append((name, dev, factor * max(float(gold[name + "|e_ref"]), FLOOR)))
    return out
