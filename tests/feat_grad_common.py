"""Inputs, the float64 restatement and the fixture format of the feature-map gradient tests (tests/golden/feat_grads_*.npz,
tools/gen_golden_feat_grads.py): d error / d (every lr map, the hr map) of the loss grad_common states, i.e. the d error / d X that
grad_common.mlp_backward returns for both classifiers, scattered through grad_common.bilinear's four taps (the transpose of the
gather).  mlp_lr's rows were sampled at points_mr, mlp_hr's at points_sr; columns [0, D) belong to the stack's lr map, [D, D + 64) to
the hr map, z and q to no map.

The maps are NOT square and differ between lr and hr (every grad_common case is 16^2 / 64^2, where an h / w swap goes unseen).
Everything on the input side comes from seeds; a fixture holds the kept (kink-safe, grad_common's definition) indices, the
reference's float64 map gradients - whole: every map here has fewer than 65 536 elements - and per tensor e_ref = max |fp32 - fp64|
/ max |fp64| of the reference's own float32 run."""
import os
from collections import OrderedDict

import numpy as np

import common
import grad_common as gc
from surs_amd import prng, weights

CHUNK = 2048       # points per chunk of the library's gradient pass (include/surs.h)
# name -> (S, B, N kept, lr map (h, w), hr map (h, w)); the classifier flags are grad_common's case of the same name
CASES = OrderedDict([
    ("d48", (2, 1, 2125, (12, 20), (24, 40))),      # two chunks: 2048 + 77
    ("tiny", (2, 2, 77, (5, 7), (9, 6))),           # image 1's points_mr on another calibration than its points_sr
    ("res0", (1, 1, 300, (5, 7), (9, 6))),          # a skip at layer 0 (both halves of the doubled input) and at layer 2
])
# d48's candidates leave x > 0.7 and y < -0.7 of the image empty (points in [-0.55, 0.35]^3 under diag(2, -2, 2)), so that some hr
# pixels receive nothing; the other cases cover [-1.1, 1.1]^2 as grad_common's do
POINT_RANGE = {"d48": (-0.55, 0.35)}


def opt(name):
    return gc.opt(name)


def fixture_path(golden_dir, name):
    return os.path.join(golden_dir, "feat_grads_%s.npz" % name)


def load_fixture(golden_dir, name):
    return dict(np.load(fixture_path(golden_dir, name)))


def tensor_names(name):
    """The stored tensors: lr0 .. lr{S-1} [B,D,hl,wl], hr [B,64,hh,wh]."""
    return ["lr%d" % s for s in range(CASES[name][0])] + ["hr"]


def inputs(name):
    """grad_common.inputs with this module's map sizes, stack count and (d48) point range."""
    S, B, _, (hl, wl), (hh, wh) = CASES[name]
    D = opt(name).hg_dim
    lo, hi = POINT_RANGE.get(name, (-0.55, 0.55))
    return dict(
        feat_lr=[[prng.uniform("feat_lr", 3 + 7 * b + s, (D, hl, wl), -1.0, 1.0) for s in range(S)] for b in range(B)],
        feat_hr=[prng.uniform("feat_hr", 3 + 7 * b, (64, hh, wh), -1.0, 1.0) for b in range(B)],
        points_mr=np.stack([weights.synthetic_points(gc.N_CAND, seed=30 + b, lo=lo, hi=hi) for b in range(B)]),
        points_sr=np.stack([weights.synthetic_points(gc.N_CAND, seed=40 + b, lo=lo, hi=hi) for b in range(B)]),
        calib_mr=np.stack([gc.CALIB_B if (name == "tiny" and b == 1) else common.CALIB for b in range(B)]),
        calib_sr=np.stack([common.CALIB] * B),
        lab_lr=(prng.uniform("lab_hr", 1, (B, gc.N_CAND), 0.0, 1.0) > 0.5).astype(np.float32),
        lab_hr=(prng.uniform("lab_lr", 1, (B, gc.N_CAND), 0.0, 1.0) > 0.5).astype(np.float32),
    )


def kept_inputs(golden_dir, name):
    gold = load_fixture(golden_dir, name)
    return gold, gc.kept(inputs(name), gold["keep"])


# ------------------------------------------------------------------ the float64 restatement
def taps(H, W, x, y):
    """grad_common.bilinear's four taps of points x, y [N] on an H x W map: [(flat pixel index [N] (clamped), weight [N] - 0 where
    the tap lies outside the map -, inside [N] bool)] in the order (x0, y0), (x1, y0), (x0, y1), (x1, y1)."""
    ix, iy = (x + 1.0) / 2.0 * (W - 1), (y + 1.0) / 2.0 * (H - 1)
    x0, y0 = np.floor(ix), np.floor(iy)
    out = []
    for xx, yy, w in ((x0, y0, (x0 + 1 - ix) * (y0 + 1 - iy)), (x0 + 1, y0, (ix - x0) * (y0 + 1 - iy)),
                      (x0, y0 + 1, (x0 + 1 - ix) * (iy - y0)), (x0 + 1, y0 + 1, (ix - x0) * (iy - y0))):
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        xi, yi = np.clip(xx, 0, W - 1).astype(np.int64), np.clip(yy, 0, H - 1).astype(np.int64)
        out.append((yi * W + xi, np.where(ok, w, 0.0), ok))
    return out


def scatter(C, H, W, x, y, d):
    """[C,H,W]: the transpose of grad_common.bilinear - d [C,N] = d error / d (the sampled values) added to the four taps' pixels."""
    g = np.zeros((C, H * W))
    for pix, w, _ in taps(H, W, x, y):
        np.add.at(g, (slice(None), pix), d * w)        # (w = 0 where the tap lies outside: the clamped pixel receives 0)
    return g.reshape(C, H, W)


def map_grads_f64(sd, x, loss_weights=gc.LOSS_WEIGHTS):
    """(g_lr: list of S arrays [B,D,hl,wl], g_hr [B,64,hh,wh], error) in float64 for mlp state dict sd and inputs x: the loop of
    grad_common.grads_f64 with the input gradients kept instead of the parameters'."""
    shapes = gc.shapes_of(sd)
    nets = [(gc._layers(sd, p), set(shapes[m][1])) for m, p in enumerate(("mlp_lr.", "mlp_hr."))]
    B, S = len(x["feat_hr"]), len(x["feat_lr"][0])
    N = x["points_mr"].shape[2]
    M = B * N
    w1, w2, wd = loss_weights
    D, hl, wl = x["feat_lr"][0][0].shape
    _, hh, wh = x["feat_hr"][0].shape
    g_lr, g_hr = [np.zeros((B, D, hl, wl)) for _ in range(S)], np.zeros((B, 64, hh, wh))
    error = 0.0
    for b in range(B):
        ll, lh = np.asarray(x["lab_lr"][b], np.float64), np.asarray(x["lab_hr"][b], np.float64)
        for s in range(S):
            (Wl, bl), rl = nets[0]
            (Wh, bh), rh = nets[1]
            Xl, mask_mr, xy_mr = gc.point_rows(x["feat_lr"][b][s], x["feat_hr"][b], x["points_mr"][b], x["calib_mr"][b])
            Xs, mask_sr, xy_sr = gc.point_rows(x["feat_lr"][b][s], x["feat_hr"][b], x["points_sr"][b], x["calib_sr"][b])
            lg_l, ins_l, zs_l = gc.mlp_forward(Wl, bl, rl, Xl)
            sg_l = 1.0 / (1.0 + np.exp(-lg_l))
            q = mask_mr * sg_l
            lg_h, ins_h, zs_h = gc.mlp_forward(Wh, bh, rh, np.concatenate([Xs, q[None]]))
            sg_h = 1.0 / (1.0 + np.exp(-lg_h))
            r = mask_sr * sg_h
            dr = w2 * 2.0 * (r - lh) / (S * M)
            dq = w1 * 2.0 * (q - ll) / (S * M)
            error += w1 * np.sum((q - ll) ** 2) / (S * M) + w2 * np.sum((r - lh) ** 2) / (S * M)
            if s == S - 1:
                d = (r - q) - (lh - ll)
                dr = dr + wd * 2.0 * d / M
                dq = dq - wd * 2.0 * d / M
                error += wd * np.sum(d ** 2) / M
            _, _, dXh = gc.mlp_backward(Wh, rh, ins_h, zs_h, dr * mask_sr * sg_h * (1.0 - sg_h))
            _, _, dXl = gc.mlp_backward(Wl, rl, ins_l, zs_l, (dq + dXh[-1]) * mask_mr * sg_l * (1.0 - sg_l))
            for dX, (px, py) in ((dXh, xy_sr), (dXl, xy_mr)):
                g_lr[s][b] += scatter(D, hl, wl, px, py, dX[:D])
                g_hr[b] += scatter(64, hh, wh, px, py, dX[D:D + 64])
    return g_lr, g_hr, error


def named(g_lr, g_hr):
    return OrderedDict([("lr%d" % s, g) for s, g in enumerate(g_lr)] + [("hr", g_hr)])


# ------------------------------------------------------------------ what the point sets must exercise
def coverage(name, x):
    """Counts on kept inputs x: hr pixels that receive no tap at all (`hr_empty`), the largest number of taps one lr pixel receives
    from one point set within one chunk (`lr_max_taps`), lr + hr pixels that receive taps from more than one chunk of one point set
    (`across_chunks`), image 0."""
    _, _, N, (hl, wl), (hh, wh) = CASES[name]
    hr_hit = np.zeros(hh * wh, bool)
    lr_max, across = 0, 0
    for pts, cal in ((x["points_mr"][0], x["calib_mr"][0]), (x["points_sr"][0], x["calib_sr"][0])):
        xyz = gc.project(pts, cal)
        for H, W, is_hr in ((hl, wl, False), (hh, wh, True)):
            per_chunk = np.zeros(((N + CHUNK - 1) // CHUNK, H * W), np.int64)
            for pix, _, ok in taps(H, W, xyz[0], xyz[1]):
                for p in np.nonzero(ok)[0]:
                    per_chunk[p // CHUNK, pix[p]] += 1
            if is_hr:
                hr_hit |= per_chunk.sum(0) > 0
            else:
                lr_max = max(lr_max, int(per_chunk.max()))
            across += int(((per_chunk > 0).sum(0) > 1).sum())
    return dict(hr_empty=int((~hr_hit).sum()), lr_max_taps=lr_max, across_chunks=across)


def check_coverage(name, cov):
    if name == "d48":
        assert cov["hr_empty"] >= 1 and cov["lr_max_taps"] >= 8 and cov["across_chunks"] >= 1, cov


# ------------------------------------------------------------------ the fixture format and the parity bound
def compare(gold, got, factor=8.0, scale=1.0):
    """[(tensor name, max |g / scale - g64| / max |g64|, factor * max(e_ref, 2^-22))] for got: name -> array of the stored shape."""
    out = []
    for k, g in got.items():
        ref = gold[k]
        dev = float(np.abs(np.asarray(g, np.float64) / scale - ref).max() / np.abs(ref).max())
        out.append((k, dev, factor * max(float(gold[k + "|e_ref"]), gc.FLOOR)))
    return out
