"""What the fused classifier evaluator SHOULD compute: a numpy model (no GPU, no product code) of csrc/surs_mlp_fused.inc,
surs_mlp_fused_views.inc and surs_mlp_fused_stacks.inc (csrc/ = the package's csrc directory), written from their sources and the blob
layout of surs_mlp_generic.h.  It takes the weights from the state dict and rounds them itself (it never reads the blob), rounds the
activations where the kernels do and forms exactly the partial products they form; everything else is accumulation, which the model
runs either in float64 (the reference: the exact sum of the listed products) or in an fp32 accumulator that takes each product of
each 32-wide k-step as one addend, k-steps ascending or descending.  That second form measures what a summation order may change; it
does NOT model the inside of a v_mfma_f32_16x16x32 bit for bit.  tests/test_fused_model_host.py checks the model,
tests/test_gpu_fused_model.py holds the kernels to it.

What the sources state ("fused" = surs_mlp_fused.inc, "views" = surs_mlp_fused_views.inc, "gemm" = surs_gemm.inc, "pack" =
surs_pack.cpp, "query" = surs_query.hip):
  point      mlp_fused_body, fused:207-225: X, Y, Z = c3 + ((c0 x + c1 y) + c2 z) (query:95-97), the in-image mask on the fp32 X and Y
             (query:104-106), z_feat = fp32(fp32(Z zmul) / zdiv) (fused:215).
  features   the row [D lr | 64 hr | z_feat | p_lr | zeros up to gen_c0pad(D)] in fp32 (fused:222-224, :231): p_lr is 0 for the lr
             classifier and mask * sigmoid(logit_lr) as an fp32 value (fused:244-245), or the caller's p_lr (fused:216), for hr.  The
             gather is gc.bilinear in float64: the cases of tests/fused_cases.py are chosen so that every arithmetic gives the same
             features (tests/test_fused_model_host.py asserts it).
  parts      SplitKind<NP>::split (gemm:55-77), the blob images w1 / w2 / w3 (pack:335-339): NP = 1 f16(x); NP = 2 hi = f16(x),
             lo = f16(fp32(x - hi)); NP = 3 three bf16 parts, each the rounding of what the earlier ones left (query:147-156).  The
             activations are split from the fp32 value in LDS once per k-step in EVERY layer, the last included (fused:120-135): there
             is no fp32 fmaf tail here - which is where this model differs from column_model.points_one_product, whose layer 4 is an
             fp32 fmaf chain over unrounded operands.
  products   per k-step of 32 (fused_layers, fused:146-153), written (weight part, point part): NP = 1 (0,0); NP = 2 (1,0) (0,1)
             (0,0); NP = 3 (2,0) (1,1) (0,2) (1,0) (0,1) (0,0).
  k order    the k1pad rows of the previous layer's outputs (layer 0: the features) first, on a skip layer the k2pad = gen_c0pad(D)
             feature rows behind them (fused:117-118; pack:334); a skip at layer 0 reads the features twice.  Padded k and padded
             output rows are exact zeros (pack:320).
  epilogue   y = fp32(acc + bias); every layer but the last: y >= 0 ? y : fp32(y * 0.01f) (fused:172-173); the last layer's row 0 is
             the logit; occupancy = fp32(mask * fp32(sigmoid)) (fused:244, :259).
  views      mlp_fused_views_body: per view in view order layers 0 .. M (M = L / 2) on that view's own feature row, layer M's outputs
             (after its LeakyReLU unless M is the last layer) and the feature row - z_feat and p_lr included - summed in fp32 in view
             order (fused:175-177, views:109-117), times fp32(1 / V) (views:132-138, :236); layers M + 1 .. L - 1 once on the means; one
             logit per point, pred_v = mask_v * sigmoid (views:149); the hr row of view v holds mask_v * sigmoid(logit_lr)
             (views:100).  Those fp32 sums and products run in a known order: every form of the model keeps them, as it keeps the
             bias addition.
  stacks     surs_mlp_fused_stacks.inc runs mlp_fused_body per lr map: `single` on that map.

Every function returns {"logit_lr", "occ_lr", "logit_hr", "occ_hr", "mask"} and takes acc (np.float64 / np.float32), order ("asc" /
"desc"), rounding (False: every rounding point is the identity - the model is then the classifier itself) and pert (a wrong model,
for tests/test_fused_model_host.py's separation test):
    {"trunc_act": True}        (a) the first part of every activation converted towards zero
    {"drop_kstep": (m, l)}     (b) the last k-step of layer l's k1 segment missing in classifier m
    {"swap_skip": True}        (c) the z_feat and p_lr rows of every skip segment swapped
    {"bias16": (m, l)}         (d) layer l's bias of classifier m through the 16-bit type
    {"drop_products": [...]}   (e) the listed (weight part, point part) products not formed
    {"sum_pre_lrelu": True}    (f) views: layer M's outputs summed before their LeakyReLU (which then acts on the mean)
    {"plr_unmasked": True}     (g) views: the hr row's p_lr without the view's mask
A change to a rounding point or to the product order of fused_layers must change this file in the same commit."""
import numpy as np

import grad_common as gc
from column_model import FACTOR, Rounding, bounds, breaks, gemm, sigmoid

KT = 32                                               # GEN_KT: k per MFMA step
C_HR = 64                                             # GEN_C_HR
PRODUCTS = {1: [(0, 0)], 2: [(1, 0), (0, 1), (0, 0)], 3: [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]}
LOGIT_FLOOR = 2.0 ** -22                              # of the largest |logit|: the project's floor for logits straight from the library


def pad32(v):
    return (v + KT - 1) // KT * KT


def c0pad(D):
    """gen_c0pad (surs_mlp_generic.h:56)."""
    return pad32(D + C_HR + 2)


class Net:
    """One classifier's tensors as float64 (of fp32 values): W[l] [out, in], b[l], dims, skip layers."""

    def __init__(self, sd, m):
        self.m = m
        self.W, self.b = gc._layers(sd, "mlp_hr." if m else "mlp_lr.")
        self.dims, self.res = gc.shapes_of(sd)[m]
        self.L = len(self.W)
        self.D = gc.shapes_of(sd)[0][0][0] - C_HR - 1


def _rounding(NP, rounding, pert):
    assert NP in (1, 2, 3)
    return Rounding("bf16" if NP == 3 else "fp16", rounding, trunc_act=bool(pert.get("trunc_act")))


def parts(R, NP, x, act):
    """The NP 16-bit parts of fp32 values x; act: an activation (the B operand), whose first conversion perturbation (a) breaks."""
    x = np.asarray(x, np.float64)
    if not R.on:
        return [x]
    out = [R.act(x) if act else R.h(x)]
    r = x
    for _ in range(NP - 1):
        r = R.f(r - out[-1])
        out.append(R.h(r))
    return out


# ------------------------------------------------------------------ the point and its feature row
def project(R, points, calib):
    """(X, Y, Z) of points [3, N] under calib (12 values, rows 0 .. 2): c3 + ((c0 x + c1 y) + c2 z) in fp32 (query:95-97)."""
    c = np.asarray(calib, np.float64).reshape(-1)[:12]
    p = R.f(points)
    return [R.f(c[4 * i + 3] + R.f(R.f(R.f(c[4 * i] * p[0]) + R.f(c[4 * i + 1] * p[1])) + R.f(c[4 * i + 2] * p[2]))) for i in range(3)]


def feature_rows(R, points, calib, zmul, zdiv, feat_lr, feat_hr):
    """(F [gen_c0pad(D), N]: D lr, 64 hr, z_feat, a zero p_lr slot, zeros; mask [N])."""
    X, Y, Z = project(R, points, calib)
    mask = ((X >= -1.0) & (X <= 1.0) & (Y >= -1.0) & (Y <= 1.0)).astype(np.float64)
    D = np.shape(feat_lr)[0]
    F = np.zeros((c0pad(D), X.shape[0]))
    F[:D] = R.f(gc.bilinear(feat_lr, X, Y))
    F[D:D + C_HR] = R.f(gc.bilinear(feat_hr, X, Y))
    F[D + C_HR] = R.f(R.f(Z * float(zmul)) / float(zdiv))
    return F, mask


# ------------------------------------------------------------------ one layer
def layer(R, NP, net, l, y, F, acc, order, pert, lrelu=True):
    """Layer l of net on the previous outputs y [dims[l], N] (layer 0: the feature rows F themselves) and, on a skip layer, the
    feature rows F [gen_c0pad(D), N] behind them.  Returns [dims[l + 1], N] fp32 values (the padded rows, exact zeros, left out)."""
    W, b = net.W[l], net.b[l]
    k1, c0, cp = net.dims[l], net.dims[0], F.shape[0]
    k1p, res = pad32(k1), l in net.res
    assert W.shape[1] == k1 + (c0 if res else 0) and (l > 0 or k1p == cp)
    Wi = np.zeros((W.shape[0], k1p + (cp if res else 0)))
    Wi[:, :k1] = W[:, :k1]
    X = np.zeros((Wi.shape[1], y.shape[1]))
    X[:y.shape[0]] = y
    if res:
        Wi[:, k1p:k1p + c0] = W[:, k1:]                                  # the feature part starts at k1pad (pack:334)
        X[k1p:] = F
        if pert.get("swap_skip"):                                        # (c)
            cg = net.D + C_HR
            X[[k1p + cg, k1p + cg + 1]] = X[[k1p + cg + 1, k1p + cg]]
    if pert.get("drop_kstep") == (net.m, l):                             # (b)
        X[k1p - KT:k1p] = 0.0
    wp, xp = parts(R, NP, Wi, False), parts(R, NP, X, True)
    pairs = [q for q in PRODUCTS[NP] if q not in pert.get("drop_products", ())] if R.on else [(0, 0)]
    a = gemm([(wp[i], xp[j]) for i, j in pairs], acc, order, kstep=KT)
    if pert.get("bias16") == (net.m, l):                                 # (d)
        b = R.h(b)
    t = R.f(a + b[:, None])
    if l == net.L - 1 or not lrelu:
        return t
    return lrelu01(R, t)


def lrelu01(R, t):
    """y >= 0 ? y : y * 0.01f (fused:173)."""
    return np.where(t >= 0.0, t, R.f(t * R.c01))


def occupancy(R, mask, logit):
    """mask * (1 / (1 + expf(-l))) (fused:244, :259)."""
    return R.f(mask * R.f(sigmoid(logit)))


def _with_plr(F, D, p):
    F = F.copy()
    F[D + C_HR + 1] = p
    return F


# ------------------------------------------------------------------ mlp_fused_body
def single(sd, NP, points, calib, zmul, zdiv, feat_lr, feat_hr, p_lr=None, acc=np.float64, order="asc", rounding=True, pert=None):
    """surs_query_points_generic on points [3, N]; p_lr [N] given: the hr classifier alone (logit_lr is None, occ_lr is p_lr)."""
    pert = dict(pert or {})
    R = _rounding(NP, rounding, pert)
    F, mask = feature_rows(R, points, calib, zmul, zdiv, feat_lr, feat_hr)
    D = np.shape(feat_lr)[0]
    out = {"mask": mask, "logit_lr": None, "occ_lr": None if p_lr is None else R.f(p_lr)}
    for m, tag in ((0, "lr"), (1, "hr")):
        if m == 0 and p_lr is not None:
            continue
        net = Net(sd, m)
        assert net.D == D
        Fm = _with_plr(F, D, out["occ_lr"] if m else 0.0)
        y = Fm
        for l in range(net.L):
            y = layer(R, NP, net, l, y, Fm, acc, order, pert)
        out["logit_" + tag], out["occ_" + tag] = y[0], occupancy(R, mask, y[0])
    return out


def stacks(sd, NP, points, calib, zmul, zdiv, feats_lr, feat_hr, **kw):
    """surs_query_points_generic_stacks: `single` per lr map."""
    return [single(sd, NP, points, calib, zmul, zdiv, f, feat_hr, **kw) for f in feats_lr]


# ------------------------------------------------------------------ mlp_fused_views_body
def views(sd, NP, points, calibs, zmul, zdiv, feats_lr, feats_hr, p_lr=None, acc=np.float64, order="asc", rounding=True, pert=None):
    """surs_query_points_generic_views: points [V, 3, N], calibs [V, 12], feature maps [V][...]; p_lr [V, N] given: hr alone.
    logit_* [N], occ_* and mask [V, N]."""
    pert = dict(pert or {})
    R = _rounding(NP, rounding, pert)
    V = len(points)
    D = np.shape(feats_lr[0])[0]
    rows = [feature_rows(R, points[v], calibs[v], zmul, zdiv, feats_lr[v], feats_hr[v]) for v in range(V)]
    mask = np.stack([r[1] for r in rows])
    inv = R.f(1.0 / V)
    out = {"mask": mask, "logit_lr": None, "occ_lr": None if p_lr is None else R.f(p_lr)}
    sprob = None
    for m, tag in ((0, "lr"), (1, "hr")):
        if m == 0 and p_lr is not None:
            continue
        net = Net(sd, m)
        M = net.L // 2
        fsum = vsum = None
        for v in range(V):
            if m == 0:
                pl = 0.0
            elif p_lr is not None:
                pl = out["occ_lr"][v]
            else:
                pl = sprob if pert.get("plr_unmasked") else R.f(mask[v] * sprob)                 # in * sprob (views:100); (g)
            Fm = _with_plr(rows[v][0], D, pl)
            y = Fm
            for l in range(M + 1):
                y = layer(R, NP, net, l, y, Fm, acc, order, pert, lrelu=not (l == M and pert.get("sum_pre_lrelu")))
            fsum = Fm if v == 0 else R.f(fsum + Fm)
            vsum = y if v == 0 else R.f(vsum + y)
        Fmean, y = R.f(fsum * inv), R.f(vsum * inv)
        if pert.get("sum_pre_lrelu") and M < net.L - 1:                                           # (f)
            y = lrelu01(R, y)
        for l in range(M + 1, net.L):
            y = layer(R, NP, net, l, y, Fmean, acc, order, pert)
        sprob = R.f(sigmoid(y[0]))
        out["logit_" + tag], out["occ_" + tag] = y[0], R.f(mask * sprob[None])
    return out


# ------------------------------------------------------------------ the bound
def logit_bounds(ref, forms, tag, sel=None):
    """column_model.bounds for logits straight from the library: over the points sel (all of them unless given), e = the larger
    deviation of the two fp32-accumulating forms from the float64 model, floor = 2^-22 max |logit|; bound[s] = FACTOR max(s(e),
    s(floor)) for s = mean, max, median.  Returns (bound, e, sel)."""
    want = ref["logit_" + tag]
    sel = np.ones(want.shape, bool) if sel is None else sel
    floor = np.full(int(sel.sum()), LOGIT_FLOOR * np.abs(want[sel]).max())
    bound, e = bounds(ref, forms, tag, sel, floor)
    return bound, e, sel
