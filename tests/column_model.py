"""What the reduced-precision classifiers SHOULD compute: a numpy model (no GPU, no product code) of the bf16 / fp16 column kernels
and of the one-product point path, written from the kernels' sources.  It rounds to 16 bits exactly where the sources do and forms
exactly the partial products they form; everything else is accumulation, which the model runs either in float64 (the reference) or
in fp32 by k-steps of 16 in ascending or descending k order (the measure of what a summation order may change).  A correct kernel
differs from the float64 model by accumulation order only - and by the rare activation that this order pushes across a 16-bit
rounding boundary.  tests/test_column_model_host.py checks the model, tests/test_gpu_column_model.py holds the kernels to it.

    dense               column kernel 3            csrc/surs_grid_v3.inc
    restated            column kernels 10 and 12   csrc/surs_grid_restated.inc, surs_grid_v10.inc (12 reproduces 10's bits)
    points_one_product  the point path inside native.reduced_point_operands()   csrc/surs_gemm.inc, run_points_fp32

(csrc/ = the package's csrc directory; "query" below = csrc/surs_query.hip, "pack" = csrc/surs_pack.cpp.)  Every function returns
{"logit_lr", "occ_lr", "logit_hr", "occ_hr", "mask"}; the hr classifier is fed the model's own lr occupancy.  A change to a
rounding point of the kernels must change this file in the same commit."""
import numpy as np

import grad_common as gc

D1, D2, D3, D4, C_G = 1024, 512, 256, 128, 320
RES = (2, 3, 4)                                       # the skip layers of the released classifiers
B1FRAG_SCALE = {"bf16": 1.0, "fp16": 4096.0}          # csrc/surs_mlp_layout.h:42


# ------------------------------------------------------------------ the number formats
def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even) as float32, by integer arithmetic on the bits (pack:14-20)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    r = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    r = np.where(nan, (u & np.uint32(0xffff0000)) | np.uint32(0x00400000), r)
    return r.astype(np.uint32).view(np.float32)


def bf16_truncate(x):
    """float32 -> bf16 by dropping the low 16 bits: the WRONG conversion of perturbation (a)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (u & np.uint32(0xffff0000)).view(np.float32)


def f16_truncate(x):
    """float32 -> f16 towards zero (perturbation (a) on the fp16 kernels)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float32)


class Rounding:
    """The rounding points.  on=False makes every one of them the identity (the model is then the classifier itself)."""

    def __init__(self, prec, on=True, trunc_act=False):
        assert prec in ("bf16", "fp16")
        self.prec, self.on, self.trunc_act = prec, on, trunc_act
        self.c01 = float(np.float32(0.01)) if on else 0.01                       # 0.01f
        self.k99 = float(np.float32(1.0) - np.float32(0.01)) if on else 0.99     # 1.0f - 0.01f (surs_grid_v10.inc:262)

    def f(self, x):
        """An fp32 value."""
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float64) if self.on else np.asarray(x, np.float64)

    def fma(self, a, b, c):
        """fmaf on fp32 operands (their product is exact in float64)."""
        return self.f(np.asarray(a, np.float64) * b + c)

    def f16(self, x):
        if not self.on:
            return np.asarray(x, np.float64)
        with np.errstate(over="ignore"):
            return np.asarray(x, np.float64).astype(np.float32).astype(np.float16).astype(np.float64)

    def h(self, x):
        """The kernel's 16-bit type, round to nearest even: weights, operand parts."""
        if not self.on:
            return np.asarray(x, np.float64)
        if self.prec == "fp16":
            return self.f16(x)
        return bf16_round(np.asarray(x, np.float64).astype(np.float32)).astype(np.float64)

    def act(self, x):
        """The kernel's 16-bit type for an ACTIVATION (the conversion perturbation (a) breaks)."""
        if not (self.on and self.trunc_act):
            return self.h(x)
        x32 = np.asarray(x, np.float64).astype(np.float32)
        return (bf16_truncate(x32) if self.prec == "bf16" else f16_truncate(x32)).astype(np.float64)

    def lrelu01(self, x):
        """max(x, 0.01f * x) with the product an fp32 value (query:592-593)."""
        return np.maximum(x, self.f(self.c01 * x))

    def split3(self, x):
        """split3_elem (surs_grid_restated.inc:49-57): three 16-bit parts, each the rounding of what the earlier ones left."""
        if not self.on:
            x = np.asarray(x, np.float64)
            return [x, np.zeros_like(x), np.zeros_like(x)]
        p0 = self.h(x)
        r = self.f(x - p0)
        p1 = self.h(r)
        r = self.f(r - p1)
        return [p0, p1, self.h(r)]

    def split2_f16(self, x):
        """SplitKind<2>::split (surs_gemm.inc:70-76) / split2_f16 (pack:44-47): hi = f16(x), lo = f16(x - hi)."""
        if not self.on:
            return [np.asarray(x, np.float64), 0.0]
        hi = self.f16(x)
        return [hi, self.f16(self.f(x - hi))]


# ------------------------------------------------------------------ accumulation
def gemm(products, acc, order, init=None, kstep=16):
    """sum over k of the listed products: products = [(W [M,K], X [K,N]), ...], all added into one accumulator k-step by k-step
    in the listed order (an MFMA each).  acc = np.float64: the exact sum (to float64).  acc = np.float32: an fp32 accumulator
    that takes every k-step of `kstep` (16: the 32x32x16 MFMA of the column kernels and the layer GEMM; tests/fused_model.py passes
    the fused evaluator's 32) as one addend, k-steps ascending (order "asc") or descending ("desc")."""
    K = products[0][0].shape[1]
    if acc is np.float64:
        out = 0.0 if init is None else np.asarray(init, np.float64)
        for W, X in products:
            out = out + W @ X
        return out
    assert acc is np.float32 and order in ("asc", "desc")
    M, N = products[0][0].shape[0], products[0][1].shape[1]
    a = np.zeros((M, N), np.float32) if init is None else np.array(np.broadcast_to(init, (M, N)), np.float32)
    steps = list(range(0, K, kstep))
    for s in (steps if order == "asc" else steps[::-1]):
        for W, X in products:
            a += (W[:, s:s + kstep] @ X[s:s + kstep]).astype(np.float32)
    return a.astype(np.float64)


def _pad16(W, X):
    k = W.shape[1]
    if k % 16 == 0:
        return W, X
    pad = 16 - k % 16
    return np.pad(W, ((0, 0), (0, pad))), np.pad(X, ((0, pad), (0, 0)))


def gemm_split2(R, W, X, acc, order):
    """The fp32-grade layer GEMM on two f16 parts per operand (gemm_x3g_kernel<.., NP = 2>): per k-step the products lo x hi,
    hi x lo (phase 1, surs_gemm.inc:202-210) and hi x hi (phase 2, :221); lo x lo is not formed.  Result: an fp32 value."""
    if not R.on:
        return W @ X
    W, X = _pad16(W, X)
    (wh, wl), (xh, xl) = R.split2_f16(W), R.split2_f16(X)
    return R.f(gemm([(wl, xh), (wh, xl), (wh, xh)], acc, order))


def sigmoid(l):
    return 1.0 / (1.0 + np.exp(-l))


# ------------------------------------------------------------------ weights
class Mlp:
    """One classifier's tensors as float64 (of fp32 values): W[l] [out, in], b[l]."""

    def __init__(self, sd, m):
        self.m = m
        self.W, self.b = gc._layers(sd, "mlp_hr." if m else "mlp_lr.")
        assert [w.shape[0] for w in self.W] == [D1, D2, D3, D4, 1] and self.W[0].shape[1] == C_G + 1 + m
        self.wz = [self.W[0][:, C_G], None, self.W[2][:, D2 + C_G], self.W[3][:, D3 + C_G], self.W[4][:, D4 + C_G]]
        z1 = np.zeros(D1)
        self.wp = ([self.W[0][:, C_G + 1], None, self.W[2][:, D2 + C_G + 1], self.W[3][:, D3 + C_G + 1], self.W[4][:, D4 + C_G + 1]]
                   if m else [z1, None, np.zeros(D3), np.zeros(D4), np.zeros(1)])
        # feature columns of the skip layers and of layer 0: what the column constants are made of (pack:93-111)
        self.wf = [self.W[0][:, :C_G], None, self.W[2][:, D2:D2 + C_G], self.W[3][:, D3:D3 + C_G], self.W[4][:, D4:D4 + C_G]]


# ------------------------------------------------------------------ geometry of a sweep
def sweep_geometry(R, mat, calib, cols, rz, zmul, zdiv, feat_lr, feat_hr):
    """cols: [C, 2] (i, j) grid indices.  Returns (feats [320, C] fp32 values, mask [C], zf [rz], zmid) as the sweep forms them:
    the column's point at k = 0 in float64, stored as float32 (make_point, query:85-88), projected (query:95-97; exact for the
    calibrations the column kernels accept with power-of-two scales), sampled as tests/grad_common.py's point_rows does; the
    depth feature per voxel from (float)(dz k + z0) (surs_grid_v10.inc:522-526), zmid at k = rz / 2 (query:1278-1279, :1570)."""
    mat = np.asarray(mat, np.float64).reshape(3, 4)
    cal4 = np.eye(4)
    cal4[:3] = np.asarray(calib, np.float64).reshape(-1)[:12].reshape(3, 4)
    ij = np.asarray(cols, np.float64).T
    pts = mat[:, :1] * ij[0] + mat[:, 1:2] * ij[1] + mat[:, 3:4]
    pts = R.f(pts)
    rows, mask, _ = gc.point_rows(feat_lr, feat_hr, pts, cal4)
    c22, c23 = cal4[2, 2], cal4[2, 3]

    def zf_of(k):
        zw = R.f(mat[2, 2] * np.asarray(k, np.float64) + mat[2, 3])
        Z = R.f(c23 + R.f(c22 * zw))
        return R.f(R.f(Z * zmul) / zdiv)
    return R.f(rows[:C_G]), mask, zf_of(np.arange(rz)), float(zf_of(rz // 2)), zf_of


def column_constants(R, net, feats, acc, order):
    """a0 [1024, C], a2 [256, C], a3 [128, C], a4 [1, C]: W_l[:, features] f + b_l on the fp32-grade layer GEMM (column_constants,
    query:1077-1091; bias added to the fp32 accumulator, surs_gemm.inc:274-278)."""
    return {l: R.f(gemm_split2(R, net.wf[l], feats, acc, order) + net.b[l][:, None]) for l in (0, 2, 3, 4)}


# ------------------------------------------------------------------ layers 2 - 4 and the output, shared by kernels 3, 10, 12
def _tail(R, net, cc, zf, p, acc1, acc, order):
    """acc1 [512, C, rz]: layer 1's accumulators.  surs_grid_v3.inc:296-461 / surs_grid_v10.inc:342-500."""
    C, rz = p.shape
    N = C * rz
    y = R.act(R.lrelu01(acc1)).reshape(D2, N)                       # cvt8: LeakyReLU in fp32, then the 16-bit type
    for l, dk in ((2, D2), (3, D3)):
        init = R.fma(zf[None, None, :], net.wz[l][:, None, None], cc[l][:, :, None])          # a_l + w_lz zf   (v3.inc:345)
        if net.m:
            init = R.fma(p[None], net.wp[l][:, None, None], init)                               # + w_lp p        (v3.inc:346)
        a = gemm([(R.h(net.W[l][:, :dk]), y)], acc, order, init.reshape(-1, N))                # 16-bit core (pack:156-174)
        y = R.lrelu01(a)
        if l == 2:
            y = R.act(y)                                                                        # y2 (v3.inc:400)
    s = gemm([(net.W[4][:, :D4], y)], acc, order)                   # layer 4 in fp32: fp32 weights, fp32 LeakyReLU(acc3) (v3.inc:446)
    y4 = R.fma(zf[None, :], net.wz[4][0], cc[4][0][:, None])        # v3.inc:458
    if net.m:
        y4 = R.fma(p, net.wp[4][0], y4)
    return R.f(y4 + s.reshape(C, rz))                               # v3.inc:460


def _occupancy(R, mask, logit):
    """cmask * (1 / (1 + expf(-l))) (surs_grid_v3.inc:508)."""
    return R.f(mask[:, None] * R.f(sigmoid(logit)))


def _sweep(layer1, sd, prec, geom, acc, order, rounding, pert):
    pert = dict(pert or {})
    R = Rounding(prec, rounding, trunc_act=bool(pert.get("trunc_act")))
    feats, mask, zf, zmid, zf_of = geom(R)
    if pert.get("zshift"):                     # perturbation (c): the depth feature one voxel off from voxel `zshift` on
        k = np.arange(len(zf))
        zf = zf_of(np.where(k >= pert["zshift"], k + 1, k))
    out = {"mask": mask}
    p = np.zeros((feats.shape[1], len(zf)))
    for m, tag in ((0, "lr"), (1, "hr")):
        net = Mlp(sd, m)
        if pert.get("b1_16"):                  # perturbation (d): b1 through a 16-bit rounding
            net.b[1] = R.h(net.b[1])
        cc = column_constants(R, net, feats, acc, order)
        acc1 = layer1(R, net, cc, zf, zmid, p, acc, order, pert if m == pert.get("mlp", 0) else {})
        logit = _tail(R, net, cc, zf, p, acc1, acc, order)
        p = _occupancy(R, mask, logit)
        out["logit_" + tag], out["occ_" + tag] = logit, p
    return out


# ------------------------------------------------------------------ kernel 3
def _layer1_dense(R, net, cc, zf, zmid, p, acc, order, pert):
    C, rz = p.shape
    x = R.fma(zf[None, None, :], net.wz[0][:, None, None], cc[0][:, :, None])      # fmaf(zf, w0z, a0)  (surs_grid_v3.inc:177)
    if net.m:
        x = R.fma(p[None], net.wp[0][:, None, None], x)                            # fmaf(p, w0p, .)    (v3.inc:178)
    y0 = R.act(R.lrelu01(x))                                                       # (elem)lrelu01(v)   (v3.inc:182)
    if "drop" in pert:                         # perturbation (b): one channel's contribution missing over some voxels
        ch, col, ks = pert["drop"]
        y0[ch, col, ks] = 0.0
    # b1 through its three 16-bit parts (pack:281-297) against 1 / scale (v3.inc:215-228): one MFMA into a zero accumulator
    scale = B1FRAG_SCALE[R.prec] if R.on else 1.0
    parts = R.split3(R.f(net.b[1] * scale))
    b1 = sum(np.asarray(q, np.float64) * R.h(1.0 / scale) for q in parts)
    if acc is np.float32:
        b1 = R.f(b1)
    init = np.broadcast_to(b1[:, None], (D2, C * rz))
    return gemm([(R.h(net.W[1]), y0.reshape(D1, C * rz))], acc, order, init).reshape(D2, C, rz)      # 16-bit core (pack:146-153)


def dense(sd, prec, geom, acc=np.float64, order="asc", rounding=True, pert=None):
    """Column kernel 3: every layer-0 activation rounded to 16 bits, the K = 1024 product whole."""
    return _sweep(_layer1_dense, sd, prec, geom, acc, order, rounding, pert)


# ------------------------------------------------------------------ kernels 10 and 12
def r_vectors(R, net, a0, zmid, acc, order):
    """R = W1 (g . [a0 | w0z | w0p]) [3][512, C] with g from colsum_prepare_kernel's expressions (query:654-656).  bf16 sweep: ONE
    f16 part of each operand (rparts == 1, query:1287; the weights' f16(w) plane, query:1320), fp16 sweep: the fp32-grade split."""
    xm = R.fma(zmid, net.wz[0][:, None], a0)
    if net.m:
        xm = R.fma(0.5, net.wp[0][:, None], xm)
    g = np.where(xm > 0.0, 1.0, R.c01)
    out = []
    for v in (a0, np.broadcast_to(net.wz[0][:, None], a0.shape), np.broadcast_to(net.wp[0][:, None], a0.shape)):
        val = R.f(g * v)
        if R.on and R.prec == "bf16":
            out.append(R.f(gemm([(R.f16(net.W[1]), R.f16(val))], acc, order)))
        else:
            out.append(gemm_split2(R, net.W[1], val, acc, order))
    return out, xm > 0.0


def _layer1_restated(R, net, cc, zf, zmid, p, acc, order, pert):
    C, rz = p.shape
    (RA, RB, RC), g1 = r_vectors(R, net, cc[0], zmid, acc, order)
    # ---- the affine part: one k-step of the parts of (b1 + RA, RB, RC) against those of (1, zf, p); the six partial products per
    #      factor that flo / fhi x lo / hi hold (surs_grid_v10.inc:108-112, :294-299)
    a = R.split3(R.f(RA + net.b[1][:, None]))                        # rp[0] + b1[row] in fp32, then split (v10.inc:108)
    b = R.split3(RB)
    z = R.split3(zf)
    pairs = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))
    aff = (a[0] + a[1] + a[2])[:, :, None] + np.zeros((D2, C, rz))
    for i, j in pairs:
        aff += b[i][:, :, None] * z[j][None, None, :]
    if net.m:
        c = R.split3(RC)
        q = R.split3(p)
        for i, j in pairs:
            aff += c[i][:, :, None] * q[j][None]
    if acc is np.float32:
        aff = R.f(aff)
    # ---- the residuals, for EVERY channel: a channel on its mid-column branch yields an exact 0 (v10.inc:262-277)
    x = R.fma(zf[None, None, :], net.wz[0][:, None, None], cc[0][:, :, None])      # fmaf(zf_own, cz, ca)
    if net.m:
        x = R.fma(p[None], net.wp[0][:, None, None], x)                            # fmaf(p_own, cp, x)
    clamped = np.where(g1[:, :, None], np.minimum(x, 0.0), np.maximum(x, 0.0))     # med3(x, lo, hi)
    r = R.act(R.f(np.where(g1, -R.k99, R.k99)[:, :, None] * clamped))              # the product in fp32, THEN converted
    if "drop" in pert:                         # perturbation (b): the channel's affine share and its residual
        ch, col, ks = pert["drop"]
        r[ch, col, ks] = 0.0
        gx = np.where(g1[ch, col], 1.0, R.c01) * x[ch, col, ks]
        aff[:, col, ks] -= R.h(net.W[1])[:, ch, None] * gx[None]
    N = C * rz
    return gemm([(R.h(net.W[1]), r.reshape(D1, N))], acc, order, aff.reshape(D2, N)).reshape(D2, C, rz)      # W1t (pack:264-270)


def restated(sd, prec, geom, acc=np.float64, order="asc", rounding=True, pert=None):
    """Column kernels 10 and 12: layer 1 as the per-column affine part (fp32 grade) + the residuals (16 bits)."""
    return _sweep(_layer1_restated, sd, prec, geom, acc, order, rounding, pert)


def layer0_lr(sd, prec, geom):
    """|LeakyReLU(x)| [1024, C, rz] of the lr classifier's layer 0 in the float64 model: how much a channel contributes where."""
    R = Rounding(prec)
    feats, _, zf, _, _ = geom(R)
    net = Mlp(sd, 0)
    cc = column_constants(R, net, feats, np.float64, "asc")
    return np.abs(R.lrelu01(R.fma(zf[None, None, :], net.wz[0][:, None, None], cc[0][:, :, None])))


# ------------------------------------------------------------------ the one-product point path
def points_one_product(sd, points, calib, zmul, zdiv, feat_lr, feat_hr, acc=np.float64, order="asc", rounding=True):
    """run_points_fp32 with parts = 1 (query:476-519): the features, the depth feature and the lr occupancy as ONE f16 part
    (gather_kernel, query:196-206, :249; mlp_last_kernel, query:282-287), the weights' f16(w) plane (query:503) in the four layer
    GEMMs, fp32 accumulation, bias and LeakyReLU in fp32 (surs_gemm.inc:286-287), the activations as one f16 part - layer 3's stay
    fp32 (G3_F32) -; layer 4 is an fp32 fmaf chain over layer 3's fp32 outputs and the UNROUNDED fp32 features (query:275-277)."""
    R = Rounding("fp16", rounding)
    cal4 = np.eye(4)
    cal4[:3] = np.asarray(calib, np.float64).reshape(-1)[:12].reshape(3, 4)
    rows, mask, _ = gc.point_rows(feat_lr, feat_hr, R.f(points), cal4)
    N = rows.shape[1]
    Z = R.f(gc.project(R.f(points), cal4)[2])                        # exact for the calibrations used (power-of-two scales)
    zfeat = R.f(R.f(Z * zmul) / zdiv)                                # Z * zmul / zdiv (query:193)
    F = np.concatenate([R.f(rows[:C_G]), zfeat[None], np.zeros((1, N))])
    out = {"mask": mask}
    for m, tag in ((0, "lr"), (1, "hr")):
        net = Mlp(sd, m)
        X = F[:C_G + 1 + m]
        Xh = R.f16(X)
        y = None
        for l in range(4):
            W = R.f16(net.W[l])
            dk = (0, D1, D2, D3)[l]
            prods = []
            if l > 0:
                prods.append((W[:, :dk], y))
            if l in (0, 2, 3):
                prods.append(_pad16(W[:, dk:], Xh))
            a = 0.0
            for pr in prods:                                         # segment s1 (y), then s2 (features): k-tiles in this order
                a = gemm([pr], acc, order, a if np.ndim(a) else None)
            t = R.f(a + net.b[l][:, None])
            y = np.where(t > 0.0, t, R.f(R.c01 * t))
            if l < 3:
                y = R.f16(y)
        if acc is np.float64:
            logit = net.b[4][0] + net.W[4][0, :D4] @ y + net.W[4][0, D4:] @ X
        else:
            logit = np.full(N, net.b[4][0])
            for k in range(D4):
                logit = R.fma(net.W[4][0, k], y[k], logit)
            for k in range(C_G + 1 + m):
                logit = R.fma(net.W[4][0, D4 + k], X[k], logit)
        p = R.f(mask * R.f(sigmoid(logit)))
        F[C_G + 1] = p
        out["logit_" + tag], out["occ_" + tag] = logit, p
    return out


# ------------------------------------------------------------------ the bound
FACTOR = 8.0            # what tests/grad_common.py's compare() gives "another summation order"
SAT = 5.0               # |logit| from which an fp32 occupancy no longer resolves its logit (tools/precision_report.py field_stats)


def floor_of(logit):
    """4 * 2^-24 / (p (1 - p)): four fp32 roundings (expf, add, divide, the stored occupancy) seen through the logit."""
    p = sigmoid(logit)
    return 4.0 * 2.0 ** -24 / (p * (1.0 - p))


def bounds(ref, fp32_forms, tag, sel, floor=None):
    """({"mean", "max", "median": bound}, e) over the voxels sel of classifier tag: e = the larger deviation of the two
    fp32-accumulating forms from the float64 model; floor: per compared voxel, floor_of the model's logit unless given.
    bound[s] = 8 max(s(e), s(floor)).  Mean and max are the two statistics the kernels were to be held to; the median is a third,
    sharper one for errors that touch every voxel: accumulation order moves few voxels by much (e's mean is 30 to 90 times its median),
    a bias through a 16-bit rounding moves every voxel by a little - in fp16 by 3 to 6 times mean(e), which the mean lets through,
    and by 3 times the median's bound (tests/test_column_model_host.py)."""
    e = np.max([np.abs(f["logit_" + tag] - ref["logit_" + tag]) for f in fp32_forms], 0)[sel]
    fl = floor_of(ref["logit_" + tag])[sel] if floor is None else floor
    return {s: FACTOR * max(f(e), f(fl)) for s, f in (("mean", np.mean), ("max", np.max), ("median", np.median))}, e


def breaks(dev, bound):
    """The statistics of deviations dev that exceed their bound."""
    return [s for s, f in (("mean", np.mean), ("max", np.max), ("median", np.median)) if f(dev) > bound[s]]
