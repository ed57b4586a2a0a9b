"""sha256 of the gradient GEMM kernels' outputs on seeded inputs at shapes that reach every edge of the 64 x 64 tile (csrc/surs_grad_tile.h):
A/B of library builds (SURS_LIB_PATH) for bit identity.  One line per call: conv_grad_weight / conv_grad_input at the PRIMS shapes of
tests/test_gpu_sr_grads.py (masked by a stored output, then accumulating into seeded buffers through pitched Imgs), mlp_grads with
feature maps on grad_common's tiny and d48 cases, tail_joint_grad at both tile heights."""
import hashlib, os, sys
import numpy as np
import torch
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_common as g, grad_common as gc
from surs_amd import native, prng
PRIMS = [(32, 3, 8, 16, 3, 1), (3, 32, 8, 16, 3, 1), (512, 512, 1, 2, 3, 1), (64, 64, 24, 44, 3, 1), (32, 32, 8, 16, 3, 2),
         (32, 32, 6, 10, 3, 2), (64, 64, 8, 16, 1, 1)]
dev = g.dev()


def u(tag, seed, shape):
    return prng.uniform("grad_hash_" + tag, seed, shape, -1.0, 1.0)


def img(a, pitch=0):
    """numpy [C,H,W] -> native.Img whose channel pitch is C + pitch, zeros in the gap."""
    c, h, w = a.shape
    buf = torch.zeros((h * w, c + pitch), dtype=torch.float32)
    buf[:, :c] = torch.from_numpy(np.ascontiguousarray(a.transpose(1, 2, 0))).reshape(h * w, c)
    return native.Img(h, w, c, c + pitch, buf.reshape(-1).to(dev))


def show(name, *tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in tensors)).hexdigest()[:16]
    print("%-34s %s" % (name, h), flush=True)


for cin, cout, h, w, k, s in PRIMS:
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    x, wt, gr, y = u("x", cin + h, (cin, h, w)), u("w", cout + k, (cout, cin, k, k)), u("g", cout + ho, (cout, ho, wo)), u("y", cout + wo, (cout, ho, wo))
    y.reshape(-1)[::7] = 0.0
    y.reshape(-1)[3::11] = -0.0
    tag = "%d->%d %dx%d k%d s%d" % (cin, cout, h, w, k, s)
    wd = torch.from_numpy(wt).to(dev)
    dw, db = native.conv_grad_weight(img(gr), img(x), k, s, y=img(y), slope=0.2)
    dx = native.conv_grad_input(img(gr), wd, h, w, s, y=img(y), slope=0.2)
    show("conv " + tag + " masked", dw, db, dx.buf)
    dw, db = torch.from_numpy(u("dw", cin, (cout, cin, k, k))).to(dev), torch.from_numpy(u("db", cout, (cout,))).to(dev)
    native.conv_grad_weight(img(gr, 5), img(x, 3), k, s, dw=dw, db=db, accumulate=True)
    dx = native.conv_grad_input(img(gr, 5), wd, h, w, s, dx=img(u("dx", cin + w, (cin, h, w)), 7), add=True)
    show("conv " + tag + " adding", dw, db, dx.buf)

for name in ("tiny", "d48"):
    x = gc.kept(gc.inputs(name), gc.load_fixture(os.path.join(ROOT, "tests", "golden"), name)["keep"])
    sd = gc.mlp_state(name)
    params = native.MlpParams(sd, dev, native.mlp_shapes(sd, gc.opt(name)))
    B, N = x["points_mr"].shape[0], x["points_mr"].shape[2]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for b in range(B):
        grads, fgr = native.mlp_grads(up(x["points_mr"][b]), up(x["points_sr"][b]), x["calib_mr"][b].reshape(-1)[:12],
                                      x["calib_sr"][b].reshape(-1)[:12], gc.ZMUL, gc.ZDIV, [g.upload_nhwc(f) for f in x["feat_lr"][b]],
                                      g.upload_nhwc(x["feat_hr"][b]), params, up(x["lab_lr"][b]), up(x["lab_hr"][b]), gc.LOSS_WEIGHTS, B * N,
                                      feat_grads=True)
        show("mlp_grads %s image %d" % (name, b), *grads.values(), *fgr.lr, fgr.hr)

for p, D in ((70, 48), (33, 300)):
    rows = lambda a: img(a.T.reshape(a.shape[1], 1, a.shape[0]))
    wgt = lambda tag, seed, shape: torch.from_numpy(u(tag, seed, shape)).to(dev).reshape(shape + (1, 1))
    d_out, d_a = native.tail_joint_grad(rows(u("go", p + D, (p, D))), rows(u("gn", p + D + 1, (p, 256))), wgt("al", D, (256, D)),
                                        wgt("l", D + 1, (D, 256)), wgt("bl", D + 2, (256, 256)))
    show("tail_joint p=%d D=%d" % (p, D), d_out.buf, d_a.buf)
