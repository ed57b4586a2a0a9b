"""The bf16 / fp16 column kernels 12, 10 and 3 and the one-product point path, held to tests/column_model.py: a float64 model that
rounds to 16 bits where the kernels' sources do and forms the partial products they form.  A correct kernel differs from it by
accumulation order only, so the tolerance is the model's own distance to itself accumulating in fp32 (both k orders) - not the
width of bf16's rounding error, which hides everything smaller (a truncating conversion, a missing channel, a depth feature one voxel
off, a bias through 16 bits: tests/test_column_model_host.py shows that this bound catches them).

Per case and classifier, over the compared voxels:   dev = |kernel logit - float64 model logit|,   e = |fp32-accumulating model -
float64 model| (the larger of the two k orders),   floor = 4 * 2^-24 / (p (1 - p)) (four fp32 roundings between logit and the
stored occupancy; points: 2^-22 max |logit|);
    mean(dev) <= 8 max(mean(e), mean(floor))    and    max(dev) <= 8 max(max(e), max(floor)),
and the same for the median (column_model.bounds says why).  8 is what tests/grad_common.py gives another summation order.
Grids store occupancies: the logit is recovered in float64 where the model's |logit| < 5 (tools/precision_report.py, field_stats);
the other voxels - at most 1 % of a case - are compared as occupancies, |dp| <= 0.0067 (max bound) + 2^-22.  Every test prints
mean(dev) / mean(e) and max(dev) / max(e).

Cases (everything from seeds; weights common.state_dict(), features weights.body_features(32, 128)):
  S  tests/column_bits.py's grid, 2 x 8 x 296 (two full 128-voxel tiles and a ragged 40), layer 0's depth column x 1 (kernel 12
     evaluates every tile itself) and x 60 (the tiles go to kernel 10's tile mode, multi-chunk lists); 12 and 10 against
     `restated`, 3 against `dense`;
  F  36 x 32 x 168 = 1152 columns, bf16, kernel 12: the only case on rvec_fused_kernel (S runs rvec_small_kernel); 48 columns are
     modelled, 16 of them from the last 64, the end of a batch that is padded to 1280 columns;
  E  a flipped depth axis on 4 x 6 x 200 and bounds beyond the image on 6 x 5 x 72 (columns outside: exact zeros, the same set);
  P  777 points, seven of them outside the image (three 256-point tiles and a ragged 9), native.query_points inside
     native.reduced_point_operands() against `points_one_product`: the logits straight from the library."""
import numpy as np
import pytest

import column_bits as cb
import column_model as cm
import common

pytestmark = pytest.mark.gpu

ZMUL, ZDIV = 512, 200.0
F_GRID = (36, 32, 168)
_models = {}


def mlp_sd(gain):
    sd = {k: np.array(v, copy=True) for k, v in common.state_dict().items() if k.startswith("mlp_")}
    for m in ("mlp_lr.", "mlp_hr."):
        sd[m + "conv0.weight"][:, 320] *= float(gain)
    return sd


def features():
    if "features" not in _models:
        from surs_amd import weights
        _models["features"] = weights.body_features(32, 128)
    return _models["features"]


def models(key, fn, *args, **kw):
    """(float64 model, [fp32 ascending, fp32 descending]) of a case, computed once per module."""
    if key not in _models:
        _models[key] = (fn(*args, **kw), [fn(*args, acc=np.float32, order=o, **kw) for o in ("asc", "desc")])
    return _models[key]


def sweep_models(key, fn, gain, prec, mat, calib, cols, rz):
    fl, fh = features()
    geom = lambda R: cm.sweep_geometry(R, mat, calib, cols, rz, ZMUL, ZDIV, fl, fh)
    return models(key, fn, mlp_sd(gain), prec, geom)


def hold(name, tag, ref, forms, occ=None, logit=None):
    """Assert the bound for classifier tag: occ [C, rz] as the kernel stored it (grids) or logit [N] straight from the library."""
    want = ref["logit_" + tag]
    inimg = np.broadcast_to((ref["mask"] > 0).reshape(-1, *([1] * (want.ndim - 1))), want.shape)
    sat = inimg & (np.abs(want) >= cm.SAT) if logit is None else np.zeros_like(inimg)
    sel = inimg & ~sat
    share = sat.sum() / max(1, inimg.sum())
    floor = None
    if logit is None:
        occ = np.asarray(occ, np.float64)
        assert occ.shape == want.shape and np.isfinite(occ).all()
        # outside the image: exact zeros, and the same set
        assert np.array_equal(occ == 0.0, ~inimg), "%s %s: zero sets differ" % (name, tag)
        assert (occ[sel] > 0.0).all() and (occ[sel] < 1.0).all()
        got = np.log(occ[sel] / (1.0 - occ[sel]))
    else:
        got = np.asarray(logit, np.float64)[sel]
        floor = np.full(int(sel.sum()), 2.0 ** -22 * np.abs(want[sel]).max())
    bound, e = cm.bounds(ref, forms, tag, sel, floor)
    dev = np.abs(got - want[sel])
    print("%-24s %s: mean(dev) / mean(e) = %6.3f   max(dev) / max(e) = %6.3f   median(dev) / its bound = %5.3f   (dev mean %.3g max "
          "%.3g median %.3g; bounds %.3g %.3g %.3g; %d voxels, %.2f %% saturated)"
          % (name, tag, dev.mean() / e.mean(), dev.max() / e.max(), np.median(dev) / bound["median"], dev.mean(), dev.max(),
             np.median(dev), bound["mean"], bound["max"], bound["median"], int(sel.sum()), 100.0 * share))
    assert share <= 0.01, (name, tag, share)
    assert not cm.breaks(dev, bound), (name, tag, cm.breaks(dev, bound))
    if sat.any():
        dp = np.abs(occ[sat] - ref["occ_" + tag][sat]).max()
        assert dp <= 0.0067 * bound["max"] + 2.0 ** -22, (name, tag, "saturated", dp)


def grid_matrix(res, b_min, b_max, centres):
    """index -> world: voxel centres over [b_min, b_max] (centres) or the corners' lattice test_sweep_edge_geometries uses."""
    m = np.zeros((3, 4))
    for a, r in enumerate(res):
        m[a, a] = (b_max[a] - b_min[a]) / r
        m[a, 3] = b_min[a] + (0.5 * m[a, a] if centres else 0.0)
    return m.reshape(-1)


# ------------------------------------------------------------------ S
@pytest.fixture(scope="module")
def ctx():
    return cb.Context()


@pytest.mark.parametrize("kv", [12, 10, 3])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("gain", cb.GAINS)
def test_small_grid_kernels_against_the_model(ctx, gain, prec, kv):
    if gain == 60 and prec == "bf16" and kv == 12:
        # the premise of the x 60 case: the tiles list more than kernel 12 stages
        assert ctx.listed(60)[0] > 128 > ctx.listed(1)[0]
    fn = cm.dense if kv == 3 else cm.restated
    cols = [(cb.I0 + i, j) for i in range(cb.PLANES) for j in range(cb.RY)]
    ref, forms = sweep_models(("S", fn.__name__, gain, prec), fn, gain, prec, cb.matrix(), common.CALIB, cols, cb.RZ)
    vol = ctx.bits(gain, prec, kv).view(np.float32).reshape(2, cb.PLANES * cb.RY, cb.RZ)
    name = "S x%d %s kernel %d" % (gain, prec, kv)
    hold(name, "lr", ref, forms, occ=vol[1])
    hold(name, "hr", ref, forms, occ=vol[0])


# ------------------------------------------------------------------ F, E
class Sweeps:
    def __init__(self):
        import gpu_common as g
        from surs_amd import native
        self.native, self.dev = native, g.dev()
        fl, fh = features()
        self.Fl, self.Fh = g.upload_nhwc(fl), g.upload_nhwc(fh)
        self.ws = native.Workspace(self.dev)
        self.blobs = {}

    def volumes(self, res, mat, calib, prec, kv):
        """float32 [2 (hr, lr), columns, rz] of the whole grid."""
        if prec not in self.blobs:
            self.blobs[prec] = self.native.pack_mlp(mlp_sd(1), prec, self.dev)[0]
        cal = np.asarray(calib, np.float32).reshape(-1)[:12]
        vh, vl = self.native.query_grid(0, res[0], res[1], res[2], mat, cal, ZMUL, ZDIV, self.Fl, self.Fh, self.blobs[prec], prec, self.ws,
                                        kernel=kv)
        return np.stack([vh.cpu().numpy(), vl.cpu().numpy()]).reshape(2, res[0] * res[1], res[2])


@pytest.fixture(scope="module")
def sweeps():
    return Sweeps()


def test_fused_r_kernel_batch_against_the_model(sweeps):
    assert sweeps.native.get_option("r_fused") == 1
    planes, ry, rz = F_GRID
    ncols = planes * ry
    assert ncols == 1152 > 1024                       # more than 1024 columns: rvec_fused_kernel
    rng = np.random.RandomState(1152)
    pick = np.sort(np.concatenate([rng.choice(ncols - 64, 32, replace=False), ncols - 64 + rng.choice(64, 16, replace=False)]))
    mat = grid_matrix(F_GRID, [-0.5] * 3, [0.5] * 3, centres=True)
    cols = [divmod(int(c), ry) for c in pick]
    ref, forms = sweep_models(("F",), cm.restated, 1, "bf16", mat, common.CALIB, cols, rz)
    vol = sweeps.volumes(F_GRID, mat, common.CALIB, "bf16", 12)[:, pick]
    hold("F bf16 kernel 12", "lr", ref, forms, occ=vol[1])
    hold("F bf16 kernel 12", "hr", ref, forms, occ=vol[0])


FLIP = (np.diag([1.0, 1.0, -1.0, 1.0]).astype(np.float32) @ common.CALIB).astype(np.float32)
EDGES = {"flipped": (FLIP, [-0.5] * 3, [0.5] * 3, (4, 6, 200)),
         "beyond": (common.CALIB, [-0.6, -0.55, -0.5], [0.6, 0.5, 0.45], (6, 5, 72))}


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("edge", sorted(EDGES))
def test_edge_geometries_against_the_model(sweeps, edge, prec):
    calib, b_min, b_max, res = EDGES[edge]
    mat = grid_matrix(res, b_min, b_max, centres=False)
    cols = [(i, j) for i in range(res[0]) for j in range(res[1])]
    ref, forms = sweep_models(("E", edge, prec), cm.restated, 1, prec, mat, calib, cols, res[2])
    outside = int((ref["mask"] == 0).sum())
    assert (outside > 0) == (edge == "beyond") and outside < len(cols)
    vol = sweeps.volumes(res, mat, calib, prec, 12)
    name = "E %s %s kernel 12" % (edge, prec)
    hold(name, "lr", ref, forms, occ=vol[1])
    hold(name, "hr", ref, forms, occ=vol[0])


# ------------------------------------------------------------------ P
def test_one_product_point_path_against_the_model(sweeps):
    import torch
    from surs_amd import weights
    nat = sweeps.native
    pts = weights.synthetic_points(777, seed=12, lo=-0.5, hi=0.5)
    pts[0, 770:] = np.array([0.51, -0.6, 0.7, -0.75, 0.55, 0.3, -0.2], np.float32)     # seven points outside the image:
    pts[1, 775:] = np.array([0.52, -0.8], np.float32)                                  # five in x, two in y
    fl, fh = features()
    cal = common.CALIB.reshape(-1)[:12]
    ref, forms = models(("P",), cm.points_one_product, mlp_sd(1), pts, cal, ZMUL, ZDIV, fl, fh)
    assert int((ref["mask"] == 0).sum()) == 7
    blob = sweeps.native.pack_mlp(mlp_sd(1), "bf16", sweeps.dev)[0]
    with nat.reduced_point_operands():
        phr, plr, lhr, llr = nat.query_points(torch.from_numpy(pts).to(sweeps.dev), cal, ZMUL, ZDIV, sweeps.Fl, sweeps.Fh, blob, sweeps.ws,
                                              want_logits=True)
    for tag, occ, lg in (("lr", plr, llr), ("hr", phr, lhr)):
        occ, lg = occ.cpu().numpy().astype(np.float64), lg.cpu().numpy()
        hold("P one product", tag, ref, forms, logit=lg)
        inimg = ref["mask"] > 0
        assert np.array_equal(occ == 0.0, ~inimg)
        # the occupancy is the sigmoid of the logit it came with (four fp32 roundings)
        assert np.abs(occ[inimg] - cm.sigmoid(lg.astype(np.float64)[inimg])).max() <= 2.0 ** -22
