"""The cases of tests/test_fused_model_host.py and tests/test_gpu_fused_model.py: classifier shapes, seeded inputs on which the fp32
gather is exact, and the models of tests/fused_model.py computed once per process.

Why these inputs: the kernels gather in fp32 (bilinear_taps, then tap_sum as four multiply-adds the compiler may or may not
contract); with two or three operand parts an ulp of difference between a float64 restatement of the gather and the kernel's is as
large as the effect measured.  So: maps of (2^a + 1) x (2^b + 1) pixels, feature values k 2^-8, coordinates k 2^-7, calibrations with
dyadic entries - every tap weight and every product is then exact in fp32 (test_fused_model_host.py asserts it)."""
import numpy as np

import common
import fused_model as fm
import grad_common as gc
from surs_amd import options, weights

ZMUL, ZDIV = 1024 // 2, 200.0
C_HR = 64
N = 777                                   # 24 tiles of 32 and a ragged 9 / 48 tiles of 16 and a ragged 9
OUTSIDE = 7


def _dims(tag, dims):
    return ["--mlp_dim_" + tag] + [str(d) for d in dims]


def _res(tag, res):
    return ["--mlp_res_layers_" + tag] + [str(r) for r in res]


def _hg(D, hidden, res=None):
    out = ["--hg_dim", str(D)] + _dims("lr", [D + 65] + hidden + [1]) + _dims("hr", [D + 66] + hidden + [1])
    return out + (_res("lr", res) + _res("hr", res) if res is not None else [])


_ODD = [1000, 500, 250, 100]
SHAPES = {   # the flags of tests/test_gpu_mlp_shapes.py's shapes (l2: test_gpu_mlp_shapes_views.py), the released shape, two other --hg_dim
    "s1": _dims("lr", [321, 512, 256, 128, 1]) + _dims("hr", [322, 512, 256, 128, 1]) + _res("lr", [1, 2, 3]) + _res("hr", [1, 2, 3]),
    "odd": _dims("lr", [321] + _ODD + [1]) + _dims("hr", [322] + _ODD + [1]),
    "deep": _dims("lr", [321, 1024, 1024, 512, 256, 128, 1]) + _dims("hr", [322, 1024, 1024, 512, 256, 128, 1])
    + _res("lr", [2, 3, 4, 5]) + _res("hr", [2, 3, 4, 5]),
    "res0": _res("lr", [0, 2]) + _res("hr", [0, 2]),
    "l1": _dims("lr", [321, 1]) + _dims("hr", [322, 1]) + ["--no_residual"],
    "nores": ["--no_residual"],
    "mixed": _dims("lr", [321, 512, 256, 128, 1]) + _res("lr", [1, 2, 3]) + _dims("hr", [322] + _ODD + [1]),
    "released": [],
    "l2": _dims("lr", [321, 64, 1]) + _dims("hr", [322, 64, 1]) + _res("lr", [1]) + _res("hr", [1]),
    "d48": gc.CASES["d48"][0],                          # D = 48: gen_c0pad 128, the feature row partly lr, partly hr inside one k-step
    "d288": _hg(288, [512, 256, 128], [1, 2, 3]),       # D = 288: gen_c0pad 384, not the released 352
}
SINGLE = ["s1", "odd", "deep", "res0", "l1", "nores", "mixed", "released"]          # case A
HG_DIM = ["d48", "d288"]                                                              # case B (non-square maps)
VIEWS = [("s1", 2), ("odd", 2), ("l1", 3), ("l2", 2)]                                 # case D
STACKS = 3                                                                            # case E: s1 on three lr maps
STACK_SEED = 70

_cache = {}


def hg_dim(name):
    return {"d48": 48, "d288": 288}.get(name, 256)


def opt(name):
    return options.BaseOptions().parse(common.FLAGS + SHAPES[name])


def mlp_sd(name):
    key = ("sd", name)
    if key not in _cache:
        sd = weights.synthetic_state_dict(opt(name), seed=0)
        _cache[key] = {k: v for k, v in sd.items() if k.startswith("mlp_")}
    return _cache[key]


# ------------------------------------------------------------------ inputs
def maps(D, seed, square=True):
    """(lr [D, 17, 17], hr [64, 65, 65]) - or 9 x 17 and 33 x 65 - float32: seeded integers times 2^-8, in [-1, 1]."""
    rng = np.random.RandomState(seed)
    hl, hh = (17, 65) if square else (9, 33)
    return ((rng.randint(-256, 257, (D, hl, 17)) / 256.0).astype(np.float32),
            (rng.randint(-256, 257, (C_HR, hh, 65)) / 256.0).astype(np.float32))


def points(seed, n=N):
    """[3, n] float32: seeded integers times 2^-7 in [-0.5, 0.5]; the last seven put outside the image of common.CALIB by hand, five
    in x, two in y (case P of tests/test_gpu_column_model.py)."""
    p = (np.random.RandomState(seed).randint(-64, 65, (3, n)) / 128.0).astype(np.float32)
    p[0, n - 7:] = np.array([65, -77, 90, -96, 70, 38, -26], np.float32) / 128.0
    p[1, n - 2:] = np.array([66, -102], np.float32) / 128.0
    return p


CALIB12 = common.CALIB.reshape(-1)[:12]
# view 0: common.CALIB; view 1: a 90 degree turn about y, a shear of 2^-2 and offsets of 2^-5; view 2: a mirror with shears and offsets
VIEW_CALIBS = np.array([
    [2, 0, 0, 0, 0, -2, 0, 0, 0, 0, 2, 0],
    [0, 0.25, 2, 2.0 ** -5, 0, -2, 0, -2.0 ** -5, -2, 0, 0, 0],
    [-2, 0, 0.25, -2.0 ** -5, 0.25, -2, 0, 2.0 ** -5, 0, 0, -2, 2.0 ** -4]], np.float32)


def single_inputs(name):
    D = hg_dim(name)
    fl, fh = maps(D, 50 + D, square=name not in HG_DIM)
    return dict(points=points(12), calib=CALIB12, feat_lr=fl, feat_hr=fh)


def views_inputs(V):
    f = [maps(256, 60 + v) for v in range(V)]
    return dict(points=np.stack([points(12)] * V), calibs=VIEW_CALIBS[:V], feats_lr=[a for a, _ in f], feats_hr=[b for _, b in f])


def stack_inputs():
    return dict(points=points(12), calib=CALIB12, feats_lr=[maps(256, STACK_SEED + s)[0] for s in range(STACKS)],
                feat_hr=maps(256, STACK_SEED)[1])


# ------------------------------------------------------------------ models, once per process
def models(key, fn, *args, **kw):
    """(float64 model, [fp32 ascending, fp32 descending])."""
    if key not in _cache:
        _cache[key] = (fn(*args, **kw), [fn(*args, acc=np.float32, order=o, **kw) for o in ("asc", "desc")])
    return _cache[key]


def single_models(name, NP):
    x = single_inputs(name)
    return models(("single", name, NP), fm.single, mlp_sd(name), NP, x["points"], x["calib"], ZMUL, ZDIV, x["feat_lr"], x["feat_hr"])


def hr_alone_models(name, NP):
    """Case C: the hr classifier alone on the float64 model's own lr occupancy as fp32."""
    x = single_inputs(name)
    p_lr = single_models(name, NP)[0]["occ_lr"].astype(np.float32)
    return p_lr, models(("hr", name, NP), fm.single, mlp_sd(name), NP, x["points"], x["calib"], ZMUL, ZDIV, x["feat_lr"], x["feat_hr"],
                        p_lr=p_lr)


def views_models(name, V, NP):
    x = views_inputs(V)
    return models(("views", name, V, NP), fm.views, mlp_sd(name), NP, x["points"], x["calibs"], ZMUL, ZDIV, x["feats_lr"], x["feats_hr"])


def stack_models(s, NP=1):
    x = stack_inputs()
    return models(("stack", s, NP), fm.single, mlp_sd("s1"), NP, x["points"], x["calib"], ZMUL, ZDIV, x["feats_lr"][s], x["feat_hr"])
