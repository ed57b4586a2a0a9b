"""tests/fused_model.py is checked before it judges a kernel (no GPU, no product code):
  * the inputs of tests/fused_cases.py make the gather exact: the float64 gather equals its own fp32 rounding for every point and
    channel, and a numpy fp32 restatement of bilinear_taps / tap_sum, with and without fused multiply-adds, gives those same values;
  * with every rounding switched off the model IS the classifier: `single` equals grad_common.mlp_forward on point_rows for every
    shape the GPU cases use, `views` equals a float64 restatement of the reference's SurfaceClassifier.forward with num_views > 1
    (lib/model/SurfaceClassifier.py:53-81) written here from the formulas;
  * the fp32-grade claim as a measurement: max |NP = 2 model - unrounded model| and the same for NP = 3 on the logits, per shape;
  * the bound of tests/test_gpu_fused_model.py separates wrong models: the perturbed float64 models (a) - (g) of fused_model's
    docstring each break it against the unperturbed forms in the mean, the max or the median, on shapes s1 and odd.  One does not:
    (a) with two or three parts, where the later parts pick up what a truncated first part leaves (NOTES.md, "What the bound cannot
    see"); the test prints its ratios and asserts that it stays inside, so that the note stays true."""
import numpy as np
import pytest

import fused_cases as fc
import fused_model as fm
import grad_common as gc
from column_model import Rounding

ALL_SHAPES = fc.SINGLE + fc.HG_DIM + ["l2"]
OFF = Rounding("fp16", on=False)


# ------------------------------------------------------------------ the inputs
def _taps_f32(fmap, u, v, fused):
    """bilinear_taps and tap_sum (csrc/surs_query.hip:111-136) in numpy float32: [C, N] float32.  fused: every a += t * w as one fmaf
    (the product exact in float64, one rounding), else the product rounded to fp32 first."""
    f32 = np.float32
    fmap = np.asarray(fmap, f32)
    H, W = fmap.shape[1:]
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    ix = ((u + f32(1.0)) / f32(2.0)) * f32(W - 1)
    iy = ((v + f32(1.0)) / f32(2.0)) * f32(H - 1)
    assert ix.dtype == f32 and iy.dtype == f32
    x0, y0 = np.floor(ix), np.floor(iy)
    x1, y1 = x0 + f32(1.0), y0 + f32(1.0)
    ok = lambda a, n: (a >= 0) & (a < n)
    zero = f32(0.0)
    w = [np.where(ok(y0, H) & ok(x0, W), (x1 - ix) * (y1 - iy), zero), np.where(ok(y0, H) & ok(x1, W), (ix - x0) * (y1 - iy), zero),
         np.where(ok(y1, H) & ok(x0, W), (x1 - ix) * (iy - y0), zero), np.where(ok(y1, H) & ok(x1, W), (ix - x0) * (iy - y0), zero)]
    cl = lambda a, n: np.clip(a, 0, n - 1).astype(np.int64)
    taps = [fmap[:, cl(y0, H), cl(x0, W)], fmap[:, cl(y0, H), cl(x1, W)], fmap[:, cl(y1, H), cl(x0, W)], fmap[:, cl(y1, H), cl(x1, W)]]
    a = np.zeros(taps[0].shape, f32)
    for t, wq in zip(taps, w):
        assert t.dtype == f32 and wq.dtype == f32
        if fused:
            a = (a.astype(np.float64) + t.astype(np.float64) * wq.astype(np.float64)[None]).astype(f32)
        else:
            a = a + t * wq[None]
    assert a.dtype == f32
    return a


def _gather_inputs():
    out = []
    for name in ("s1", "d48", "d288"):
        x = fc.single_inputs(name)
        out.append((name, x["points"], x["calib"], x["feat_lr"], x["feat_hr"]))
    xv = fc.views_inputs(3)
    for v in range(3):
        out.append(("view %d" % v, xv["points"][v], xv["calibs"][v], xv["feats_lr"][v], xv["feats_hr"][v]))
    xs = fc.stack_inputs()
    for s in range(fc.STACKS):
        out.append(("stack %d" % s, xs["points"], xs["calib"], xs["feats_lr"][s], xs["feat_hr"]))
    return out


def test_the_inputs_make_the_gather_exact():
    on = Rounding("fp16")
    for name, pts, calib, fl, fh in _gather_inputs():
        X, Y, Z = fm.project(OFF, pts, calib)
        for a, b in zip((X, Y, Z), fm.project(on, pts, calib)):
            assert np.array_equal(a, b), name                                  # the projection is exact in fp32
        inside = (np.abs(X) <= 1.0) & (np.abs(Y) <= 1.0)
        assert 0 < (~inside).sum() < inside.sum(), name
        assert fl.shape[1:] in ((17, 17), (9, 17)) and fh.shape[1:] in ((65, 65), (33, 65))
        for fmap in (fl, fh):
            want = gc.bilinear(fmap, X, Y)
            assert np.array_equal(want, want.astype(np.float32).astype(np.float64)), name
            for fused in (False, True):
                got = _taps_f32(fmap, X, Y, fused)
                assert np.array_equal(got.astype(np.float64), want), (name, fused)
        assert np.abs(want).max() > 0.5
    assert {tuple(x[3].shape[1:]) for x in _gather_inputs()} == {(17, 17), (9, 17)}      # the non-square maps are among them


# ------------------------------------------------------------------ rounding off
def _rows(feat_lr, feat_hr, points, calib):
    cal4 = np.eye(4)
    cal4[:3] = np.asarray(calib, np.float64).reshape(3, 4)
    rows, mask, _ = gc.point_rows(feat_lr, feat_hr, points, cal4)
    return rows, mask


@pytest.mark.parametrize("name", ALL_SHAPES)
def test_rounding_off_the_model_is_the_classifier(name):
    assert (gc.ZMUL, gc.ZDIV) == (fc.ZMUL, fc.ZDIV)
    sd, x = fc.mlp_sd(name), fc.single_inputs(name)
    got = fm.single(sd, 2, x["points"], x["calib"], fc.ZMUL, fc.ZDIV, x["feat_lr"], x["feat_hr"], rounding=False)
    rows, mask = _rows(x["feat_lr"], x["feat_hr"], x["points"], x["calib"])
    (_, rl), (_, rh) = gc.shapes_of(sd)
    lg_l = gc.mlp_forward(*gc._layers(sd, "mlp_lr."), set(rl), rows)[0]
    q = mask * fm.sigmoid(lg_l)
    lg_h = gc.mlp_forward(*gc._layers(sd, "mlp_hr."), set(rh), np.concatenate([rows, q[None]]))[0]
    assert np.array_equal(got["mask"], mask) and int((mask == 0).sum()) == fc.OUTSIDE
    for tag, want in (("lr", lg_l), ("hr", lg_h)):
        err = np.abs(got["logit_" + tag] - want).max() / np.abs(want).max()
        print("rounding off, %-8s %s: single vs mlp_forward %.2e of the largest logit %.3f" % (name, tag, err, np.abs(want).max()))
        assert err <= 1e-12
    assert np.abs(got["occ_hr"] - mask * fm.sigmoid(lg_h)).max() <= 1e-12
    # the hr classifier alone on a given p_lr: the same numbers
    alone = fm.single(sd, 2, x["points"], x["calib"], fc.ZMUL, fc.ZDIV, x["feat_lr"], x["feat_hr"], p_lr=q, rounding=False)
    assert alone["logit_lr"] is None and np.abs(alone["logit_hr"] - lg_h).max() <= 1e-12 * np.abs(lg_h).max()


def _classifier_views_f64(Ws, bs, res, feature):
    """SurfaceClassifier.forward with num_views = V > 1 on feature [V, C, N] (SurfaceClassifier.py:53-81): the view mean of y and of
    the skip input after layer L // 2 (after its LeakyReLU unless it is the last layer).  Returns the logits [N]."""
    y = tmpy = feature
    L = len(Ws)
    for i in range(L):
        inp = np.concatenate([y, tmpy], -2) if i in res else y
        y = Ws[i] @ inp + bs[i][:, None]
        if i != L - 1:
            y = np.where(y > 0, y, 0.01 * y)
        if i == L // 2:
            y, tmpy = y.mean(0), feature.mean(0)
    assert y.shape[0] == 1
    return y[0]


@pytest.mark.parametrize("name,V", fc.VIEWS)
def test_rounding_off_the_views_model_is_the_reference_formula(name, V):
    sd, x = fc.mlp_sd(name), fc.views_inputs(V)
    got = fm.views(sd, 3, x["points"], x["calibs"], fc.ZMUL, fc.ZDIV, x["feats_lr"], x["feats_hr"], rounding=False)
    per_view = [_rows(x["feats_lr"][v], x["feats_hr"][v], x["points"][v], x["calibs"][v]) for v in range(V)]
    rows, mask = np.stack([r for r, _ in per_view]), np.stack([m for _, m in per_view])
    (_, rl), (_, rh) = gc.shapes_of(sd)
    lg_l = _classifier_views_f64(*gc._layers(sd, "mlp_lr."), set(rl), rows)
    q = mask * fm.sigmoid(lg_l)[None]
    lg_h = _classifier_views_f64(*gc._layers(sd, "mlp_hr."), set(rh), np.concatenate([rows, q[:, None]], 1))
    assert np.array_equal(got["mask"], mask)
    for tag, want in (("lr", lg_l), ("hr", lg_h)):
        err = np.abs(got["logit_" + tag] - want).max() / np.abs(want).max()
        print("rounding off, %-4s V = %d %s: views vs the formula %.2e of the largest logit %.3f" % (name, V, tag, err, np.abs(want).max()))
        assert err <= 1e-12
    assert np.abs(got["occ_lr"] - q).max() <= 1e-12 and got["occ_hr"].shape == (V, fc.N)


# ------------------------------------------------------------------ the fp32-grade claim
@pytest.mark.parametrize("name", ALL_SHAPES)
def test_fp32_grade_parts_measured(name):
    sd, x = fc.mlp_sd(name), fc.single_inputs(name)
    args = (x["points"], x["calib"], fc.ZMUL, fc.ZDIV, x["feat_lr"], x["feat_hr"])
    exact = fm.single(sd, 2, *args, rounding=False)
    err = {}
    for NP in (2, 3):
        got = fm.single(sd, NP, *args)
        err[NP] = max(np.abs(got["logit_" + tag] - exact["logit_" + tag]).max() for tag in ("lr", "hr"))
    print("%-8s max |model - unrounded model| on the logits: two f16 parts %.3e, three bf16 parts %.3e" % (name, err[2], err[3]))
    assert err[3] <= err[2] < 1e-4


# ------------------------------------------------------------------ the bound separates wrong models
def _ratios(ref, forms, pert, tag):
    """(dev mean / e mean, dev max / e max, dev median / its bound, the statistics that break their bound)."""
    bound, e, sel = fm.logit_bounds(ref, forms, tag)
    dev = np.abs(pert["logit_" + tag] - ref["logit_" + tag])[sel]
    return dev.mean() / e.mean(), dev.max() / e.max(), np.median(dev) / bound["median"], fm.breaks(dev, bound)


def _report(name, NP, what, got):
    print("%-4s NP = %d (%s): lr mean %.1fx max %.1fx of e_model, median %.2fx of its bound, breaks %s; hr mean %.1fx max %.1fx, median "
          "%.2fx, breaks %s" % ((name, NP, what) + got["lr"] + got["hr"]))


DROPPED = {2: [(1, 0)], 3: [(2, 0), (1, 1), (0, 2)]}


@pytest.mark.parametrize("NP", [1, 2, 3])
@pytest.mark.parametrize("name", ["s1", "odd"])
def test_the_bound_separates_wrong_models(name, NP):
    sd, x = fc.mlp_sd(name), fc.single_inputs(name)
    ref, forms = fc.single_models(name, NP)
    for tag in ("lr", "hr"):
        assert not _ratios(ref, forms, forms[0], tag)[3]                 # the bound holds for what it has to let through
    ragged = [l for l, d in enumerate(fm.Net(sd, 0).dims[:-1]) if d % fm.KT]
    # odd: 1000 -> 1024, 500 -> 512, 250 -> 256, 100 -> 128; the features 321 -> 352 in both
    assert ragged == ([0, 1, 2, 3, 4] if name == "odd" else [0])
    perts = [("a truncated first part of the activations", {"trunc_act": True})]
    perts += [("b last k-step of layer %d's k1 segment missing" % l, {"drop_kstep": (0, l)}) for l in ragged]
    perts += [("c z_feat and p_lr swapped in the skip segments", {"swap_skip": True}), ("d layer 1's bias through 16 bits", {"bias16": (0, 1)})]
    if NP > 1:
        perts.append(("e products %s missing" % DROPPED[NP], {"drop_products": DROPPED[NP]}))
    for what, pert in perts:
        out = fm.single(sd, NP, x["points"], x["calib"], fc.ZMUL, fc.ZDIV, x["feat_lr"], x["feat_hr"], pert=pert)
        got = {tag: _ratios(ref, forms, out, tag) for tag in ("lr", "hr")}
        _report(name, NP, what, got)
        if what[0] == "a" and NP > 1:
            # what the bound cannot see: the second part picks up what the truncated first part leaves
            assert not got["lr"][3] and got["lr"][0] < 1.0 and got["lr"][1] < 1.0, (what, got)
        else:
            assert got["lr"][3], (what, got)


@pytest.mark.parametrize("NP", [1, 2, 3])
@pytest.mark.parametrize("name", ["s1", "odd"])
def test_the_bound_separates_wrong_views_models(name, NP):
    sd, x = fc.mlp_sd(name), fc.views_inputs(2)
    ref, forms = fc.views_models(name, 2, NP)
    one_view_only = ref["mask"][0] != ref["mask"][1]
    assert one_view_only.sum() >= 20                                     # (g) needs points inside one view and outside the other
    for tag in ("lr", "hr"):
        assert not _ratios(ref, forms, forms[0], tag)[3]
    for what, pert, tag in (("f layer M summed before its LeakyReLU", {"sum_pre_lrelu": True}, "lr"),
                            ("g the hr row's p_lr without the view's mask", {"plr_unmasked": True}, "hr")):
        out = fm.views(sd, NP, x["points"], x["calibs"], fc.ZMUL, fc.ZDIV, x["feats_lr"], x["feats_hr"], pert=pert)
        got = {t: _ratios(ref, forms, out, t) for t in ("lr", "hr")}
        _report(name, NP, "V = 2, " + what, got)
        assert got[tag][3], (what, got)
        if what[0] == "g":
            moved = out["logit_hr"] != ref["logit_hr"]
            assert moved[one_view_only].all() and not moved[ref["mask"].min(0) == 1].any()   # only points outside some view move


def test_stacks_model_leaves_the_occupancy_comparison_few_points():
    """Case E recovers the logit from the stored occupancy where the model's |logit| < column_model.SAT: the model alone must leave
    at most 1 % of the compared points to the occupancy comparison for the chosen seed."""
    from column_model import SAT
    for s in range(fc.STACKS):
        ref = fc.stack_models(s)[0]
        inimg = ref["mask"] > 0
        for tag in ("lr", "hr"):
            share = (np.abs(ref["logit_" + tag][inimg]) >= SAT).mean()
            print("stack %d %s: %.2f %% of the in-image points at |logit| >= %g" % (s, tag, 100.0 * share, SAT))
            assert share <= 0.01
