"""The fused classifier evaluator (csrc/surs_mlp_fused.inc, surs_mlp_fused_views.inc, surs_mlp_fused_stacks.inc of the package) held
to tests/fused_model.py: a float64 model that rounds where the kernels' sources round and forms the partial products they form.  A
correct kernel differs from it by accumulation order only, so the tolerance is the model's own distance to itself accumulating in
fp32 (both k orders) - not the 4e-3 / 1e-4 of the parity tests, which hide a truncating conversion, a lost k-step, a swapped feature
slot, a bias through 16 bits or a missing partial product (tests/test_fused_model_host.py shows that this bound catches them).

Per case, operand split (parts = 1: one f16 product per MAC, 2: two f16 parts, 3: three bf16 parts) and classifier, over all points:
    dev = |kernel logit - float64 model logit|,   e = |fp32-accumulating model - float64 model| (the larger of the two k orders),
    floor = 2^-22 max |logit| (logits straight from the library),
    s(dev) <= 8 max(s(e), s(floor))   for s = mean, max, median   (column_model.bounds; 8 = FACTOR),
the occupancies are exact zeros exactly where the model's mask is 0 and within 2^-22 of the sigmoid of their own logit elsewhere.
Every test prints mean(dev) / mean(e), max(dev) / max(e) and median(dev) over its bound.  In cases A, B and D the hr classifier runs on
the kernel's own lr occupancy while the model uses its own; case C gives the hr kernel the model's.

Cases (tests/fused_cases.py; 777 points, seven outside the image: 24 tiles of 32 or 48 of 16 and a ragged 9; weights
weights.synthetic_state_dict(opt, seed=0) of each shape's flags; inputs on which the fp32 gather is exact):
  A  single view, parts 1 2 3: s1 (P = 32), odd (ragged k1), deep and the released shape packed generically (P = 16), res0 (a skip at
     layer 0), l1 (one layer: the only GEMM is the last layer), nores, mixed (different lr and hr shapes);
  B  --hg_dim 48 and 288 (mlp_anyd_kernel: the wave-per-point gather, a run-time feature stride; gen_c0pad 128 and 384) on 9 x 17 and
     33 x 65 maps, parts 1 2 3;
  C  the hr classifier alone (p_lr = the model's lr occupancy as fp32), s1, parts 1 2;
  D  views, parts 1 2 3: s1 and odd at V = 2, l1 at V = 3 (M = L - 1 = 0: the mean is taken of the logits), l2 at V = 2 (M = L - 1 = 1:
     layer 0 per view, the mean of the logits); points inside one view and outside another;
  E  stacks, parts 1: s1 on three lr maps through native.query_points_generic_stacks, which returns occupancies: the logit is
     recovered where the model's |logit| < column_model.SAT, floor 4 * 2^-24 / (p (1 - p)) as for the grids of
     tests/test_gpu_column_model.py; at most 1 % of the compared points may be left to the occupancy comparison."""
import numpy as np
import pytest
import torch

import column_model as cm
import fused_cases as fc
import fused_model as fm

pytestmark = pytest.mark.gpu

_dev = {}


def packed(name):
    import gpu_common as g
    from surs_amd import native
    if ("gm", name) not in _dev:
        sd = fc.mlp_sd(name)
        _dev[("gm", name)] = native.pack_mlp_generic(sd, g.dev(), native.mlp_shapes(sd, fc.opt(name)))
    return _dev[("gm", name)]


def with_parts(parts, fn, *args, **kw):
    from surs_amd import native
    native.check(native.lib().surs_set_operand_split_local(parts))
    try:
        outs = fn(*args, **kw)
    finally:
        native.check(native.lib().surs_set_operand_split_local(0))
    return [None if o is None else o.cpu().numpy() for o in outs]


def hold(name, tag, ref, forms, logit=None, occ=None):
    """Assert the bound for classifier tag: logit [N] straight from the library, or occ [N] as the kernel stored it (stacks)."""
    want = ref["logit_" + tag]
    if logit is not None:
        got = np.asarray(logit, np.float64)
        assert got.shape == want.shape and np.isfinite(got).all()
        bound, e, sel = fm.logit_bounds(ref, forms, tag)
        got, share, sat = got[sel], 0.0, None
    else:
        inimg = ref["mask"] > 0
        sat = inimg & (np.abs(want) >= cm.SAT)
        sel = inimg & ~sat
        share = sat.sum() / max(1, inimg.sum())
        occ = np.asarray(occ, np.float64)
        assert occ.shape == want.shape and np.isfinite(occ).all()
        assert np.array_equal(occ == 0.0, ~inimg), "%s %s: zero sets differ" % (name, tag)
        assert (occ[sel] > 0.0).all() and (occ[sel] < 1.0).all()
        got = np.log(occ[sel] / (1.0 - occ[sel]))
        bound, e = cm.bounds(ref, forms, tag, sel)
    dev = np.abs(got - want[sel])
    print("%-26s %s: mean(dev) / mean(e) = %6.3f   max(dev) / max(e) = %6.3f   median(dev) / its bound = %5.3f   (dev mean %.3g max "
          "%.3g median %.3g; bounds %.3g %.3g %.3g; %d points, %.2f %% saturated)"
          % (name, tag, dev.mean() / e.mean(), dev.max() / e.max(), np.median(dev) / bound["median"], dev.mean(), dev.max(),
             np.median(dev), bound["mean"], bound["max"], bound["median"], int(sel.sum()), 100.0 * share))
    assert share <= 0.01, (name, tag, share)
    assert not fm.breaks(dev, bound), (name, tag, fm.breaks(dev, bound))
    if sat is not None and sat.any():
        dp = np.abs(occ[sat] - ref["occ_" + tag][sat]).max()
        assert dp <= 0.0067 * bound["max"] + 2.0 ** -22, (name, tag, "saturated", dp)


def occupancy_of_own_logit(name, mask, occ, logit):
    """Exact zeros exactly where the mask is 0; elsewhere the sigmoid of the logit it came with (four fp32 roundings)."""
    occ, inimg = np.asarray(occ, np.float64), mask > 0
    assert np.array_equal(occ == 0.0, ~inimg), name
    s = np.broadcast_to(cm.sigmoid(np.asarray(logit, np.float64)), occ.shape)
    assert np.abs(occ - s)[inimg].max() <= 2.0 ** -22, name


def single_inputs_on_device(name):
    import gpu_common as g
    if ("in", name) not in _dev:
        x = fc.single_inputs(name)
        _dev[("in", name)] = (torch.from_numpy(x["points"]).to(g.dev()), x["calib"], g.upload_nhwc(x["feat_lr"]), g.upload_nhwc(x["feat_hr"]))
    return _dev[("in", name)]


def run_single(name, parts, p_lr=None):
    from surs_amd import native
    pts, calib, Fl, Fh = single_inputs_on_device(name)
    pl = None if p_lr is None else torch.from_numpy(np.ascontiguousarray(p_lr, np.float32)).to(pts.device)
    return with_parts(parts, native.query_points_generic, pts, calib, fc.ZMUL, fc.ZDIV, Fl, Fh, packed(name), p_lr=pl, want_logits=True)


def check_single(case, name, parts):
    ref, forms = fc.single_models(name, parts)
    assert int((ref["mask"] == 0).sum()) == fc.OUTSIDE
    phr, plr, lhr, llr = run_single(name, parts)
    label = "%s %s parts %d" % (case, name, parts)
    for tag, occ, lg in (("lr", plr, llr), ("hr", phr, lhr)):
        hold(label, tag, ref, forms, logit=lg)
        occupancy_of_own_logit((label, tag), ref["mask"], occ, lg)


# ------------------------------------------------------------------ A
TILE_POINTS = {"s1": 32, "odd": 16, "deep": 16, "released": 16, "res0": 16, "nores": 16, "l1": 32, "mixed": 16}


@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("name", fc.SINGLE)
def test_single_view_against_the_model(name, parts):
    if parts == 1:
        from surs_amd import native
        assert packed(name).info()[0] == TILE_POINTS[name]              # both tile sizes are among the shapes
        assert native.is_default_mlp(packed(name).shapes) == (name == "released")
    check_single("A", name, parts)


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("name", fc.HG_DIM)
def test_other_hg_dim_against_the_model(name, parts):
    from surs_amd import native
    x = fc.single_inputs(name)
    assert native.mlp_hg_dim(packed(name).shapes) == fc.hg_dim(name) != 256
    assert fm.c0pad(fc.hg_dim(name)) == {"d48": 128, "d288": 384}[name]
    assert x["feat_lr"].shape == (fc.hg_dim(name), 9, 17) and x["feat_hr"].shape == (64, 33, 65)      # the non-square maps
    check_single("B", name, parts)


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("parts", [1, 2])
def test_hr_alone_on_the_models_lr_occupancy(parts):
    p_lr, (ref, forms) = fc.hr_alone_models("s1", parts)
    phr, plr, lhr, llr = run_single("s1", parts, p_lr=p_lr)
    assert llr is None and np.array_equal(plr, p_lr)
    label = "C s1 parts %d" % parts
    hold(label, "hr", ref, forms, logit=lhr)
    occupancy_of_own_logit(label, ref["mask"], phr, lhr)


# ------------------------------------------------------------------ D
def views_inputs_on_device(V):
    import gpu_common as g
    if ("views", V) not in _dev:
        x = fc.views_inputs(V)
        nhwc = lambda maps: torch.from_numpy(np.ascontiguousarray(np.stack(maps).transpose(0, 2, 3, 1))).to(g.dev())
        _dev[("views", V)] = (torch.from_numpy(x["points"]).to(g.dev()), x["calibs"], nhwc(x["feats_lr"]), nhwc(x["feats_hr"]))
    return _dev[("views", V)]


@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("name,V", fc.VIEWS)
def test_views_against_the_model(name, V, parts):
    from surs_amd import native
    ref, forms = fc.views_models(name, V, parts)
    mask = ref["mask"]
    assert mask.shape == (V, fc.N) and ((mask.min(0) == 0) & (mask.max(0) == 1)).sum() >= 20      # inside one view, outside another
    pts, calibs, fl, fh = views_inputs_on_device(V)
    phr, plr, lhr, llr = with_parts(parts, native.query_points_generic_views, pts, calibs, fc.ZMUL, fc.ZDIV, fl, fh, packed(name),
                                    want_logits=True)
    label = "D %s V = %d parts %d" % (name, V, parts)
    for tag, occ, lg in (("lr", plr, llr), ("hr", phr, lhr)):
        assert occ.shape == (V, fc.N) and lg.shape == (fc.N,)
        hold(label, tag, ref, forms, logit=lg)
        occupancy_of_own_logit((label, tag), mask, occ, lg)          # a view's occupancy is 0 exactly where that view's mask is 0


# ------------------------------------------------------------------ E
def test_stacks_against_the_single_map_model():
    import gpu_common as g
    from surs_amd import native
    x = fc.stack_inputs()
    pts = torch.from_numpy(x["points"]).to(g.dev())
    Fls, Fh = [g.upload_nhwc(f) for f in x["feats_lr"]], g.upload_nhwc(x["feat_hr"])
    phr, plr = with_parts(1, native.query_points_generic_stacks, pts, x["calib"], fc.ZMUL, fc.ZDIV, Fls, Fh, packed("s1"))
    assert phr.shape == plr.shape == (fc.STACKS, fc.N)
    for s in range(fc.STACKS):
        ref, forms = fc.stack_models(s)
        hold("E s1 stack %d parts 1" % s, "lr", ref, forms, occ=plr[s])
        hold("E s1 stack %d parts 1" % s, "hr", ref, forms, occ=phr[s])
    assert not np.array_equal(plr[0], plr[1]) and not np.array_equal(plr[1], plr[2])
