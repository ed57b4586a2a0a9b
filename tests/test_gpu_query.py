"""GPU parity of the point evaluator (through the C ABI) against the reference's golden outputs and the oracle.
Tolerances: fp32 mode 1e-4 on occupancies and pre-sigmoid logits (BASELINE.json north_star);
bf16 / fp16 grid mode has its own, looser bound, stated per test."""
import os

import numpy as np
import pytest
import torch

import common

pytestmark = pytest.mark.gpu

ZMUL, ZDIV = 1024 // 2, 200.0


@pytest.fixture(scope="module")
def setup():
    import gpu_common as g
    from surs_amd import native
    fl, fh = common.synth_features()
    return dict(g=g, native=native, fl=fl, fh=fh, Fl=g.upload_nhwc(fl), Fh=g.upload_nhwc(fh), ws=native.Workspace(g.dev()))


def _q(s, pts, calib):
    nat = s["native"]
    p = torch.from_numpy(np.ascontiguousarray(pts)).to(s["g"].dev())
    outs = nat.query_points(p, np.asarray(calib, np.float32).reshape(-1)[:12], ZMUL, ZDIV, s["Fl"], s["Fh"],
                            s["g"].blob("bf16"), s["ws"], want_logits=True)
    return [o.cpu().numpy() for o in outs]


def test_query_50k_vs_reference(setup, golden_dir):
    from surs_amd import weights
    g = np.load(os.path.join(golden_dir, "query.npz"))
    phr, plr, lhr, llr = _q(setup, weights.synthetic_points(50000, seed=2), common.CALIB)
    assert np.abs(phr - g["a_pred_hr"]).max() < 1e-4
    assert np.abs(plr - g["a_pred_lr"]).max() < 1e-4
    assert np.abs(lhr - g["a_logit_hr"]).max() < 1e-4
    assert np.abs(llr - g["a_logit_lr"]).max() < 1e-4
    assert ((phr == 0) == (g["a_pred_hr"] == 0)).all()


def test_query_50k_full_size_features_vs_reference(setup_full, golden_dir):
    """BASELINE configs[1] as stated: 50 000 random points, fp32, feature maps of the 512 x 512 input's sizes (256 x 256^2,
    64 x 1024^2), against the reference's outputs (tests/golden/query_h512.npz): 1e-4 on occupancies and logits."""
    from surs_amd import weights
    g = np.load(os.path.join(golden_dir, "query_h512.npz"))
    phr, plr, lhr, llr = _q(setup_full, weights.synthetic_points(50000, seed=2), common.CALIB)
    assert np.abs(phr - g["pred_hr"]).max() < 1e-4 and np.abs(plr - g["pred_lr"]).max() < 1e-4
    assert np.abs(lhr - g["logit_hr"]).max() < 1e-4 and np.abs(llr - g["logit_lr"]).max() < 1e-4
    assert ((phr == 0) == (g["pred_hr"] == 0)).all()


def test_query_50k_full_size_features_one_product_path(setup_full, golden_dir):
    """The one-product point path (surs_set_operand_split_local(1): one f16 part per operand) on BASELINE configs[1]'s points over
    full-size feature maps, against the reference's outputs (tests/golden/query_h512.npz) at the fp16 bound of the column kernels
    (4e-3 on the occupancies); the fp32-grade test above is untouched by it."""
    from surs_amd import native, weights
    g = np.load(os.path.join(golden_dir, "query_h512.npz"))
    with native.reduced_point_operands():
        phr, plr, lhr, llr = _q(setup_full, weights.synthetic_points(50000, seed=2), common.CALIB)
    eh, el = np.abs(phr - g["pred_hr"]).max(), np.abs(plr - g["pred_lr"]).max()
    print("one-product point path, full-size features: max |d occupancy| hr %.3e lr %.3e; max |d logit| hr %.3e" % (eh, el, np.abs(lhr - g["logit_hr"]).max()))
    assert 1e-6 < eh < 4e-3 and el < 4e-3
    assert ((phr == 0) == (g["pred_hr"] == 0)).all()
    phr2, plr2, _, _ = _q(setup_full, weights.synthetic_points(50000, seed=2), common.CALIB)     # (outside: fp32-grade again)
    assert np.abs(phr2 - g["pred_hr"]).max() < 1e-4 and np.abs(plr2 - g["pred_lr"]).max() < 1e-4


def test_query_general_calib_ragged_and_edges(setup, golden_dir):
    from surs_amd import weights
    g = np.load(os.path.join(golden_dir, "query.npz"))
    phr, plr, lhr, llr = _q(setup, weights.synthetic_points(4099, seed=5), g["b_calib"])
    assert np.abs(phr - g["b_pred_hr"]).max() < 1e-4 and np.abs(plr - g["b_pred_lr"]).max() < 1e-4
    assert np.abs(lhr - g["b_logit_hr"]).max() < 2e-4
    phr, plr, _, _ = _q(setup, g["c_points"], common.CALIB)
    assert np.abs(phr - g["c_pred_hr"]).max() < 1e-4 and np.abs(plr - g["c_pred_lr"]).max() < 1e-4
    assert phr[5] == 0 and phr[6] == 0 and phr[0] > 0
    # single point and empty input
    one = _q(setup, g["c_points"][:, :1], common.CALIB)
    assert abs(one[0][0] - g["c_pred_hr"][0]) < 1e-4
    empty = _q(setup, np.zeros((3, 0), np.float32), common.CALIB)
    assert empty[0].shape == (0,)


def _grid(s, R, dtype, i0=0, i1=None):
    import oracle
    nat = s["native"]
    mat = oracle.coords_matrix(R, [-0.5] * 3, [0.5] * 3)
    i1 = R if i1 is None else i1
    vh, vl = nat.query_grid(i0, i1, R, R, mat[:3].reshape(-1), common.CALIB.reshape(-1)[:12], ZMUL, ZDIV, s["Fl"], s["Fh"],
                            s["g"].blob("f16" if dtype == "fp16" else "bf16"), dtype, s["ws"])
    return vh.cpu().numpy(), vl.cpu().numpy()


def test_grid_fp32_vs_oracle(setup):
    import oracle
    R = 24
    vh, vl = _grid(setup, R, "fp32")
    pts = oracle.grid_points(R, [-0.5] * 3, [0.5] * 3)
    phr, plr = oracle.query(common.state_dict(), pts, common.CALIB, setup["fl"], setup["fh"], 1024, 200.0)
    assert np.abs(vh.reshape(-1) - phr).max() < 1e-4
    assert np.abs(vl.reshape(-1) - plr).max() < 1e-4


@pytest.mark.parametrize("dtype,tol", [("bf16", 3e-2), ("fp16", 4e-3)])
def test_grid_column_kernel_vs_fp32(setup, dtype, tol):
    """Reduced-precision column kernel vs the fp32 path on the same grid (ragged R: 40 is not a multiple of the
    128-voxel z tile, and 40*40 columns is not a multiple of the column batch)."""
    R = 40
    vh32, vl32 = _grid(setup, R, "fp32")
    vh, vl = _grid(setup, R, dtype)
    eh, el = np.abs(vh - vh32).max(), np.abs(vl - vl32).max()
    print("column kernel %s: max|d| hr %.3e lr %.3e, mean|d| hr %.3e" % (dtype, eh, el, np.abs(vh - vh32).mean()))
    assert eh < tol and el < tol
    # slab consistency: evaluating [i0,i1) separately gives identical bits (multi-GPU sharding property)
    a, _ = _grid(setup, R, dtype, 8, 24)
    assert np.array_equal(a, vh[8:24])


@pytest.fixture(scope="module")
def setup_full():
    """BASELINE's feature-map sizes (512 x 512 input): im_feat_lr 256 x 256^2, im_feat_hr 64 x 1024^2, PRNG values."""
    import gpu_common as g
    from surs_amd import native
    fl, fh = common.synth_features(seed=7, hl=256, hh=1024)
    s = dict(g=g, native=native, Fl=g.upload_nhwc(fl), Fh=g.upload_nhwc(fh), ws=native.Workspace(g.dev()))
    del fl, fh
    return s


@pytest.mark.parametrize("dtype,tol,tol_logit", [("fp32", 2e-5, 1e-4), ("bf16", 3e-2, None), ("fp16", 4e-3, None)])
def test_full_size_sweep_properties(setup_full, dtype, tol, tol_logit):
    """BASELINE's full grid (512^3 = 134 217 728 queries) over full-size feature maps, every precision of the column
    kernels (the defaults: fp32 = v11, bf16 / fp16 = v10), through properties that do not need a CPU pass over the grid: (1) four flat
    ranges of 65 536 voxels - a plane boundary, a slab boundary of the sweep and two interior ones - against the fp32 point
    evaluator on the oracle's coordinates for those voxels (the point evaluator is itself held to the reference's goldens
    at 1e-4); for fp32 also in logit space, at the north star's 1e-4; (2) the same bits on a second run; (3) slab
    consistency: planes [200, 296) evaluated on their own equal those planes of the full sweep."""
    import oracle
    R = 512
    s, nat = setup_full, setup_full["native"]
    mat = oracle.coords_matrix(R, [-0.5] * 3, [0.5] * 3)[:3].reshape(-1)
    cal = common.CALIB.reshape(-1)[:12]
    dev = s["g"].dev()
    blob = s["g"].blob("f16" if dtype == "fp16" else "bf16")
    vh = torch.empty((R, R, R), dtype=torch.float32, device=dev)
    vl = torch.empty_like(vh)
    nat.query_grid(0, R, R, R, mat, cal, ZMUL, ZDIV, s["Fl"], s["Fh"], blob, dtype, s["ws"], vh, vl)
    n = 65536
    lg = lambda p: torch.log(p.double() / (1.0 - p.double()))
    for start in (0, 31 * R * R + 509 * R - 7, 32 * R * R - n // 2, R ** 3 - n):
        pts = torch.from_numpy(oracle.grid_points(R, [-0.5] * 3, [0.5] * 3, start, start + n)).to(dev)
        phr, plr, lhr, llr = nat.query_points(pts, cal, ZMUL, ZDIV, s["Fl"], s["Fh"], blob, s["ws"], want_logits=True)
        a, b = vh.view(-1)[start:start + n], vl.view(-1)[start:start + n]
        eh, el = (a - phr).abs().max().item(), (b - plr).abs().max().item()
        assert eh < tol and el < tol, (start, eh, el)
        if tol_logit is not None:
            ok = (a > 1e-4) & (a < 1 - 1e-4) & (b > 1e-4) & (b < 1 - 1e-4)
            dh, dl = (lg(a) - lhr.double()).abs()[ok].max().item(), (lg(b) - llr.double()).abs()[ok].max().item()
            assert dh < tol_logit and dl < tol_logit, (start, dh, dl)
    vh2 = torch.empty_like(vh)
    vl2 = torch.empty_like(vl)
    nat.query_grid(0, R, R, R, mat, cal, ZMUL, ZDIV, s["Fl"], s["Fh"], blob, dtype, s["ws"], vh2, vl2)
    assert torch.equal(vh, vh2) and torch.equal(vl, vl2)
    nat.query_grid(200, 296, R, R, mat, cal, ZMUL, ZDIV, s["Fl"], s["Fh"], blob, dtype, s["ws"], vh2[200:296].zero_(), vl2[200:296].zero_())
    assert torch.equal(vh[200:296], vh2[200:296]) and torch.equal(vl[200:296], vl2[200:296])
    assert float(vh.min()) >= 0.0 and float(vh.max()) <= 1.0 and bool(torch.isfinite(vh).all())


def test_grid_fp32_column_kernel_vs_layer_kernels(setup):
    """surs_query_grid(SURS_F32) on an axis-aligned sweep runs the fp32-grade column kernel (v11: split-f16 operands, three
    MFMA products per MAC); on a general calibration it runs the per-point layer kernels (split-bf16, six products).  Both
    are fp32-grade: the same grid through both, occupancies within 2e-6 and logits within 2e-5 of each other (ragged R)."""
    import oracle
    nat = setup["native"]
    R = 40
    vh, vl = _grid(setup, R, "fp32")
    pts = torch.from_numpy(oracle.grid_points(R, [-0.5] * 3, [0.5] * 3)).to(setup["g"].dev())
    phr, plr, lhr, llr = nat.query_points(pts, common.CALIB.reshape(-1)[:12], ZMUL, ZDIV, setup["Fl"], setup["Fh"],
                                          setup["g"].blob("bf16"), setup["ws"], want_logits=True)
    a, b = torch.from_numpy(vh.reshape(-1)).to(pts.device), torch.from_numpy(vl.reshape(-1)).to(pts.device)
    lg = lambda p: torch.log(p.double() / (1.0 - p.double()))
    assert (a - phr).abs().max().item() < 2e-6 and (b - plr).abs().max().item() < 2e-6
    assert (lg(a) - lhr.double()).abs().max().item() < 2e-5 and (lg(b) - llr.double()).abs().max().item() < 2e-5
    # a general calibration (rotated about x: the projected Y depends on k) takes the layer kernels and agrees with the
    # point path bit for bit (same kernels, same batches of 65 536)
    c, s_ = np.cos(0.3), np.sin(0.3)
    calib = (np.array([[1, 0, 0, 0], [0, c, -s_, 0], [0, s_, c, 0], [0, 0, 0, 1]], np.float32) @ common.CALIB).astype(np.float32)
    mat = oracle.coords_matrix(R, [-0.5] * 3, [0.5] * 3)
    gh, gl = nat.query_grid(0, R, R, R, mat[:3].reshape(-1), calib.reshape(-1)[:12], ZMUL, ZDIV, setup["Fl"], setup["Fh"],
                            setup["g"].blob("bf16"), "fp32", setup["ws"])
    phr, plr = nat.query_points(pts, calib.reshape(-1)[:12], ZMUL, ZDIV, setup["Fl"], setup["Fh"], setup["g"].blob("bf16"), setup["ws"])
    assert torch.equal(gh.view(-1)[:65536], phr[:65536]) and torch.equal(gl.view(-1)[:65536], plr[:65536])


def test_restated_kernels_match_dense_kernel(tmp_path):
    """The restated column kernels (layer 1 as a per-column affine part + the residuals of the listed channels: v10 on eight
    waves, v12 streamed on two workgroups per CU; R = 40 runs several chunks per tile) against the dense-layer-1 kernel v3 on the same inputs, each in
    its own process selected by SURS_GRID_KERNEL: <= 4e-3 on the occupancies (v3 rounds every layer-0 activation to 16 bits,
    the restated kernels carry the affine part at fp32 grade).  Every launch of a kernel must reproduce its own bits
    (three launches per size: race screen), for ragged and multi-tile grids."""
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    ref = str(tmp_path / "v3.npz")
    for ver, mode in (("3", "save"), ("10", "cmp"), ("12", "cmp")):
        env = dict(os.environ, SURS_GRID_KERNEL=ver)
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "gpu_grid_cmp.py"), mode, ref], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        st = [l for l in lines if l.startswith(("bf16 ", "fp16 "))]
        assert len(st) == 4 and all("stable finite" in l for l in st), (ver, st)
        if mode == "save":
            continue
        diffs = {l.split()[0]: float(l.split("=")[1].split()[0]) for l in lines if "max|diff|" in l}
        assert len(diffs) == 8, lines
        for k, d in diffs.items():
            assert d <= 4e-3, (ver, k, d)


def test_operand_splits_agree(tmp_path):
    """The fp32 point path's layer kernel takes its operands as two f16 parts (default) or three bf16 parts (SURS_SPLIT=bf16x3).
    The logits of the two splits differ by the 22- / 24-bit operand split and the number of products: <= 2e-5."""
    import subprocess
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    ref = str(tmp_path / "bf16x3.npz")
    for name, extra, mode in (("bf16x3", {"SURS_SPLIT": "bf16x3"}, "save"), ("f16x2", {}, "cmp")):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "gpu_points_cmp.py"), mode, ref],
                           env=dict(os.environ, **extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        if mode == "save":
            continue
        lines = [l for l in r.stdout.splitlines() if "max|diff|" in l]
        assert len(lines) == 10, r.stdout   # 2 batch sizes x 4 outputs + the two fields of a small bf16 sweep
        for l in lines:
            d = float(l.split("=")[1].split()[0])
            # (the sweep's column constants go through the same kernel; behind them sits the bf16 column kernel, which
            #  rounds the layer-0 activations to bf16: a constant that differs in the last fp32 bit can flip one of those)
            assert d <= (2e-5 if not l.startswith("grid_") else 2e-3), (name, l)


def test_multiview_and_perspective_vs_reference(setup, golden_dir):
    """num_views = 2 (orthogonal) and 3 (perspective) through surs_query_points_views against the outputs of the
    reference's own multi-view path (tests/golden/query_views.npz): 1e-4 on occupancies and logits."""
    from surs_amd import weights
    nat, gg = setup["native"], setup["g"]
    g = np.load(os.path.join(golden_dir, "query_views.npz"))
    for tag, V, proj, n in (("o2", 2, "orthogonal", 3001), ("p3", 3, "perspective", 2050)):
        fl = np.stack([common.synth_features(seed=10 + v)[0] for v in range(V)])
        fh = np.stack([common.synth_features(seed=10 + v)[1] for v in range(V)])
        Fl = torch.from_numpy(np.ascontiguousarray(fl.transpose(0, 2, 3, 1))).to(gg.dev())
        Fh = torch.from_numpy(np.ascontiguousarray(fh.transpose(0, 2, 3, 1))).to(gg.dev())
        pts = weights.synthetic_points(n, seed=20 + V)
        P = torch.from_numpy(np.ascontiguousarray(np.repeat(pts[None], V, 0))).to(gg.dev())
        outs = nat.query_points_views(P, g[tag + "_calibs"].reshape(V, -1)[:, :12], proj, ZMUL, ZDIV, Fl, Fh, gg.blob("bf16"),
                                      setup["ws"], want_logits=True)
        for name, o in zip(("pred_hr", "pred_lr", "logit_hr", "logit_lr"), outs):
            o = o.cpu().numpy()
            assert o.shape == g[tag + "_" + name].shape, (tag, name)
            assert np.abs(o - g[tag + "_" + name]).max() < 1e-4, (tag, name, np.abs(o - g[tag + "_" + name]).max())


def test_multiview_single_view_equals_plain_query(setup):
    """V = 1, orthogonal through the multi-view entry point: the same kernels in the same order as surs_query_points."""
    from surs_amd import weights
    nat, gg = setup["native"], setup["g"]
    pts = weights.synthetic_points(4099, seed=5)
    a = _q(setup, pts, common.CALIB)
    Fl = torch.from_numpy(np.ascontiguousarray(setup["fl"].transpose(1, 2, 0)[None])).to(gg.dev())
    Fh = torch.from_numpy(np.ascontiguousarray(setup["fh"].transpose(1, 2, 0)[None])).to(gg.dev())
    P = torch.from_numpy(np.ascontiguousarray(pts[None])).to(gg.dev())
    b = nat.query_points_views(P, common.CALIB.reshape(1, -1)[:, :12], "orthogonal", ZMUL, ZDIV, Fl, Fh, gg.blob("bf16"),
                               setup["ws"], want_logits=True)
    for x, y in zip(a, (b[0][0], b[1][0], b[2], b[3])):
        assert np.array_equal(x, y.cpu().numpy())


def test_restated_layer1_kernel_is_closer_to_fp32_than_dense_kernel(setup):
    """Column kernel v10 (layer 1 restated; the default) against v3 (dense layer 1) and the fp32-grade sweep on the same grid: v10's affine part
    of layer 1 is fp32-grade, so its logits sit closer to the fp32 sweep than v3's in the mean, and it reproduces its own bits.
    Also a sweep whose z tiles span the whole depth range (R = 24: most channels change branch inside the tile, ten chunks)
    and the profile counter of the residual k-steps."""
    import ctypes as C
    import oracle
    from surs_amd import _lib
    nat, g = setup["native"], setup["g"]
    L = _lib.lib()
    lg = lambda p: torch.log(p.double() / (1 - p.double()))
    try:
        for R in (24, 96):
            mat = oracle.coords_matrix(R, [-0.5] * 3, [0.5] * 3)[:3].reshape(-1)
            cal = common.CALIB.reshape(-1)[:12]
            ref = nat.query_grid(0, R, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], g.blob("bf16"), "fp32", setup["ws"])
            ref = [v.clone() for v in ref]
            err = {}
            for prec, blob in (("bf16", g.blob("bf16")), ("fp16", g.blob("f16"))):
                for kv in (3, 10):
                    L.surs_set_grid_kernel(kv)
                    a = [v.clone() for v in nat.query_grid(0, R, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], blob, prec, setup["ws"])]
                    b = nat.query_grid(0, R, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], blob, prec, setup["ws"])
                    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (R, prec, kv)
                    assert all(bool(torch.isfinite(v).all()) for v in a)
                    err[(prec, kv)] = [(lg(x) - lg(r)).abs() for x, r in zip(a, ref)]
                for i in range(2):
                    e3, e7 = err[(prec, 3)][i], err[(prec, 10)][i]
                    bound = 2e-2 if prec == "bf16" else 2.5e-3
                    assert e7.max().item() < bound and e3.max().item() < bound, (R, prec, i, e3.max().item(), e7.max().item())
                    assert e7.mean().item() < 1.05 * e3.mean().item(), (R, prec, i, e3.mean().item(), e7.mean().item())
        # the fp32-grade pair (v11 restated, v5 dense) and the bf16 x 3 operand split of the per-column GEMMs
        R = 48
        mat = oracle.coords_matrix(R, [-0.5] * 3, [0.5] * 3)[:3].reshape(-1)
        cal = common.CALIB.reshape(-1)[:12]
        vols = {}
        for kv, split in ((5, 0), (11, 0), (11, 3)):
            L.surs_set_grid_kernel(kv)
            L.surs_set_operand_split(split)
            vols[(kv, split)] = [v.clone() for v in nat.query_grid(0, R, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"],
                                                                   g.blob("bf16"), "fp32", setup["ws"])]
        L.surs_set_operand_split(0)
        for key in ((11, 0), (11, 3)):
            for x, r in zip(vols[key], vols[(5, 0)]):
                assert (lg(x) - lg(r)).abs().max().item() < 3e-5, key
        L.surs_set_grid_kernel(10)
        L.surs_set_operand_split(3)
        a3 = [v.clone() for v in nat.query_grid(0, R, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], g.blob("f16"), "fp16", setup["ws"])]
        L.surs_set_operand_split(0)
        a2 = nat.query_grid(0, R, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], g.blob("f16"), "fp16", setup["ws"])
        for x, r in zip(a3, a2):
            assert (lg(x) - lg(r)).abs().max().item() < 1e-3
        L.surs_profile_enable(1)
        R = 96
        mat = oracle.coords_matrix(R, [-0.5] * 3, [0.5] * 3)[:3].reshape(-1)
        nat.query_grid(0, R, R, R, mat, common.CALIB.reshape(-1)[:12], ZMUL, ZDIV, setup["Fl"], setup["Fh"], g.blob("bf16"), "bf16", setup["ws"])
        tiles, ks = C.c_double(0), C.c_double(0)
        L.surs_profile_read_ksteps(C.byref(tiles), C.byref(ks))
        assert tiles.value == 2 * R * R and 0 < ks.value <= 64 * tiles.value, (tiles.value, ks.value)
    finally:
        L.surs_profile_enable(0)
        L.surs_set_grid_kernel(0)
        L.surs_set_operand_split(0)


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-4), ("bf16", 3e-2), ("fp16", 4e-3)])
def test_sweep_edge_geometries_vs_point_path(setup, dtype, tol):
    """The column kernels on sweeps the other tests do not cover, against the fp32 point evaluator on the oracle's coordinates:
    a calibration that flips the depth axis (z_feat decreases with k: the tile box of the restated layer 1 takes min / max of its
    two ends), bounds that reach outside the image (columns with a zero mask), and a non-cubic grid whose depth is neither a
    multiple of the 64- nor of the 128-voxel tile.  fp32: logits at 1e-4."""
    import oracle
    nat, g = setup["native"], setup["g"]
    lg = lambda p: torch.log(p.double() / (1 - p.double()))
    flip = (np.diag([1.0, 1.0, -1.0, 1.0]).astype(np.float32) @ common.CALIB).astype(np.float32)
    for calib, b_min, b_max, res in ((flip, [-0.5] * 3, [0.5] * 3, (20, 24, 200)),
                                     (common.CALIB, [-0.6, -0.55, -0.5], [0.6, 0.5, 0.45], (24, 20, 72))):
        rx, ry, rz = res
        m = np.eye(4)
        for a, r in enumerate(res):
            m[a, a] = (b_max[a] - b_min[a]) / r
            m[a, 3] = b_min[a]
        ii, jj, kk = np.meshgrid(np.arange(rx), np.arange(ry), np.arange(rz), indexing="ij")
        idx = np.stack([ii.reshape(-1), jj.reshape(-1), kk.reshape(-1), np.ones(rx * ry * rz)]).astype(np.float64)
        pts = torch.from_numpy((m[:3] @ idx).astype(np.float32)).to(g.dev())
        cal = np.asarray(calib, np.float32).reshape(-1)[:12]
        blob = g.blob("f16" if dtype == "fp16" else "bf16")
        vh, vl = nat.query_grid(0, rx, ry, rz, m[:3].reshape(-1), cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], blob, dtype, setup["ws"])
        phr, plr, lhr, llr = nat.query_points(pts, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], g.blob("bf16"), setup["ws"], want_logits=True)
        assert (vh.reshape(-1) - phr).abs().max().item() < tol and (vl.reshape(-1) - plr).abs().max().item() < tol
        assert torch.equal(vh.reshape(-1) == 0, phr == 0)        # the same columns are masked
        if b_min[0] < -0.5:
            assert int((phr == 0).sum().item()) > 0
        if dtype == "fp32":
            ok = (phr > 0) & (phr < 1)
            assert (lg(vh.reshape(-1)[ok]) - lhr.double()[ok]).abs().max().item() < 1e-4


def test_dense_kernels_chosen_where_most_channels_are_listed(setup):
    """native.grid_kernel_for (what reconstruction / reconstruction_streamed / reconstruction_sharded ask before a sweep): a
    restated kernel for the ordinary field (fp32: the library default; bf16: the streamed kernel 12 up to LISTED_STREAM_THRESHOLD
    listed channels per tile, the eight-wave kernel 10 above); for a field in which about half of the layer-0
    channels change branch inside a z tile (the depth weights of layer 0 scaled by 60) the dense fp32-grade kernel (5), while the
    eight-wave bf16 kernel is still the faster one there (profiles/r03_listed_sensitivity.json).  The probe looks at the middle plane of the whole grid, so a slab gets the same
    answer; the chosen kernel's result equals the explicitly selected kernel's bit for bit."""
    import oracle
    from surs_amd import _lib
    nat, g = setup["native"], setup["g"]
    L = _lib.lib()
    R = 96
    mat = oracle.coords_matrix(R, [-0.5] * 3, [0.5] * 3)[:3].reshape(-1)
    cal = common.CALIB.reshape(-1)[:12]
    ws = setup["ws"]
    R2 = 256
    mat2 = oracle.coords_matrix(R2, [-0.5] * 3, [0.5] * 3)[:3].reshape(-1)
    for prec in ("bf16", "fp32"):
        blob = g.blob("bf16")
        pick = nat.grid_kernel_for(R2, R2, R2, mat2, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], blob, prec, ws)
        lr, hr = nat.probe_listed(R2 // 2, R2, R2, 64 if prec == "fp32" else 128, mat2, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], blob, ws)
        print(prec, "listed per tile at R=256: lr %.1f, hr bound %.1f -> kernel %d" % (lr, hr, pick))
        assert 0 < lr < 300 and hr >= lr * 0.5, (lr, hr)
        # fp32: the library's default (11).  bf16: the streamed kernel (12) while few channels are listed, the eight-wave one (10) above
        assert pick == (0 if prec == "fp32" else (12 if lr <= nat.LISTED_STREAM_THRESHOLD else 10)), (prec, pick, lr)
    sd = {k: np.array(v, copy=True) for k, v in common.state_dict().items() if k.startswith("mlp_")}
    for m in ("mlp_lr.", "mlp_hr."):
        sd[m + "conv0.weight"][:, 320] *= 60.0
    blob, _ = nat.pack_mlp(sd, "bf16", g.dev())
    for prec, dense in (("bf16", 3), ("fp32", 5)):
        kern = nat.grid_kernel_for(R, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], blob, prec, ws)
        listed = ws.kernel_choice[1]
        # (the eight-wave bf16 kernel stays ahead of the dense one up to ~600 listed channels, the fp32-grade pair crosses at 400)
        assert kern == (dense if listed > nat.LISTED_DENSE_THRESHOLDS[prec] else (0 if prec == "fp32" else 10)) and listed > 300, (prec, kern, ws.kernel_choice)
        if prec == "fp32":
            assert kern == dense, ws.kernel_choice
        a = [v.clone() for v in nat.query_grid(8, 40, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], blob, prec, ws, kernel=dense)]
        try:
            L.surs_set_grid_kernel(dense)
            b = [v.clone() for v in nat.query_grid(8, 40, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], blob, prec, ws)]
            L.surs_set_grid_kernel(10 if prec == "bf16" else 8)
            c = nat.query_grid(8, 40, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], blob, prec, ws)
        finally:
            L.surs_set_grid_kernel(0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])     # per-call option == process-wide setting
        # the restated kernels still agree on this field (many chunks per tile; its layer-0 activations are 60x the usual
        # size, and so are the fp32 roundings: 1e-3 instead of the 1e-4 of the ordinary fields)
        tol = 3e-2 if prec == "bf16" else 1e-3
        assert (a[0] - c[0]).abs().max().item() < tol and (a[1] - c[1]).abs().max().item() < tol
    # a second subject (other features in the same, recycled buffers) is probed again: nothing is cached
    n0 = ws.probes
    nat.grid_kernel_for(R, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], g.blob("bf16"), "bf16", ws)
    nat.grid_kernel_for(R, R, R, mat, cal, ZMUL, ZDIV, setup["Fl"], setup["Fh"], g.blob("bf16"), "bf16", ws)
    assert ws.probes == n0 + 2


# ------------------------------------------------------------------ point runs: the column kernels behind the point signature

def _run_points(seed=5, ncols=110, lo=180, hi=512, descending=False, outside=3):
    """Points as the reference's sweep loop hands them over (lib/sdf.py:32-45): runs of points that share (x, y), z monotonic
    inside a run - here with ragged run lengths, a first and a last run that are cut (a chunk starts and ends mid-column), a few
    runs outside the image, and (x, y) that are NOT on a lattice."""
    rng = np.random.RandomState(seed)
    xs, ys, zs = [], [], []
    for c in range(ncols):
        k = int(rng.randint(lo, hi + 1))
        x, y = rng.uniform(-0.45, 0.45, 2)
        if c < outside:
            x += 1.0   # projects outside [-1, 1]: masked runs
        z = np.sort(rng.uniform(-0.5, 0.5, k))
        if descending:
            z = z[::-1]
        xs.append(np.full(k, x)); ys.append(np.full(k, y)); zs.append(z)
    return np.stack([np.concatenate(xs), np.concatenate(ys), np.concatenate(zs)]).astype(np.float32)


def _qc(s, pts, dtype, calib=None):
    nat = s["native"]
    p = torch.from_numpy(np.ascontiguousarray(pts)).to(s["g"].dev())
    cal = np.asarray(common.CALIB if calib is None else calib, np.float32).reshape(-1)[:12]
    return nat.query_points_columns(p, cal, ZMUL, ZDIV, s["Fl"], s["Fh"], s["g"].blob("f16" if dtype == "fp16" else "bf16"), dtype, s["ws"])


@pytest.mark.parametrize("descending", [False, True])
def test_point_runs_fp32_vs_point_path_and_oracle(setup, descending):
    """surs_query_points_columns (kernel v11 on the runs of a point array) against surs_query_points on the same points - 1e-4 on
    the occupancies, the zero set (the in-image mask) identical - and against the oracle itself on a sample."""
    import oracle
    pts = _run_points(descending=descending)
    got = _qc(setup, pts, "fp32")
    assert got is not None
    phr, plr = [o.cpu().numpy() for o in got]
    rhr, rlr, _, _ = _q(setup, pts, common.CALIB)
    print("point runs fp32 (%d points): max |d occupancy| hr %.3e lr %.3e" % (pts.shape[1], np.abs(phr - rhr).max(), np.abs(plr - rlr).max()))
    assert np.abs(phr - rhr).max() < 1e-4 and np.abs(plr - rlr).max() < 1e-4
    assert ((phr == 0) == (rhr == 0)).all() and (phr == 0).sum() > 100
    sel = np.random.RandomState(1).choice(pts.shape[1], 3000, replace=False)
    ohr, olr = oracle.query(common.state_dict(), pts[:, sel], common.CALIB, setup["fl"], setup["fh"], 1024, 200.0)
    assert np.abs(phr[sel] - ohr).max() < 1e-4 and np.abs(plr[sel] - olr).max() < 1e-4


@pytest.mark.parametrize("dtype,tol", [("bf16", 3e-2), ("fp16", 4e-3)])
def test_point_runs_reduced_precision(setup, dtype, tol):
    """The 16-bit column kernel (v10, tile mode) on point runs, at the bounds of the sweep's own test (test_grid_column_kernel_vs_fp32)."""
    pts = _run_points(seed=6)
    got = _qc(setup, pts, dtype)
    assert got is not None
    phr, plr = [o.cpu().numpy() for o in got]
    rhr, rlr, _, _ = _q(setup, pts, common.CALIB)
    eh, el = np.abs(phr - rhr).max(), np.abs(plr - rlr).max()
    print("point runs %s: max |d occupancy| hr %.3e lr %.3e" % (dtype, eh, el))
    assert 1e-7 < eh < tol and el < tol
    assert ((phr == 0) == (rhr == 0)).all()


def test_point_runs_grid_chunk_equals_the_sweep(setup):
    """A 50 000-point piece of a flattened grid (what lib/sdf.py:32-45 passes per call), starting and ending mid-column: the runs
    path returns the fp32 sweep's values (same kernel, same per-column constants, the points' z read from the array instead of
    generated from (z0, dz): equal floats; the depth at which the per-column branches are taken differs, so the listed channels
    and the last bits do) - and a run longer than 4096 points is cut, not refused."""
    import oracle
    R = 96
    vh, vl = _grid(setup, R, "fp32")
    pts = oracle.grid_points(R, [-0.5] * 3, [0.5] * 3).astype(np.float32)
    a = 37 * R * R + 11 * R + 40
    piece = np.ascontiguousarray(pts[:, a:a + 50000])
    phr, plr = [o.cpu().numpy() for o in _qc(setup, piece, "fp32")]
    assert np.abs(phr - vh.reshape(-1)[a:a + 50000]).max() < 2e-5 and np.abs(plr - vl.reshape(-1)[a:a + 50000]).max() < 2e-5
    # more points than one library call takes (262 144): the host walks the array in pieces, a run cut at a piece's end is two runs
    big = np.ascontiguousarray(pts[:, 5 * R * R + 7:5 * R * R + 7 + 300000])
    bhr, blr = [o.cpu().numpy() for o in _qc(setup, big, "fp32")]
    assert np.abs(bhr - vh.reshape(-1)[5 * R * R + 7:5 * R * R + 7 + 300000]).max() < 2e-5
    assert np.abs(blr - vl.reshape(-1)[5 * R * R + 7:5 * R * R + 7 + 300000]).max() < 2e-5
    long_run = np.stack([np.full(10000, 0.123, np.float32), np.full(10000, -0.2, np.float32), np.linspace(-0.5, 0.5, 10000, dtype=np.float32)])
    got = _qc(setup, long_run, "fp32")
    assert got is not None
    rhr, rlr, _, _ = _q(setup, long_run, common.CALIB)
    assert np.abs(got[0].cpu().numpy() - rhr).max() < 1e-4 and np.abs(got[1].cpu().numpy() - rlr).max() < 1e-4


def test_point_runs_refused_where_there_are_none(setup):
    """Random samples, short arrays, z that goes both ways inside the runs, a calibration whose image position depends on z: the
    entry point writes nothing and says so; the caller takes the point kernels."""
    from surs_amd import weights
    assert _qc(setup, weights.synthetic_points(50000, seed=2), "fp32") is None
    assert _qc(setup, _run_points(ncols=4, lo=300, hi=400), "fp32") is None            # fewer than 2048 points
    pts = _run_points(seed=8)
    zig = pts.copy()
    zig[2, 5000:5100] = zig[2, 5000:5100][::-1].copy()                                   # a stretch that descends among ascending runs
    assert _qc(setup, zig, "fp32") is None
    cal = np.array(common.CALIB, np.float32).copy()
    cal[0, 2] = 0.05
    assert _qc(setup, pts, "fp32", calib=cal) is None
    short = _run_points(seed=9, ncols=6000, lo=4, hi=12)                                 # ~ 8 points per run
    assert _qc(setup, short, "fp32") is None


def test_point_runs_launches_sized_from_the_previous_call(setup):
    """surs_query_points_columns sizes its launches from the PREVIOUS call's run count (same array length) and reads the true count after
    the enqueue: arrays of one length with very different run structures, one after the other - many more runs than guessed (the batch
    runs again), far fewer, no runs at all (refused: the guess is dropped) - must give the bits of the call that reads the count first
    (option point_runs_speculate = 0)."""
    nat = setup["native"]
    n = 40000
    def fit(pts):   # cut / repeat to n points (whole array structure kept: the last run is cut)
        reps = -(-n // pts.shape[1])
        return np.ascontiguousarray(np.concatenate([pts] * reps, 1)[:, :n]) if reps > 1 else np.ascontiguousarray(pts[:, :n])
    arrays = [fit(_run_points(seed=21, ncols=120, lo=300, hi=512)),        # ~ 100 runs
              fit(_run_points(seed=22, ncols=1200, lo=30, hi=40)),         # ~ 1150 runs: 10 x the guess
              fit(_run_points(seed=23, ncols=30, lo=1200, hi=1500)),       # ~ 30 runs (cut at 4096 points: more columns than runs)
              fit(_run_points(seed=21, ncols=120, lo=300, hi=512))]
    from surs_amd import weights
    rnd = weights.synthetic_points(n, seed=4)
    for dtype in ("fp32", "bf16"):
        nat.set_option("point_runs_speculate", 0)
        try:
            want = [_qc(setup, a, dtype) for a in arrays]
        finally:
            nat.set_option("point_runs_speculate", 1)
        assert all(w is not None for w in want)
        got = []
        for i, a in enumerate(arrays):
            got.append(_qc(setup, a, dtype))
            if i == 1:
                assert _qc(setup, rnd, dtype) is None      # no runs: refused although the previous call left a guess
        for w, g_ in zip(want, got):
            assert g_ is not None and torch.equal(w[0], g_[0]) and torch.equal(w[1], g_[1])


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_small_batch_affine_gemm_equals_the_tiled_gemm_bit_for_bit(setup, dtype):
    """Batches of <= 1024 columns (a point-runs call: ~ 100 runs) take rvec_small_kernel for R = W1 (g . [a0 | w0z | w0p]) - 64 x 128
    workgroups reading MFMA fragments straight from the images - instead of four to six workgroups of the 256 x 256-tile GEMM: the same
    products in the same order, so the predictions must be equal bit for bit (option rvec_small = 0: the tiled kernel)."""
    nat = setup["native"]
    pts = _run_points(seed=31, ncols=150, lo=200, hi=500)
    got = _qc(setup, pts, dtype)
    nat.set_option("rvec_small", 0)
    try:
        want = _qc(setup, pts, dtype)
    finally:
        nat.set_option("rvec_small", 1)
    assert got is not None and want is not None
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_point_runs_kernel_equals_its_restatement(setup):
    """surs_point_runs (one workgroup: ballots, bit counts, two carries across blocks of 4096 points) against oracle.point_runs
    (plain loops) on ragged runs, runs cut at 4096 points, a chunk cut out of a grid, NaN and -0.0, and an array of singles."""
    import oracle
    nat = setup["native"]

    def check(pts, tile):
        cs, kc, tl, meta = nat.point_runs(torch.from_numpy(np.ascontiguousarray(pts)).to(setup["g"].dev()), tile)
        ocs, okc, otl, oviol = oracle.point_runs(pts, tile)
        assert meta[0] == len(ocs) and np.array_equal(cs, ocs)
        assert (bool(meta[2]), bool(meta[3])) == oviol
        if len(ocs) * (tile // 4) <= pts.shape[1]:
            assert np.array_equal(kc, okc) and meta[1] == len(otl)
            assert np.array_equal(tl[np.lexsort((tl[:, 1], tl[:, 0]))], otl)
        else:
            assert meta[1] == 0
    check(_run_points(seed=11, ncols=300, lo=33, hi=700), 64)
    check(_run_points(seed=12, ncols=90, lo=100, hi=512, descending=True), 128)
    long_runs = np.concatenate([_run_points(seed=13, ncols=3, lo=9000, hi=9500), _run_points(seed=14, ncols=40, lo=40, hi=80)], axis=1)
    check(long_runs, 64)
    grid = oracle.grid_points(64, [-0.5] * 3, [0.5] * 3)
    check(np.ascontiguousarray(grid[:, 12345:12345 + 50000]), 128)
    odd = _run_points(seed=15, ncols=120, lo=50, hi=90)
    odd[2, 777] = np.nan
    odd[0, 1500:1510] = -0.0
    odd[0, 1510:1520] = 0.0
    check(odd, 64)
    from surs_amd import weights
    check(weights.synthetic_points(5000, seed=3), 64)
    check(_run_points(seed=16, ncols=5000, lo=40, hi=64)[:, :262144], 64)    # the largest call: 64 blocks of 4096 points


@pytest.mark.gpu
def test_nonfinite_flag():
    """surs_nonfinite (the facade's check after every query): NaN / +-inf anywhere in either array are seen - first element, last
    element, an odd length; finite arrays (denormals, the largest float) pass; the flag is written, not accumulated."""
    from surs_amd import native
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(3)
    for n in (1, 63, 1025, 50000, 262144 + 7):
        a = torch.rand(n, generator=g).to(dev)
        b = torch.rand(n, generator=g).to(dev)
        a[0] = torch.finfo(torch.float32).max
        b[-1] = 1e-45
        assert native.any_nonfinite(a, b) is False and native.any_nonfinite(a) is False
        for bad in (float("nan"), float("inf"), float("-inf")):
            for arr, pos in ((a, 0), (a, n - 1), (b, n // 2), (b, n - 1)):
                keep = arr[pos].clone()
                arr[pos] = bad
                assert native.any_nonfinite(a, b) is True
                assert native.any_nonfinite(arr) is True
                arr[pos] = keep
        assert native.any_nonfinite(a, b) is False
        if n > 1:   # (views that do not start on 16 bytes: the scalar form of the kernel)
            assert native.any_nonfinite(a[1:], b[1:]) is False
            b[-1] = float("inf")
            assert native.any_nonfinite(a[1:], b[1:]) is True and native.any_nonfinite(a[:-1], b[:-1]) is False
    assert native.any_nonfinite(torch.empty(0, device=dev)) is False
