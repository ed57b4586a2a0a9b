"""CPU checks of --hg_dim other than 256 (the channels of the hourglass encoder's output): the state dict against the reference's
key / shape lists (tests/golden/state_dict_keys_hg_dim.json, tools/gen_golden_hg_dim.py), the limits native.mlp_shapes and the
constructor enforce, the generic blob's layout for another D and its bytes for the released one, the LDS limit per D, and the
fused kernels' resource usage."""
import hashlib
import json
import os

import numpy as np
import pytest

import common
from surs_amd import _lib, model, native, options, prng, weights


def _flags(D, hidden, res=None):
    s = lambda tag, v: ["--mlp_" + tag] + [str(x) for x in v]
    out = ["--hg_dim", str(D)] + s("dim_lr", [D + 65] + hidden + [1]) + s("dim_hr", [D + 66] + hidden + [1])
    if res is not None:
        out += s("res_layers_lr", res) + s("res_layers_hr", res)
    return out


CASES = {   # (the flags tools/gen_golden_hg_dim.py ran the reference with)
    "d128": _flags(128, [1024, 512, 256, 128]),
    "d384": _flags(384, [512, 256, 128], [1, 2, 3]),
    "d48": _flags(48, [1000, 500, 250, 100]),
}


def _opt(extra):
    return options.BaseOptions().parse(common.FLAGS + list(extra))


def _sd(dims_lr, res_lr, dims_hr, res_hr, seed=0):
    sd = {}
    for prefix, dims, res in (("mlp_lr.", dims_lr, res_lr), ("mlp_hr.", dims_hr, res_hr)):
        for key, shape, kind in weights._mlp(prefix, list(dims), list(res), False):
            sd[key] = prng.uniform(key, seed, shape, -0.5, 0.5)
    return sd


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_follows_hg_dim(golden_dir, name):
    with open(os.path.join(golden_dir, "state_dict_keys_hg_dim.json")) as f:
        want = [(k, tuple(s)) for k, s in json.load(f)[name]]
    opt = _opt(CASES[name])
    assert [(k, tuple(s)) for k, s, _ in weights.state_dict_spec(opt)] == want
    D = opt.hg_dim
    shapes = dict(want)
    assert shapes["image_filter_lr.l2.weight"] == (D, 256, 1, 1) and shapes["image_filter_lr.al0.weight"] == (256, D, 1, 1)
    assert shapes["image_filter_hr.l0.weight"] == (D, 256, 1, 1)   # (dead in the forward pass, part of the state dict)
    sd = weights.synthetic_state_dict(opt, seed=0)
    net = model.SuRSNet(opt)
    net.load_state_dict(sd)   # strict
    back = net.state_dict()
    assert [(k, tuple(v.shape)) for k, v in back.items()] == want
    assert all(np.array_equal(back[k].numpy(), sd[k]) for k in sd)
    with pytest.raises(RuntimeError, match="size mismatch"):
        net.load_state_dict(weights.synthetic_state_dict(common.opt(), seed=0), strict=False)


def test_mlp_shapes_takes_the_width_from_hg_dim():
    for name, flags in CASES.items():
        opt = _opt(flags)
        D = opt.hg_dim
        sd = {k: v for k, v in weights.synthetic_state_dict(opt, seed=0).items() if k.startswith("mlp_")}
        shapes = native.mlp_shapes(sd, opt)
        assert shapes[0][0][0] == D + 65 and shapes[1][0][0] == D + 66 and native.mlp_hg_dim(shapes) == D
        assert not native.is_default_mlp(shapes)
    # the released hidden widths on another D: never the released shape's kernels
    rel = native.mlp_shapes(_sd([193, 1024, 512, 256, 128, 1], [2, 3, 4], [194, 1024, 512, 256, 128, 1], [2, 3, 4]),
                            _opt(["--hg_dim", "128", "--mlp_dim_lr", "193", "1024", "512", "256", "128", "1",
                                  "--mlp_dim_hr", "194", "1024", "512", "256", "128", "1"]))
    assert not native.is_default_mlp(rel)
    # 321 / 322 with --hg_dim 128
    sd256 = {k: v for k, v in common.state_dict().items() if k.startswith("mlp_")}
    with pytest.raises(ValueError, match=r"input width 321; it must be 193 .*--hg_dim 128"):
        native.mlp_shapes(sd256, _opt(["--hg_dim", "128"]))
    # 193 / 194 without it
    sd128 = _sd([193, 64, 1], [], [194, 64, 1], [])
    with pytest.raises(ValueError, match=r"input width 193; it must be 321 .*--hg_dim 256"):
        native.mlp_shapes(sd128)
    with pytest.raises(ValueError, match="input width"):
        native.mlp_shapes(sd128, common.opt())
    # the hr input is the lr input + 1
    with pytest.raises(ValueError, match=r"mlp_hr: input width 193; it must be 194"):
        native.mlp_shapes(_sd([193, 64, 1], [], [193, 64, 1], []),
                          _opt(["--hg_dim", "128", "--mlp_dim_lr", "193", "64", "1", "--mlp_dim_hr", "194", "64", "1", "--no_residual"]))
    with pytest.raises(_lib.SursError, match="input width"):
        native.mlp_generic_info((((193, 64, 1), ()), ((195, 64, 1), ())))
    with pytest.raises(_lib.SursError, match="input width .* multiple of 16 from 16 to 512"):
        native.mlp_generic_info((((105, 64, 1), ()), ((106, 64, 1), ())))   # D = 40


@pytest.mark.parametrize("D", [0, 8, 40, 520])
def test_constructor_refuses_other_hg_dim(D):
    opt = _opt(["--hg_dim", str(D)])
    with pytest.raises(ValueError, match="hg_dim %d: the supported values are the multiples of 16 from 16 to 512" % D):
        model.SuRSNet(opt)
    with pytest.raises(ValueError, match="hg_dim"):
        native.mlp_shapes({}, opt)


def _f16(u):
    return u.view(np.float16).astype(np.float32)


def _bf16(u):
    return (u.astype(np.uint32) << 16).view(np.float32)


def test_packer_layout_d48():
    """test_mlp_shapes_host.test_packer_layout for D = 48: the feature segment of a skip layer is pad32(48 + 66) = 128 wide."""
    D = 48
    dims_lr, res_lr, dims_hr, res_hr = [D + 65, 40, 1], [1], [D + 66, 33, 7, 1], [0, 2]
    sd = _sd(dims_lr, res_lr, dims_hr, res_hr)
    shapes = native.mlp_shapes(sd, _opt(["--hg_dim", str(D), "--mlp_dim_lr"] + [str(d) for d in dims_lr] + ["--mlp_dim_hr"]
                                        + [str(d) for d in dims_hr] + ["--mlp_res_layers_lr", "1", "--mlp_res_layers_hr", "0", "2"]))
    host, shapes = native.pack_mlp_generic_host(sd, shapes)
    tile_points, lds, off = native.mlp_generic_info(shapes)
    c0pad = -(-(D + 66) // 32) * 32
    assert c0pad == 128 and tile_points == 32 and lds == 32 * ((64 + 4 + c0pad + 4) * 4 + 16)
    for m, (prefix, (dims, res)) in enumerate(zip(("mlp_lr.", "mlp_hr."), shapes)):
        c0 = dims[0]
        for l in range(len(dims) - 1):
            w = np.asarray(sd[prefix + "conv%d.weight" % l], np.float32)[:, :, 0]
            b = np.asarray(sd[prefix + "conv%d.bias" % l], np.float32)
            k1, skip = dims[l], l in res
            k1pad, k2pad, mpad = -(-k1 // 32) * 32, c0pad if skip else 0, -(-dims[l + 1] // 32) * 32
            full = np.zeros((mpad, k1pad + k2pad), np.float32)
            full[:w.shape[0], :k1] = w[:, :k1]
            if skip:
                full[:w.shape[0], k1pad:k1pad + c0] = w[:, k1:]

            def image(parts, o):
                n = (k1pad + k2pad) * mpad
                a = np.frombuffer(host, np.uint16, parts * n, int(o)).reshape(parts, (k1pad + k2pad) // 32, mpad // 16, 4, 16, 8)
                return a.transpose(0, 2, 4, 1, 3, 5).reshape(parts, mpad, k1pad + k2pad)

            one, two, three = image(1, off[m, l, 0]), image(2, off[m, l, 1]), image(3, off[m, l, 2])
            assert np.array_equal(_f16(one[0]), full.astype(np.float16).astype(np.float32))
            hi = _f16(two[0])
            assert np.array_equal(hi, full.astype(np.float16).astype(np.float32))
            assert np.array_equal(_f16(two[1]), (full - hi).astype(np.float16).astype(np.float32))
            s = _bf16(three[0]).astype(np.float64) + _bf16(three[1]) + _bf16(three[2])
            assert np.array_equal(s, full.astype(np.float64))
            bias = np.frombuffer(host, np.float32, mpad, int(off[m, l, 3]))
            assert np.array_equal(bias[:b.size], b) and not bias[b.size:].any()
    # the next offset after a skip layer's one-part image: (k1pad + 128) * mpad halves
    assert int(off[0, 1, 1] - off[0, 1, 0]) == -(-((64 + c0pad) * 32 * 2) // 256) * 256


S1 = ["--mlp_dim_lr", "321", "512", "256", "128", "1", "--mlp_dim_hr", "322", "512", "256", "128", "1", "--mlp_res_layers_lr", "1", "2",
      "3", "--mlp_res_layers_hr", "1", "2", "3"]
# sha256 of pack_mlp_generic_host's blob for shape s1 (synthetic weights, seed 0), recorded on the commit before --hg_dim was followed
S1_BLOB_SHA256 = "765f32872ad2f16c9031060b6c01e6d8bb1f89b692301924f48475d3b28412b0"
S1_BLOB_BYTES = 11878144


def test_d256_blob_is_what_it_was():
    opt = _opt(S1)
    sd = {k: v for k, v in weights.synthetic_state_dict(opt, seed=0).items() if k.startswith("mlp_")}
    host, shapes = native.pack_mlp_generic_host(sd, native.mlp_shapes(sd, opt))
    assert host.size == S1_BLOB_BYTES
    assert hashlib.sha256(host.tobytes()).hexdigest() == S1_BLOB_SHA256
    assert native.mlp_generic_info(shapes)[:2] == (32, 32 * ((512 + 4 + 356) * 4 + 16))


def _limit(D, rows, extra, cap):
    """The widest multiple of 32 W with 16 * ((W + 4) + rows * (pad32(D + 66) + 4)) * 4 + 16 * extra <= 160 KiB, at most cap."""
    fs = -(-(D + 66) // 32) * 32 + 4
    w = 0
    while 16 * ((w + 32 + 4) + rows * fs) * 4 + 16 * extra <= 160 * 1024:
        w += 32
    return min(w, cap)


def _pair(D, width):
    return (((D + 65, width, 1), ()), ((D + 66, width, 1), ()))


@pytest.mark.parametrize("D", [16, 48, 256, 384, 512])
def test_lds_limit_per_hg_dim(D):
    single, views = _limit(D, 1, 16, 2048), _limit(D, 2, 24, 1824)
    assert native.mlp_max_hidden(D) == single and native.mlp_max_hidden(D, views=True) == views
    if D <= 256:
        assert (single, views) == (2048, 1824)
    tp, lds, _ = native.mlp_generic_info(_pair(D, single))
    assert tp == 16 and lds <= 160 * 1024
    assert lds == 16 * ((single + 4 + -(-(D + 66) // 32) * 32 + 4) * 4 + 16)
    tp, lds = native.mlp_generic_views_info(_pair(D, views), 2)
    assert tp == 16 and lds <= 160 * 1024
    # the 32-point tile by the same formula
    w32 = (160 * 1024 // 32 - 16) // 4 - 4 - (-(-(D + 66) // 32) * 32 + 4)
    w32 = w32 // 32 * 32
    assert native.mlp_generic_info(_pair(D, w32))[0] == 32 and native.mlp_generic_info(_pair(D, w32 + 32))[0] == 16


def test_d512_refuses_beyond_its_limit():
    assert native.mlp_max_hidden(512) == 1920 and native.mlp_max_hidden(512, views=True) == 1312
    native.mlp_generic_info(_pair(512, 1920))
    with pytest.raises(_lib.SursError, match="hidden widths must be at most 1920 with hg_dim 512"):
        native.mlp_generic_info(_pair(512, 1952))
    with pytest.raises(ValueError, match="hidden widths must be at most 1920 with hg_dim 512"):
        native.mlp_shapes(_sd([577, 1952, 1], [], [578, 1952, 1], []), _opt(["--hg_dim", "512", "--mlp_dim_lr", "577", "1952", "1",
                                                                            "--mlp_dim_hr", "578", "1952", "1"]))
    native.mlp_generic_views_info(_pair(512, 1312), 2)
    with pytest.raises(ValueError, match="multi-view: hidden widths must be at most 1312 with hg_dim 512"):
        native.mlp_generic_views_info(_pair(512, 1344), 2)
    # D <= 256: the limits and their words as they were
    with pytest.raises(ValueError, match="multi-view: hidden widths must be at most 1824"):
        native.mlp_generic_views_info(_pair(128, 1856), 2)
    with pytest.raises(_lib.SursError, match="hidden widths must be between 1 and 2048"):
        native.mlp_generic_info(_pair(128, 2080))


def test_fused_kernels_still_six_and_six(tmp_path):
    """The released D = 256 keeps its six + six instantiations under their names (mlp_fused_kernel, mlp_fused_views_kernel); any other D
    runs the same bodies with the channel counts and the row stride as launch arguments (mlp_anyd_kernel, mlp_anyd_views_kernel): six
    each, no scratch, <= 256 registers, LDS dynamic."""
    import isa
    meta = {}
    for co in isa.code_objects(workdir=str(tmp_path)):
        meta.update(isa.kernel_metadata(co))
    for tag in ("mlp_fused_kernel", "mlp_fused_views_kernel", "mlp_anyd_kernel", "mlp_anyd_views_kernel"):
        fused = {k: v for k, v in meta.items() if tag in k}
        assert len(fused) == 6, (tag, sorted(fused))
        for name, m in fused.items():
            assert m[".private_segment_fixed_size"] == 0, name
            assert m[".vgpr_count"] + m.get(".agpr_count", 0) <= 256, name
            assert m[".group_segment_fixed_size"] == 0, name
