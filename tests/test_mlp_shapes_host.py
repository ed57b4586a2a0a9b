"""CPU checks of classifier shapes other than the released one: the limits native.mlp_shapes enforces (each raises ValueError
naming it), the blob of surs_mlp_pack_generic unpacked in numpy against the weights, and the released shape's own packer."""
import numpy as np
import pytest

import common
from surs_amd import native, options, prng, weights


def _sd(dims_lr, res_lr, dims_hr=None, res_hr=None, seed=0):
    """mlp_* weights of the given shapes (weights._mlp: the reference's in_channels rule)."""
    dims_hr = dims_hr if dims_hr is not None else [322] + list(dims_lr[1:])
    res_hr = res_hr if res_hr is not None else res_lr
    sd = {}
    for prefix, dims, res in (("mlp_lr.", dims_lr, res_lr), ("mlp_hr.", dims_hr, res_hr)):
        for key, shape, kind in weights._mlp(prefix, list(dims), list(res), False):
            sd[key] = prng.uniform(key, seed, shape, -0.5, 0.5)
    return sd


def _opt(extra):
    return options.BaseOptions().parse(common.FLAGS + extra)


@pytest.mark.parametrize("dims,res,match", [
    ([321] + [8] * 8 + [1], [], "between 1 and 8"),
    ([320, 64, 1], [], "input width"),
    ([321, 64, 2], [], "last width"),
    ([321, 2049, 1], [], "hidden widths"),
])
def test_limits(dims, res, match):
    with pytest.raises(ValueError, match=match):
        native.mlp_shapes(_sd(dims, res))


def test_hr_input_width_limit():
    sd = _sd([321, 64, 1], [], dims_hr=[321, 64, 1])
    with pytest.raises(ValueError, match="input width"):
        native.mlp_shapes(sd)


def test_no_layers():
    with pytest.raises(ValueError, match="between 1 and 8"):
        native.mlp_shapes({})


def test_skip_layers_out_of_range_from_options():
    opt = _opt(["--mlp_dim_lr", "321", "64", "1", "--mlp_dim_hr", "322", "64", "1", "--mlp_res_layers_lr", "2",
                "--mlp_res_layers_hr", "1"])
    with pytest.raises(ValueError, match=r"skip layers .* must be in \[0, 2\)"):
        native.mlp_shapes(_sd([321, 64, 1], [1]), opt)


def test_options_cross_check():
    opt = _opt(["--mlp_dim_lr", "321", "64", "1", "--mlp_dim_hr", "322", "64", "1", "--mlp_res_layers_lr", "1",
                "--mlp_res_layers_hr", "1"])
    assert native.mlp_shapes(_sd([321, 64, 1], [1]), opt) == (((321, 64, 1), (1,)), ((322, 64, 1), (1,)))
    with pytest.raises(ValueError, match="the options say"):
        native.mlp_shapes(_sd([321, 64, 1], [0]), opt)


def test_no_residual_means_no_skips():
    opt = _opt(["--no_residual"])
    sd = weights.synthetic_state_dict(opt, seed=0)
    shapes = native.mlp_shapes({k: v for k, v in sd.items() if k.startswith("mlp_")}, opt)
    assert shapes == (((321, 1024, 512, 256, 128, 1), ()), ((322, 1024, 512, 256, 128, 1), ()))
    assert not native.is_default_mlp(shapes)


def test_library_refuses_what_python_refuses():
    from surs_amd import _lib
    with pytest.raises(_lib.SursError, match="hidden widths"):
        native.mlp_generic_info((((321, 4096, 1), ()), ((322, 64, 1), ())))
    with pytest.raises(_lib.SursError, match="skip layers"):
        native.mlp_generic_info((((321, 64, 1), (2,)), ((322, 64, 1), ())))


def test_default_shape_takes_the_released_packer():
    sd = {k: v for k, v in common.state_dict().items() if k.startswith("mlp_")}
    shapes = native.mlp_shapes(sd, common.opt())
    assert native.is_default_mlp(shapes) and shapes == native.DEFAULT_MLP_SHAPES
    with pytest.raises(ValueError, match="pack_mlp_generic"):
        native.pack_mlp(_sd([321, 512, 256, 128, 1], [1, 2, 3]), "bf16", "cpu")


def _f16(u):
    return u.view(np.float16).astype(np.float32)


def _bf16(u):
    return (u.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("dims_lr,res_lr,dims_hr,res_hr", [
    ([321, 40, 1], [1], [322, 33, 7, 1], [0, 2]),
    ([321, 1], [0], [322, 1], []),
])
def test_packer_layout(dims_lr, res_lr, dims_hr, res_hr):
    sd = _sd(dims_lr, res_lr, dims_hr, res_hr)
    host, shapes = native.pack_mlp_generic_host(sd)
    tile_points, lds, off = native.mlp_generic_info(shapes)
    assert tile_points in (16, 32) and 0 < lds <= 160 * 1024
    for m, (prefix, (dims, res)) in enumerate(zip(("mlp_lr.", "mlp_hr."), shapes)):
        c0 = dims[0]
        for l in range(len(dims) - 1):
            w = np.asarray(sd[prefix + "conv%d.weight" % l], np.float32)[:, :, 0]
            b = np.asarray(sd[prefix + "conv%d.bias" % l], np.float32)
            k1, skip = dims[l], l in res
            k1pad, k2pad, mpad = -(-k1 // 32) * 32, 352 if skip else 0, -(-dims[l + 1] // 32) * 32
            # the reference's [out][y | feature] as the kernel's [out][k1pad | k2pad], zeros elsewhere
            full = np.zeros((mpad, k1pad + k2pad), np.float32)
            full[:w.shape[0], :k1] = w[:, :k1]
            if skip:
                full[:w.shape[0], k1pad:k1pad + c0] = w[:, k1:]

            def image(parts, o):
                # [part][kt][tile][lane][8]: lane = row % 16 + 16 * (k % 32 // 8), element k % 8
                n = (k1pad + k2pad) * mpad
                a = np.frombuffer(host, np.uint16, parts * n, int(o)).reshape(parts, (k1pad + k2pad) // 32, mpad // 16, 4, 16, 8)
                return a.transpose(0, 2, 4, 1, 3, 5).reshape(parts, mpad, k1pad + k2pad)

            one, two, three = image(1, off[m, l, 0]), image(2, off[m, l, 1]), image(3, off[m, l, 2])
            assert np.array_equal(_f16(one[0]), full.astype(np.float16).astype(np.float32))
            hi = _f16(two[0])
            assert np.array_equal(hi, full.astype(np.float16).astype(np.float32))
            assert np.array_equal(_f16(two[1]), (full - hi).astype(np.float16).astype(np.float32))
            # three bf16 parts sum exactly to the fp32 weight; padding is zero in every part
            s = _bf16(three[0]).astype(np.float64) + _bf16(three[1]) + _bf16(three[2])
            assert np.array_equal(s, full.astype(np.float64))
            assert not three[:, w.shape[0]:, :].any() and not two[:, w.shape[0]:, :].any()
            bias = np.frombuffer(host, np.float32, mpad, int(off[m, l, 3]))
            assert np.array_equal(bias[:b.size], b) and not bias[b.size:].any()


def test_fused_kernels_use_no_scratch(tmp_path):
    """The compiler's resource usage of the six fused-kernel instantiations in the shipped code object: no scratch, the VGPR / AGPR
    budget of eight waves per workgroup (<= 256), LDS dynamic (sized per shape by surs_mlp_generic_info)."""
    import isa
    meta = {}
    for co in isa.code_objects(workdir=str(tmp_path)):
        meta.update(isa.kernel_metadata(co))
    fused = {k: v for k, v in meta.items() if "mlp_fused_kernel" in k}
    assert len(fused) == 6, sorted(fused)
    for name, m in fused.items():
        assert m[".private_segment_fixed_size"] == 0, name
        assert m[".vgpr_count"] + m.get(".agpr_count", 0) <= 256, name
        assert m[".group_segment_fixed_size"] == 0, name
