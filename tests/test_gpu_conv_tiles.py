"""The split-operand 3x3 convolution (conv_x3_kernel) on each of its three tiles - 4 rows x 32 channels, 8 x 32, 8 x 64 - forced
through the library options conv_tall_min_wg / conv_wide_min_wg, with two f16 parts per operand and with one, against the float64
restatement of tests/conv_ref.py: whole and ragged tiles, odd chunk counts, every combination of outputs the entry points expose,
the GroupNorm statistics summed over ragged tiles and the sum in the epilogue; the selection rule at its defaults; the pointwise
kernel's two instantiations.  Bounds as in test_gpu_encoder_ops.py: 2e-5 of the output range with two parts (22 significant bits,
fp32 accumulation), 2e-3 with one (11 bits)."""
import numpy as np
import pytest
import torch

import common
import conv_ref
from conv_tiles import TILE_OPTIONS, ConvSum, fold, force_tile, hwc, tile_of  # noqa: F401  (force_tile: the fixture)
from surs_amd import prng

pytestmark = pytest.mark.gpu

TOL = {2: 2e-5, 1: 2e-3}
CANARY = 7.5
# cin, cout, h, w
CASES = {
    "a": (16, 32, 13, 37),   # one chunk; 8-row tiles: a second row tile of 5 rows, a second column tile of 5 columns; half a 64-channel tile
    "b": (48, 96, 3, 5),     # three chunks; smaller than one tile both ways; cout_pad 128, the wide tile's second block half empty
    "c": (80, 64, 16, 64),   # five chunks; whole tiles for every tile: the straight epilogue
    "d": (32, 128, 17, 64),  # one ragged row, whole columns: straight and guarded workgroups in one launch
    "e": (64, 64, 16, 33),   # one ragged column, whole rows
}
VARIANTS = ("plain", "epilogue", "prologue", "out_slice", "in_slice")
TILE_PARTS = [("4x32", 2), ("8x32", 2), ("8x64", 2), ("4x32", 1), ("8x32", 1), ("8x64", 1)]

_entry, _cases, _refs, _runs, _worst = {}, {}, {}, {}, {}


@pytest.fixture(scope="module")
def env():
    import gpu_common as g
    from surs_amd import native
    dev = g.dev()
    _entry.update({k: native.get_option(k) for k in TILE_OPTIONS})   # (what the module's last test finds again)
    return dict(g=g, native=native, dev=dev)


def _chw(img):
    return img.to_nchw()[0].cpu().numpy()


def _dev(env, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _case(env, name):
    """A case's seeded operands, on the host and (uploaded once) on the device."""
    if name not in _cases:
        nat, g = env["native"], env["g"]
        cin, cout, h, w = CASES[name]
        d = conv_ref.inputs("t" + name, 1, cin, cout, h, w)
        d["X"], d["R"] = g.upload_nhwc(d["x"]), g.upload_nhwc(d["res"])
        # the same input as channels [8, 8 + cin) of a wider tensor
        wide = np.concatenate([np.full((8, h, w), 3.25, np.float32), d["x"], np.full((4, h, w), -2.5, np.float32)])
        d["Xs"] = g.upload_nhwc(wide).slice(8, cin)
        d["S"], d["H"] = _dev(env, d["scale"]), _dev(env, d["shift"])
        d["cw"] = {(p, b): nat.ConvWeights(d["w"], d["b"] if b else None, env["dev"], reduced=p == 1) for p in (1, 2) for b in (0, 1)}
        _cases[name] = d
    return _cases[name]


def _ref(env, case, variant):
    if (case, variant) not in _refs:
        d = _case(env, case)
        _refs[case, variant] = {
            "plain": lambda: conv_ref.conv(d["x"], d["w"]),
            "epilogue": lambda: conv_ref.conv(d["x"], d["w"], d["b"], slope=0.2, residual=d["res"]),
            "prologue": lambda: conv_ref.conv(d["x"], d["w"], d["b"], in_scale=d["scale"], in_shift=d["shift"]),
            "out_slice": lambda: conv_ref.conv(d["x"], d["w"], d["b"], residual=d["res"]),
            "in_slice": lambda: _ref(env, case, "plain"),
        }[variant]()
    return _refs[case, variant]


def _args(d, variant, parts):
    """(input, weights, keyword arguments) of a variant for native.conv2d / conv2d_gn."""
    if variant in ("plain", "in_slice"):
        return d["Xs" if variant == "in_slice" else "X"], d["cw"][parts, 0], {}
    kw = {"epilogue": dict(act=1, slope=0.2, residual=d["R"]), "prologue": dict(in_scale=d["S"], in_shift=d["H"]),
          "out_slice": dict(residual=d["R"])}[variant]
    return d["X"], d["cw"][parts, 1], kw


def _launch(env, force_tile, case, variant, tile, parts):
    nat, d = env["native"], _case(env, case)
    cin, cout, h, w = CASES[case]
    x, cw, kw = _args(d, variant, parts)
    force_tile(tile)
    if variant != "out_slice":
        return _chw(nat.conv2d(x, cw, **kw))
    wide = nat.Img(h, w, cout + 40, device=env["dev"])
    wide.buf.fill_(CANARY)
    nat.conv2d(x, cw, out=wide.slice(24, cout), **kw)
    full = _chw(wide)
    # every channel outside the slice still holds the canary, bit for bit
    assert np.array_equal(full[:24], np.full((24, h, w), CANARY, np.float32)) and np.array_equal(full[24 + cout:], np.full((16, h, w), CANARY, np.float32))
    return full[24:24 + cout]


def _run(env, force_tile, case, variant, tile, parts):
    key = (case, variant, tile, parts)
    if key not in _runs:
        _runs[key] = _launch(env, force_tile, case, variant, tile, parts)
    return _runs[key]


def _note(tile, parts, err):
    k = ("%dx%d" % tile_of(tile, parts), parts)
    _worst[k] = max(_worst.get(k, 0.0), err)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("tile,parts", TILE_PARTS)
def test_every_tile_against_float64(env, force_tile, tile, parts, case):
    for variant in VARIANTS:
        y, ref = _run(env, force_tile, case, variant, tile, parts), _ref(env, case, variant)
        assert y.shape == ref.shape
        err = common.rel_err(y, ref)
        print("conv tiles: case %s %s tile %s parts %d: rel_err %.3e" % (case, variant, tile, parts, err))
        _note(tile, parts, err)
        assert err < TOL[parts], (variant, err)
    # the same pixels read through a channel slice: the same bits
    assert np.array_equal(_run(env, force_tile, case, "in_slice", tile, parts), _run(env, force_tile, case, "plain", tile, parts))
    if (tile, parts) == ("8x64", 1):    # the one-part kernel has no 64-channel form: conv_wide_min_wg does not reach it
        for variant in VARIANTS:
            assert np.array_equal(_run(env, force_tile, case, variant, tile, parts), _run(env, force_tile, case, variant, "8x32", parts)), variant


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("parts", [2, 1])
def test_tall_tile_gives_the_bits_of_the_small_tile(env, force_tile, parts, case):
    """README's "same bits": both 32-channel tiles add their partial products on three accumulators, summed as (a0 + a1) + a2."""
    for variant in VARIANTS:
        assert np.array_equal(_run(env, force_tile, case, variant, "8x32", parts), _run(env, force_tile, case, variant, "4x32", parts)), variant


@pytest.mark.parametrize("case", sorted(CASES))
def test_wide_tile_is_deterministic(env, force_tile, case):
    """8 x 64 sums in another order than the 32-channel tiles (not their bits; both are held to float64 above): two runs, equal bits."""
    for variant in VARIANTS:
        again = _launch(env, force_tile, case, variant, "8x64", 2)
        assert np.array_equal(again, _run(env, force_tile, case, variant, "8x64", 2)), variant


@pytest.mark.parametrize("tile", ["4x32", "8x32", "8x64"])
def test_the_two_part_bound_tells_a_lost_partial_product(env, force_tile, tile):
    """One f16 product per MAC is the two-part kernel without its two small partial products: on case c it must miss the two-part
    bound against float64, or that bound would pass a kernel that lost one.  (Measured on gfx950: see NOTES.md.)"""
    err = common.rel_err(_run(env, force_tile, "c", "plain", tile, 1), _ref(env, "c", "plain"))
    print("conv tiles: one-part rel_err on case c, tile %s: %.3e (two-part bound %.0e)" % (tile, err, TOL[2]))
    assert TOL[2] < err < TOL[1]


def test_options_do_not_leak_into_kernels_that_have_one_tile(env, force_tile, monkeypatch):
    nat, g = env["native"], env["g"]
    # stride 2: the 4-row tile whatever the options say
    d = conv_ref.inputs("ts", 2, 32, 64, 33, 47)
    X = g.upload_nhwc(d["x"])
    for reduced in (False, True):
        cw = nat.ConvWeights(d["w"], d["b"], env["dev"], reduced=reduced)
        force_tile("8x64")
        forced = _chw(nat.conv2d(X, cw, stride=2, act=1, slope=0.2))
        force_tile("4x32")
        assert np.array_equal(forced, _chw(nat.conv2d(X, cw, stride=2, act=1, slope=0.2)))
        assert common.rel_err(forced, conv_ref.conv(d["x"], d["w"], d["b"], stride=2, slope=0.2)) < TOL[1 if reduced else 2]
    # three bf16 parts (the wide-operand retry): the same
    monkeypatch.setenv("SURS_CONV_SPLIT", "bf16x3")
    dc = _case(env, "d")
    cw = nat.ConvWeights(dc["w"], dc["b"], env["dev"])
    assert cw.w3 is not None and cw.parts == 3
    force_tile("8x64")
    forced = _chw(nat.conv2d(dc["X"], cw, residual=dc["R"]))
    force_tile("4x32")
    assert np.array_equal(forced, _chw(nat.conv2d(dc["X"], cw, residual=dc["R"])))
    assert common.rel_err(forced, _ref(env, "d", "out_slice")) < TOL[2]


# ---------------------------------------------------------------- GroupNorm statistics over ragged tiles

def _slots(h, w, rows):
    return -(-w // 32) * -(-h // rows)


@pytest.mark.parametrize("case", ["a", "c", "d", "e"])     # cout 32, 64, 128, 64: 1, 2, 4 channels per group
@pytest.mark.parametrize("tile,parts", TILE_PARTS)
def test_statistics_of_ragged_tiles_and_their_consumer(env, force_tile, tile, parts, case):
    """conv2d_gn(want_stats=True): one slot per pixel tile of the forced tile, holding the sums of exactly the values stored (after
    LeakyReLU and residual; no padded row or column in them); the maps are those of the run without statistics.  Then the consumer: a
    second convolution that normalises with those statistics, against float64 from the first one's stored output."""
    nat, d = env["native"], _case(env, case)
    cin, cout, h, w = CASES[case]
    rows = tile_of(tile, parts)[0]
    c2 = 32
    w2, b2 = prng.uniform("t2w", cout, (c2, cout, 3, 3), -0.2, 0.2), prng.uniform("t2b", cout, (c2,), -0.5, 0.5)
    gamma, beta = prng.uniform("t2g", cout, (cout,), 0.5, 1.5), prng.uniform("t2h", cout, (cout,), -0.3, 0.3)
    cw2 = nat.ConvWeights(w2, b2, env["dev"], reduced=parts == 1)
    G = (_dev(env, gamma), _dev(env, beta))
    for variant in ("plain", "epilogue"):
        x, cw, kw = _args(d, variant, parts)
        force_tile(tile)
        out = nat.conv2d_gn(x, cw, want_stats=True, **kw)
        assert out.stats.slots == _slots(h, w, rows)
        v = _chw(out)
        assert np.array_equal(v, _chw(nat.conv2d_gn(x, cw, **kw)))
        assert np.array_equal(v, _run(env, force_tile, case, variant, tile, parts))
        got, want = fold(out.stats.buf, out.stats.slots), conv_ref.group_sums(v)
        assert np.allclose(got, want, rtol=1e-12, atol=1e-9), (variant, np.abs(got - want).max())
        force_tile(tile)
        y2 = _chw(nat.conv2d_gn(out, cw2, gn=G, act=1, slope=0.2))
        err = common.rel_err(y2, conv_ref.conv(v, w2, b2, gn=(gamma, beta), slope=0.2))
        print("conv tiles: consumer of case %s %s tile %s parts %d: rel_err %.3e" % (case, variant, tile, parts, err))
        _note(tile, parts, err)
        assert err < TOL[parts], (variant, err)


# ---------------------------------------------------------------- the sum in the epilogue

@pytest.mark.parametrize("tile,parts", TILE_PARTS)
def test_sum_in_the_epilogue_on_every_tile(env, force_tile, tile, parts):
    """surs_conv2d_nhwc_gn_sum / surs_conv2d_nhwc_sum on the smallest map of whole tiles, as
    test_gpu_encoder_net.py::test_conv_with_the_sum_in_its_epilogue_against_conv_then_add has them on the 4-row tile: the value and
    value + residual (channels [64, 128) of a 256-channel sum) against conv2d_gn + add3 under the same tile, bit for bit, and
    against float64; both sets of statistics; the form without the first output; what the entry point refuses."""
    from surs_amd._lib import SursError
    nat, g, dev = env["native"], env["g"], env["dev"]
    h, w, cin, cout, ctot, c0 = 16, 64, 64, 64, 256, 64
    rows, chans = tile_of(tile, parts)
    xh = prng.uniform("ux", 1, (cin, h, w), -1, 1)
    xin_h = prng.uniform("ur", 2, (ctot, h, w), -1, 1)
    wt = prng.uniform("uw", 3, (cout, cin, 3, 3), -0.2, 0.2)
    gam_h, bet_h = prng.uniform("ug", 4, (cin,), 0.5, 1.5), prng.uniform("ub", 4, (cin,), -0.3, 0.3)
    gam, bet = _dev(env, gam_h), _dev(env, bet_h)
    x, xin = g.upload_nhwc(xh), g.upload_nhwc(xin_h)
    cw = nat.ConvWeights(wt, None, dev, reduced=parts == 1)
    force_tile(tile)
    x0 = nat.add3(x, x, want_stats=True)     # a producer that leaves statistics: x0 = 2 x (exact)
    ref_raw = nat.conv2d_gn(x0, cw, gn=(gam, bet), want_stats=True)
    ref_sum = nat.add3(ref_raw, xin.slice(c0, cout))
    res = xin.slice(c0, cout)
    cap = _slots(h, w, 4)
    call = ConvSum(x0, cw, gam, bet, cap, parts)

    def fresh(c):
        img = nat.Img(h, w, c, device=dev)
        img.buf.fill_(CANARY)
        return img

    # 192 channels: 6 per group is no power of two
    with pytest.raises(SursError, match="bad statistics of the sum"):
        call(fresh(cout), res, fresh(192).slice(c0, cout), c0 // 6, 6)
    raw, out = fresh(cout), fresh(ctot)
    cg, g0 = ctot // 32, c0 // (ctot // 32)
    n = call(raw, res, out.slice(c0, cout), g0, cg)
    assert n == _slots(h, w, rows) == call.s_out.slots[0] == ref_raw.stats.slots and call.s_out.pitch == n
    assert torch.equal(hwc(raw), hwc(ref_raw))
    assert torch.equal(hwc(out.slice(c0, cout)), hwc(ref_sum))
    full = hwc(out)
    assert bool((full[..., :c0] == CANARY).all()) and bool((full[..., c0 + cout:] == CANARY).all())
    # the statistics: sums of the stored values
    got1, want1 = fold(call.sb1, n), conv_ref.group_sums(_chw(raw))
    assert np.allclose(got1, want1, rtol=1e-12, atol=1e-9), np.abs(got1 - want1).max()
    assert np.allclose(got1, fold(ref_raw.stats.buf, n), rtol=1e-12, atol=1e-9)
    ng = cout // cg
    want2 = conv_ref.group_sums(_chw(out.slice(c0, cout)), groups=ng)
    sb2 = call.sb2.view(32, cap, 2)
    got2 = sb2[g0:g0 + ng, :n].sum(1).cpu().numpy()
    assert np.allclose(got2, want2, rtol=1e-12, atol=1e-9), np.abs(got2 - want2).max()
    assert float(sb2[:g0].abs().max()) == 0.0 and float(sb2[g0 + ng:].abs().max()) == 0.0     # other groups: untouched
    # against float64
    ref = conv_ref.conv(2 * xh, wt, gn=(gam_h, bet_h)) + xin_h[c0:c0 + cout].astype(np.float64)
    err = common.rel_err(_chw(out.slice(c0, cout)), ref)
    print("conv tiles: sum in the epilogue, tile %s parts %d: rel_err %.3e" % (tile, parts, err))
    _note(tile, parts, err)
    assert err < TOL[parts]
    # without the first output (a ConvBlock's last convolution, whose value nobody reads): the same sum; its statistics cannot be asked for
    out_b = fresh(ctot)
    assert call(None, res, out_b.slice(c0, cout), g0, cg, raw_stats=False) == n
    assert torch.equal(hwc(out_b), hwc(out))
    with pytest.raises(SursError, match=r"GroupNorm\(32\) output statistics"):
        call(None, res, fresh(ctot).slice(c0, cout), g0, cg)
    # without any statistics (constant coefficients in): conv2d + add3 under the same tile
    sc, sh = nat.groupnorm_coeffs(x0, gam, bet)
    ref_raw_c = nat.conv2d(x0, cw, in_scale=sc, in_shift=sh)
    ref_sum_c = nat.add3(ref_raw_c, res)
    raw_c, out_c = fresh(cout), fresh(ctot)
    call(raw_c, res, out_c.slice(c0, cout), 0, 0, stats=False)
    assert torch.equal(hwc(raw_c), hwc(ref_raw_c)) and torch.equal(hwc(out_c.slice(c0, cout)), hwc(ref_sum_c))
    assert common.rel_err(_chw(out_c.slice(c0, cout)), ref) < TOL[parts]
    out_d = fresh(ctot)
    call(None, res, out_d.slice(c0, cout), 0, 0, stats=False)
    assert torch.equal(hwc(out_d), hwc(out_c))
    # the refusal follows the tile: 12 rows are whole tiles of 4 rows only, 32 channels whole tiles of 32 only
    if rows == 4:
        assert call(fresh(cout), res, fresh(ctot).slice(c0, cout), g0, cg, h=12) == _slots(12, w, 4)
    else:
        with pytest.raises(SursError, match="whole tiles"):
            call(fresh(cout), res, fresh(ctot).slice(c0, cout), g0, cg, h=12)
    call32 = ConvSum(x0, nat.ConvWeights(wt[:32], None, dev, reduced=parts == 1), gam, bet, cap, parts)
    if chans == 32:
        assert call32(fresh(32), xin.slice(c0, 32), fresh(ctot).slice(c0, 32), g0, cg) == n
    else:
        with pytest.raises(SursError, match="whole tiles"):
            call32(fresh(32), xin.slice(c0, 32), fresh(ctot).slice(c0, 32), g0, cg)


# ---------------------------------------------------------------- the selection rule at its defaults

def test_tile_selection_at_the_default_thresholds(env, force_tile):
    """conv_x3_tile() with conv_tall_min_wg = 256, conv_wide_min_wg = 512: the boundary every bit-equality pin of the encoder rests on.
    The slot count of the statistics tells the rows; the 64-channel tile is told by its bits."""
    import os
    nat, g = env["native"], env["g"]
    for k, env_name, default in zip(TILE_OPTIONS, ("SURS_CONV_TALL_MIN_WG", "SURS_CONV_WIDE_MIN_WG"), (256, 512)):
        assert _entry[k] == int(os.environ.get(env_name, default))
    # 32 -> 256 channels at 64 x 128: 8 x 4 pixel tiles of 8 rows x 8 channel tiles = 256 workgroups: 8 rows; at 56 x 128, 224: 4 rows
    d = conv_ref.inputs("tk", 5, 32, 256, 64, 128)
    cw = nat.ConvWeights(d["w"], d["b"], env["dev"])
    force_tile("defaults")
    assert nat.conv2d_gn(g.upload_nhwc(d["x"]), cw, want_stats=True).stats.slots == 4 * 8
    assert nat.conv2d_gn(g.upload_nhwc(d["x"][:, :56]), cw, want_stats=True).stats.slots == 4 * 14
    # 16 -> 128 channels at 128 x 512: 16 x 16 pixel tiles x 2 blocks of 64 channels = 512: 8 x 64; at 120 x 512, 480: 8 x 32
    d = conv_ref.inputs("tq", 6, 16, 128, 128, 512)
    cw = nat.ConvWeights(d["w"], d["b"], env["dev"])
    X, X120 = g.upload_nhwc(d["x"]), g.upload_nhwc(d["x"][:, :120])
    got, got120 = nat.conv2d(X, cw), nat.conv2d(X120, cw)
    force_tile("8x64")
    wide, wide120 = nat.conv2d(X, cw), nat.conv2d(X120, cw)
    force_tile("8x32")
    tall, tall120 = nat.conv2d(X, cw), nat.conv2d(X120, cw)
    assert torch.equal(got.buf, wide.buf) and torch.equal(got120.buf, tall120.buf)
    assert not torch.equal(wide.buf, tall.buf) and not torch.equal(wide120.buf, tall120.buf)   # (or the lines above would tell nothing)


# ---------------------------------------------------------------- the pointwise kernel's two instantiations

@pytest.mark.parametrize("cin,cout,h,w", [
    (64, 128, 5, 7),     # fewer than 128 pixels; two channel blocks of conv1x1_x2_kernel<1>
    (32, 96, 3, 43),     # 129 pixels: a second pixel block of one pixel; ragged channels
    (64, 512, 9, 15),    # conv1x1_x2_kernel<4> with two channel blocks
])
def test_pointwise_conv_instantiations(env, cin, cout, h, w):
    nat, g, dev = env["native"], env["g"], env["dev"]
    d = conv_ref.inputs("tp", cout, cin, cout, h, w, k=1)
    cw = nat.ConvWeights(d["w"], d["b"], dev)
    wide = nat.Img(h, w, cout + 40, device=dev)
    wide.buf.fill_(CANARY)
    out, stats = wide.slice(24, cout), (cout // 32) & (cout // 32 - 1) == 0
    kw = dict(out=out, act=1, slope=0.2, residual=g.upload_nhwc(d["res"]))
    if stats:
        nat.conv2d_gn(g.upload_nhwc(d["x"]), cw, want_stats=True, **kw)
    else:     # (96 channels: 3 per group, no statistics)
        nat.conv2d(g.upload_nhwc(d["x"]), cw, **kw)
    full = _chw(wide)
    assert np.array_equal(full[:24], np.full((24, h, w), CANARY, np.float32)) and np.array_equal(full[24 + cout:], np.full((16, h, w), CANARY, np.float32))
    v = full[24:24 + cout]
    err = common.rel_err(v, conv_ref.conv(d["x"], d["w"], d["b"], slope=0.2, residual=d["res"]))
    print("conv tiles: pointwise %d -> %d at %d x %d: rel_err %.3e" % (cin, cout, h, w, err))
    assert err < TOL[2]
    if stats:
        assert out.stats.slots == -(-h * w // 128)
        got, want = fold(out.stats.buf, out.stats.slots), conv_ref.group_sums(v)
        assert np.allclose(got, want, rtol=1e-12, atol=1e-9), np.abs(got - want).max()


def test_options_are_back_at_their_entry_values(env):
    """(last in the module) the forced tiles are process-wide; every later test of the run depends on the defaults."""
    for k in sorted(_worst):
        print("conv tiles: worst rel_err against float64 on tile %s with %d part(s): %.3e" % (k[0], k[1], _worst[k]))
    assert _entry and {k: env["native"].get_option(k) for k in TILE_OPTIONS} == _entry
