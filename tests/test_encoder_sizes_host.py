"""CPU-only: the size queries of csrc/surs_encoder_net.cpp against recorded values.

Every tape and workspace there is laid out by running the network's one sequencing over a counting allocator, so a size is a
function of the ORDER of the allocator's takes.  The numbers below were recorded on the build before inference, tape and backward
were merged onto one sequencing per network; equality on all of these nets is the evidence a machine without a GPU can give that
the sequencing still takes the same maps in the same order (the tape's layout in particular)."""
import ctypes as C

from surs_amd import _lib

FAKE = C.c_void_p(4096)   # a non-null pointer: the queries read shapes and flags only


def _net(residual=1, n_block=(2, 2, 2), stacks=4, depth=2, batch=False, scale=None):
    """A SursEncoderNet of the released shapes with no weights behind it (the super-resolution convolutions as in
    test_sr_grads_host._host_net, image_filter_lr's blocks as in test_hg_grads_host._host_net)."""
    cv = lambda cin, cout, k=3: _lib.Conv(None, None, None, cin, cout, k, 0)
    hv = lambda cin, cout, k=3: _lib.Conv(FAKE, FAKE, None, cin, cout, k, 0)
    blk = lambda: _lib.ConvBlock((_lib.Conv * 3)(hv(256, 128), hv(128, 64), hv(64, 64)),
                                 (_lib.GroupNorm * 3)(*[_lib.GroupNorm(FAKE, FAKE) for _ in range(3)]))
    n, keep = _lib.EncoderNet(), []
    n.residual, n.num_stack, n.hg_depth, n.parts, n.flags = residual, stacks, depth, 2, 0
    n.n_block = (C.c_int * 3)(*n_block)
    n.head = cv(3, 32)
    n.down = (_lib.Conv * 3)(cv(32, 32), cv(64, 64), cv(128, 128))
    n.tail0 = (_lib.Conv * 3)(cv(32, 32), cv(64, 64), cv(128, 128))
    n.tail2 = (_lib.Conv * 3)(cv(32, 64), cv(64, 128), cv(128, 256))
    n.bottleneck, n.bott2, n.ups2, n.ups3, n.ups4 = cv(256, 256), cv(512, 512), cv(256, 256), cv(128, 128), cv(64, 64)
    n.last0, n.last2, n.conv5 = cv(64, 32), cv(32, 3), cv(64, 64, 1)

    def array(kind, items):
        arr = (kind * max(1, len(items)))(*items)
        keep.append(arr)
        return arr

    n.body = array(_lib.Conv, [cv(c, c) for c, nb in zip((32, 64, 128), n_block) for _ in range(2 * nb)])
    n.conv2 = blk()
    n.hg = array(_lib.ConvBlock, [blk() for _ in range(stacks * (3 * depth + 1))])
    n.top_m = array(_lib.ConvBlock, [blk() for _ in range(stacks)])
    n.conv_last = array(_lib.Conv, [hv(256, 256, 1) for _ in range(stacks)])
    n.l = array(_lib.Conv, [hv(256, 256, 1) for _ in range(stacks)])
    n.next = array(_lib.Conv, [hv(256, 256, 1) for _ in range(stacks)])
    n.bn_end = array(_lib.GroupNorm, [_lib.GroupNorm(FAKE, FAKE) for _ in range(stacks)])
    if batch or scale:
        n.flags |= _lib.ENC_EXTENDED
        n.norm, n.sr_scale = (_lib.NORM_BATCH if batch else _lib.NORM_GROUP), scale or 2
    if batch:
        bns = lambda count: array(_lib.BatchNorm, [_lib.BatchNorm(FAKE, FAKE) for _ in range(count)])
        n.bn_conv2, n.bn_hg, n.bn_top_m, n.bn_end_bn = bns(3), bns(3 * stacks * (3 * depth + 1)), bns(3 * stacks), bns(stacks)
    return n, keep


NETS = {
    "released": dict(),
    "no_residual": dict(residual=0),
    "depth1_stack1": dict(stacks=1, depth=1),
    "batch": dict(batch=True),
    "scale1": dict(scale=1),
    "scale4": dict(scale=4),
}
IMAGES = ((8, 8), (16, 24), (64, 96), (512, 512))
IMAGES_SCALE1 = ((32, 32), (64, 96), (512, 512))   # depth 2 at scale 1: feature_lr is a quarter of the image, a multiple of 4
MAPS = ((3, 5), (8, 12), (128, 128))               # 3 x 5: a single ConvBlock only (the hourglass refuses it: 0)
IMAGE_QUERIES = ("surs_encoder_workspace_bytes", "surs_encoder_sr_tape_bytes", "surs_encoder_sr_backward_workspace_bytes")
MAP_QUERIES = ("surs_encoder_convblock_tape_bytes", "surs_encoder_convblock_backward_workspace_bytes",
               "surs_encoder_hourglass_tape_bytes", "surs_encoder_hourglass_backward_workspace_bytes")


def measure():
    lib = _lib.lib()
    got = {}
    for name, kw in NETS.items():
        n, keep = _net(**kw)
        images = [[h, w] + [getattr(lib, q)(C.byref(n), h, w) for q in IMAGE_QUERIES]
                  for h, w in (IMAGES_SCALE1 if name == "scale1" else IMAGES)]
        maps = [[h, w] + [getattr(lib, q)(C.byref(n), h, w) for q in MAP_QUERIES] for h, w in MAPS]
        got[name] = (images, maps)
    return got


# per net: ([h, w, workspace, sr_tape, sr_backward_workspace] per image, [h, w, convblock_tape, convblock_backward_workspace,
# hourglass_tape, hourglass_backward_workspace] per map); 0: refused (--norm batch has no hourglass gradients, 3 x 5 is no multiple
# of 2^depth)
EXPECTED = {
    'released': ([[8, 8, 3186944, 343040, 9710080], [16, 24, 3355904, 2058240, 11061760], [64, 96, 23298304, 32931840, 35392000], [512, 512, 1174274304, 1405091840, 1258553856]],
        [[3, 5, 575488, 1229312, 0, 0], [8, 12, 824320, 1480192, 1206784, 1541632], [128, 128, 50861056, 69739520, 109440000, 80225280]]),
    'no_residual': ([[8, 8, 3186944, 285696, 9710080], [16, 24, 3355904, 1714176, 11061760], [64, 96, 23298304, 27426816, 35392000], [512, 512, 1174274304, 1170210816, 1258553856]],
        [[3, 5, 575488, 1229312, 0, 0], [8, 12, 824320, 1480192, 1206784, 1541632], [128, 128, 50861056, 69739520, 109440000, 80225280]]),
    'depth1_stack1': ([[8, 8, 3186944, 343040, 9710080], [16, 24, 3355904, 2058240, 11061760], [64, 96, 23298304, 32931840, 35392000], [512, 512, 994050304, 1405091840, 1258553856]],
        [[3, 5, 575488, 1229312, 0, 0], [8, 12, 824320, 1480192, 1119232, 1529344], [128, 128, 50861056, 69739520, 97767424, 78128128]]),
    'batch': ([[8, 8, 242944, 343040, 9710080], [16, 24, 1456384, 2058240, 11061760], [64, 96, 23298304, 32931840, 35392000], [512, 512, 1168113920, 1405091840, 1258553856]],
        [[3, 5, 0, 0, 0, 0], [8, 12, 0, 0, 0, 0], [128, 128, 0, 0, 0, 0]]),
    'scale1': ([[32, 32, 3288320, 1372160, 10521088], [64, 96, 5824768, 8232960, 15927808], [512, 512, 294224128, 351272960, 314638848]],
        [[3, 5, 575488, 1229312, 0, 0], [8, 12, 824320, 1480192, 1206784, 1541632], [128, 128, 50861056, 69739520, 109440000, 80225280]]),
    'scale4': ([[8, 8, 3288320, 1372160, 10521088], [16, 24, 5824768, 8232960, 15927808], [64, 96, 101843200, 131727360, 122688000], [512, 512, 4691853568, 5620367360, 5034213888]],
        [[3, 5, 575488, 1229312, 0, 0], [8, 12, 824320, 1480192, 1206784, 1541632], [128, 128, 50861056, 69739520, 109440000, 80225280]]),
}


def test_every_size_query_returns_the_recorded_value():
    got = measure()
    assert list(got) == list(EXPECTED)
    for name in EXPECTED:
        assert got[name] == EXPECTED[name], name
