"""SuRSNet: the drop-in boundary.

Same public surface as the reference's `SuRSNet(BaseSuRSNet)` as consumed by eval_SuRS.py / gen_mesh /
reconstruction (/root/reference/lib/model/SuRSNet.py:44-187, lib/model/BaseSuRSNet.py:20-26,80-85;
SURVEY.md section 8b): name, num_views, to(), eval(), train(), state_dict(), load_state_dict(), parameters(),
super_res(), filter_hr(), filter_lr(), query_mr(), query_sr(), get_preds(), and - SuRSNet.py:196-266 - get_error_lr(), get_error_hr(),
get_errorSR(), get_error_disp_1(), forward().

It is NOT a torch.nn.Module: parameters are a flat ordered dict keyed exactly like the reference's state dict
(all 553 keys, strict; 1036 with --norm batch), and every forward method sequences hand-written HIP kernels through the C ABI.  There is
no autograd graph and no CPU path: methods raise without a GPU / built library (the optimiser over the parameter sets is optim.Optimizer).  forward() is the
VALIDATION forward: every kept stack's predictions and the reference's loss, without an autograd graph (SuRSNet.py:240-266).
The one part of the backward pass that exists is the classifiers': forward_backward() / classifier_grads() return d error / d (every
mlp_lr.* and mlp_hr.* parameter) and, with features=True, d error / d (the feature maps of im_feat_list_lr and im_feat_list_hr[0])
(native.mlp_grads) - where an encoder's backward starts; autograd.point_loss hands them to torch autograd.  The super-resolution
network and image_filter_hr.conv5 have a backward too: super_res_train() keeps the forward's maps, super_res_backward() returns the
gradients of every super_resolution.* convolution and conv5 from the gradients of img_SR, feature_lr and im_feat_list_hr[0]
(native.sr_backward), sr_parameters() are the fp32 weights it reads, autograd.super_res_features is the torch.autograd.Function over
them.  The hourglass filter (image_filter_lr.*) has a backward too (--norm group): per module, conv_block_train() /
conv_block_backward(), hourglass_train() / hourglass_backward() (native.hg_backward), stack_tail_train() / stack_tail_backward()
(native.tail_backward), and as a whole, filter_lr_train() / filter_lr_backward() (native.filter_lr_backward); hg_parameters() are the
fp32 weights they read, autograd.conv_block, autograd.hourglass, autograd.stack_tail and autograd.filter_lr the Functions over them;
forward_backward(encoder=True) returns the gradients of all three parameter sets from one taped forward.

Encoder options: --norm group | batch and --scale 1..4 (anything else: ValueError at construction).  --norm batch is nn.BatchNorm2d in
EVAL mode - y = (x - running_mean) / sqrt(running_var + 1e-5) * weight + bias, always from the running statistics: train() here keeps
every stack's output as the reference does but never switches to batch statistics; num_batches_tracked is loaded, kept and returned by
state_dict(), and otherwise ignored.  --scale s: img_SR [V,3,sH,sW], feature_lr [V,256,sH/4,sW/4], feature_hr [V,64,sH,sW].
--hg_dim D (multiples of 16 from 16 to 512): im_feat_list_lr [V,D,.,.]; the classifiers then read D + 65 / D + 66 channels
(--mlp_dim_lr / --mlp_dim_hr must start with them) and run on the fused evaluators of native.query_points_generic.
"""
from collections import OrderedDict

import math

import numpy as np
import torch

from . import encoder, native, weights


def _as_nchw_view(img):
    """zero-copy NCHW-shaped (channels_last strided) torch view of an NHWC Img with ld == c."""
    assert img.ld == img.c and img.off == 0
    return img.buf.view(1, img.h, img.w, img.c).permute(0, 3, 1, 2)


def _cat_views(imgs):
    """The [B,C,h,w] batch of the NHWC Imgs `imgs` of one shape: a zero-copy view of a single one."""
    return torch.cat([_as_nchw_view(i) for i in imgs], 0) if len(imgs) > 1 else _as_nchw_view(imgs[0])


def _as_img(t):
    """torch [1,C,H,W] (any layout) or [C,H,W] -> NHWC Img; zero-copy when it already is channels_last."""
    if t.dim() == 3:
        t = t.unsqueeze(0)
    assert t.dim() == 4 and t.shape[0] == 1 and t.dtype == torch.float32
    _, c, h, w = t.shape
    p = t.permute(0, 2, 3, 1)
    if p.is_contiguous() and t.is_cuda:
        return native.Img(h, w, c, c, p.reshape(-1))
    dev = native.require_gpu()
    return native.Img.from_nchw(t.to(dev).contiguous())


class SuRSNet:
    def __init__(self, opt, projection_mode="orthogonal", error_term=None):
        if projection_mode not in ("orthogonal", "perspective"):
            raise ValueError("projection_mode must be 'orthogonal' or 'perspective' (BaseSuRSNet.py:26)")
        self.projection_mode = projection_mode
        self.name = "base"
        self.opt = opt
        self.num_views = opt.num_views
        self.training = True
        self.device = torch.device("cpu")
        self.precision = getattr(opt, "precision", "fp32")
        self._spec = weights.state_dict_spec(opt)            # (--norm other than group | batch: ValueError)
        encoder.check_scale(getattr(opt, "scale", 2))        # (--scale outside 1..4: ValueError)
        native.check_hg_dim(getattr(opt, "hg_dim", 256))     # (--hg_dim not a multiple of 16 in 16..512: ValueError)
        # reference init: normal(0, 0.02) conv weights, zero bias, GroupNorm 1/0 (lib/net_util.py:99-132); here the
        # constructor leaves deterministic synthetic weights in place until load_state_dict() replaces them
        self._sd = OrderedDict((k, torch.from_numpy(v)) for k, v in weights.synthetic_state_dict(opt, seed=0).items())
        self._enc = None
        self._blob = None
        self._generic = None
        self._ws = None
        self.im_feat_list_lr = []
        self.im_feat_list_hr = []
        self.im_SR = self.feature_lr = self.feature_hr = None
        self.preds_lr = self.preds_hr = None
        self.intermediate_preds_list_lr = []
        self.intermediate_preds_list_hr = []
        self._mr_points = None
        self._mr_hr = None
        self._sr_points = None        # query_sr's points and (calibs, transforms): what classifier_grads() differentiates
        self._sr_args = None
        # "mlp" / "sr" / "hg" -> (native.MlpParams / SrParams / HgParams: the plain fp32 device masters, {mlp,sr,hg}_parameters()'s
        # OrderedDict of torch.nn.Parameter over them), for the sets asked for so far (dropped like the blob)
        self._param_sets = {}
        self._stale = set()           # commit(): the keys of _sd whose current values are on the device (the masters'), not yet in _sd
        self._grad_ws = None
        # what the last *_train() of each module left for its *_backward(): module -> (h, w, [one tape per image]); the modules are
        # SR_TAPES (the super-resolution net), a ConvBlock's full prefix, an hourglass's stack index, ("tail", s) and "filter_lr"
        self._tapes = {}
        self._train_ws = None         # the *_backward() calls' workspace: one buffer, grown to the largest asked for
        self.last_classifier_grads = None   # what autograd.point_loss last left: classifier_grads()'s OrderedDict
        self._feat_cache = None
        self._stack_feat_cache = None
        self.labels_lr = self.labels_hr = None
        self._mr_version = 0
        self._sharded_encode = None   # dist.encode_sharded's arguments + the tensor it produced (the overflow retry of slab mode)
        self._last_images = None      # what super_res() last ran on, and which buffers came out of that run (reencode_wide)
        self._sr_out = self._lr_from = self._hr_from = None

    # ------------------------------------------------------------------ nn.Module-like plumbing
    def to(self, device=None, **kw):
        if device is not None:
            device = torch.device(device)
            if device.type == "cuda" and device.index is None:
                device = torch.device("cuda", torch.cuda.current_device())
            self._write_back()   # (committed values live in the masters dropped below: into _sd first)
            self.device = device
            if self._enc is not None:
                encoder.drop_graphs(self._enc)
            self._enc = self._blob = None
            self._grad_ws = self._train_ws = None
            self._param_sets, self._tapes = {}, {}
        return self

    def cuda(self, index=None):
        return self.to(torch.device("cuda", index if index is not None else torch.cuda.current_device()))

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def state_dict(self):
        self._write_back()
        return OrderedDict((k, v.clone()) for k, v in self._sd.items())

    def parameters(self):
        self._write_back()
        return iter(self._sd.values())

    def _masters(self):
        """name of each parameter set -> its device masters (state-dict key -> tensor), for the sets that exist."""
        return OrderedDict((w, self._param_sets[w][0].tensors) for w in self.SETS if w in self._param_sets)

    def _write_back(self):
        """Downloads the keys commit() marked stale from their device masters into _sd (the spec's shapes: [out,in,1] classifier
        weights).  Everything that reads _sd, or drops a master, calls this first; nothing to do when nothing was committed."""
        if not self._stale:
            return
        shape = {k: tuple(sh) for k, sh, _ in self._spec}
        for tensors in self._masters().values():
            for k, t in tensors.items():
                if k in self._stale:
                    self._sd[k] = t.detach().to("cpu", torch.float32).reshape(shape[k]).contiguous()
                    self._stale.discard(k)
        assert not self._stale, "committed keys without a master: %s" % sorted(self._stale)[:3]

    SETS = ("mlp", "sr", "hg")

    def commit(self, which=None):
        """Makes the forward run on the CURRENT values of the device masters - mlp_parameters(), sr_parameters(), hg_parameters(): what
        an optimiser has just stepped - without leaving the device: the packed encoder images (EncoderWeights.refresh: surs_conv_repack,
        surs_conv1x1_merge), the classifier blob in its own dtype (surs_mlp_repack, or surs_mlp_repack_generic for any other shape) are
        rewritten in place on the current stream, with no synchronisation; no address changes, so the library's network struct and
        captured graphs stay valid.  `which`: a subset of ("mlp", "sr", "hg"); default: every set whose master exists.  The keys of the
        committed sets are then current on the device only: state_dict() / parameters() download them on demand (every other key -
        bn4, the unused parts of image_filter_hr, the mean shifts, downsample.0's aliases - keeps its loaded value), to() writes them
        back before it drops the masters, load_state_dict() replaces them.  Feature maps and predictions computed before the call
        are those of the old weights.  "hg" under --norm batch: NotImplementedError (no backward; the constants are folded)."""
        if which is None:
            which = tuple(self._masters())
        elif isinstance(which, str):
            which = (which,)
        which = tuple(which)
        for w in which:
            if w not in self.SETS:
                raise ValueError("commit: unknown parameter set %r; the sets are %s" % (w, self.SETS))
        if "hg" in which and weights.check_norm(getattr(self.opt, "norm", "group")) == "batch":
            raise NotImplementedError("commit('hg'): --norm group only (a BatchNorm encoder has no backward and its constants are folded "
                                      "on the host)")
        self._device()
        masters = self._masters()
        for w in which:
            if w not in masters:
                raise RuntimeError("commit(%r): %s_parameters() has not been asked for: there is nothing to commit" % (w, w))
        enc = OrderedDict()
        for w in ("sr", "hg"):
            if w in which:
                enc.update(masters[w])
        if enc and self._enc is not None:    # (not packed yet: the next use packs from the written-back values)
            self._enc.refresh(enc)
        if "mlp" in which and self._blob is not None:
            if self._generic is not None:
                native.mlp_repack_generic(self._param_sets["mlp"][0], self._generic)
            else:
                native.mlp_repack(self._param_sets["mlp"][0], self._blob, self._core_dtype)
        for w in which:
            self._stale.update(masters[w])
        return self

    def mlp_parameters(self):
        """The cached OrderedDict of torch.nn.Parameter over the plain fp32 device copies of every mlp_lr.* / mlp_hr.* tensor
        (state_dict() order; weights [out, in], biases [out]: the shapes native.MlpParams holds): what classifier_grads() reads and an
        optimiser steps.  The FORWARD runs on the packed blob: commit() after a step."""
        return self._param_set("mlp")[1]

    def _param_set(self, which):
        """(the native.MlpParams / SrParams / HgParams of set `which` of SETS, the OrderedDict of torch.nn.Parameter over its tensors),
        built from the current values on first use."""
        if which not in self._param_sets:
            self._write_back()
            if which == "mlp":
                sd = {k: v for k, v in self._sd.items() if k.startswith("mlp_")}
                shapes = native.mlp_shapes({k: v.numpy() for k, v in sd.items()}, self.opt)
                p = native.MlpParams(sd, self._device(), shapes)
            elif which == "sr":
                p = native.SrParams(self._sd, self.opt.n_block, self._device())
            else:
                p = native.HgParams(self._sd, self.opt.num_stack_lr, self.opt.hg_depth, self._device())
            self._param_sets[which] = (p, OrderedDict((k, torch.nn.Parameter(v)) for k, v in p.tensors.items()))
        return self._param_sets[which]

    def load_state_dict(self, sd, strict=True):
        self._write_back()   # (a key `sd` lacks keeps its CURRENT value: a committed one lives in a master dropped below)
        want = {k: tuple(s) for k, s, _ in self._spec}
        int_keys = {k for k, _, kind in self._spec if kind.endswith("bn_nbt") or kind.endswith("num_batches_tracked")}
        missing = [k for k in want if k not in sd]
        unexpected = [k for k in sd if k not in want]
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict for SuRSNet: missing %s, unexpected %s" %
                               (missing[:5], unexpected[:5]))
        new = OrderedDict()
        for k, shape in want.items():
            if k in sd:
                v = sd[k]
                dt, npdt = (torch.int64, np.int64) if k in int_keys else (torch.float32, np.float32)   # (num_batches_tracked)
                v = v.detach().to("cpu", dt) if torch.is_tensor(v) else torch.from_numpy(np.asarray(v, npdt))
                if tuple(v.shape) != shape:
                    raise RuntimeError("size mismatch for %s: %s vs %s" % (k, tuple(v.shape), shape))
                new[k] = v.contiguous()
            else:
                new[k] = self._sd[k]
        self._sd = new
        self._stale = set()
        if self._enc is not None:
            encoder.drop_graphs(self._enc)
        self._enc = self._blob = None
        self._param_sets = {}
        return self

    # ------------------------------------------------------------------ lazily packed device state
    def _device(self):
        if self.device.type != "cuda":
            raise RuntimeError("SuRSNet has no CPU path: call .to(device=torch.device('cuda:N')) first")
        return self.device

    def _encoder_weights(self):
        if self._enc is None:
            self._write_back()
            self._enc = encoder.EncoderWeights(self._sd, self.opt, self._device())
        return self._enc

    def _mlp_blob(self):
        if self._blob is None:
            self._write_back()
            sd = {k: v.numpy() for k, v in self._sd.items() if k.startswith("mlp_")}
            shapes = native.mlp_shapes(sd, self.opt)
            if native.is_default_mlp(shapes):
                self._generic = None
                self._blob, self._core_dtype = native.pack_mlp(sd, self.precision, self._device())
            else:
                # any other --mlp_dim_* / --mlp_res_layers_* / --no_residual: the fused evaluator (surs_query_points_generic)
                self._generic = native.pack_mlp_generic(sd, self._device(), shapes)
                self._blob = self._generic.blob
                self._core_dtype = native.DTYPES["bf16" if self.precision == "fp32" else self.precision]
        return self._blob

    def generic_mlp(self):
        """The packed classifiers (native.GenericMlp) when their shape is not the released one, else None."""
        self._mlp_blob()
        return self._generic

    def _workspace(self):
        if self._ws is None:
            self._ws = native.Workspace(self._device())
        return self._ws

    # ------------------------------------------------------------------ encoder
    def super_res(self, images):
        """images [V,3,H,W] -> (img_SR [V,3,2H,2W], feature_lr [V,256,H/2,W/2], feature_hr [V,64,2H,2W]); with --scale s:
        [V,3,sH,sW], [V,256,sH/4,sW/4], [V,64,sH,sW]."""
        W = self._encoder_weights()
        self._last_images = images   # (kept for reencode_wide: the retry after an f16 overflow)
        self._sharded_encode = None  # (features about to be made by THIS device's encoder: dist.encode_sharded's record is stale)
        # (one view: through the captured HIP graph - encoder.graphed; several views would share the graph's output buffers)
        sr = encoder.super_res_g if (images.shape[0] == 1 or encoder.native_enabled(W)) else encoder.super_res
        outs = [sr(W, _as_img(images[v:v + 1])) for v in range(images.shape[0])]
        cat = lambda i: torch.cat([_as_nchw_view(o[i]) for o in outs], 0) if len(outs) > 1 else _as_nchw_view(outs[0][i])
        self.im_SR, self.feature_lr, self.feature_hr = cat(0), cat(1), cat(2)
        self._sr_out = (self.feature_lr.data_ptr(), self.feature_hr.data_ptr())
        self._lr_from = self._hr_from = None
        return self.im_SR, self.feature_lr, self.feature_hr

    def filter_lr(self, images):
        W = self._encoder_weights()
        flr = encoder.filter_lr_g if (images.shape[0] == 1 or encoder.native_enabled(W)) else encoder.filter_lr
        per_view = [flr(W, _as_img(images[v:v + 1]), keep_all=self.training) for v in range(images.shape[0])]
        n_out = len(per_view[0])
        self._sharded_encode = None
        self._feat_lr_imgs = [[pv[i] for pv in per_view] for i in range(n_out)]
        self.im_feat_list_lr = [torch.cat([_as_nchw_view(pv[i]) for pv in per_view], 0) if len(per_view) > 1
                                else _as_nchw_view(per_view[0][i]) for i in range(n_out)]
        # (features of the last super_res()'s images only if they were computed from ITS feature_lr)
        self._lr_from = self.im_feat_list_lr[-1].data_ptr() if (self._sr_out and images.data_ptr() == self._sr_out[0]) else None

    def filter_hr(self, images):
        W = self._encoder_weights()
        per_view = [encoder.filter_hr(W, _as_img(images[v:v + 1])) for v in range(images.shape[0])]
        self._sharded_encode = None
        self._feat_hr_imgs = [[pv[0] for pv in per_view]]
        self.im_feat_list_hr = [torch.cat([_as_nchw_view(pv[0]) for pv in per_view], 0) if len(per_view) > 1
                                else _as_nchw_view(per_view[0][0])]
        self._hr_from = self.im_feat_list_hr[0].data_ptr() if (self._sr_out and images.data_ptr() == self._sr_out[1]) else None

    # ------------------------------------------------------------------ training: taped forwards and their backwards
    SR_TAPES = "super_res"   # the super-resolution network's key in _tapes

    def _train(self, module, fn, *batches):
        """The per-image train forward of one module: fn(Img, ...) -> (outputs ..., tape) on every image of the [B,C,h,w] tensors
        `batches` (a None stays None), (h, w, [the tape of every image]) filed under `module` in _tapes.  Returns every image's outputs."""
        batches = [None if t is None else t.detach().to(self._device(), torch.float32) for t in batches]
        outs, tapes = [], []
        for b in range(batches[0].shape[0]):
            *o, tape = fn(*[None if t is None else _as_img(t[b:b + 1]) for t in batches])
            outs.append(o)
            tapes.append(tape)
        self._tapes[module] = (batches[0].shape[2], batches[0].shape[3], tapes)
        return outs

    def _kept_tapes(self, module, tapes, what, of=""):
        """`tapes` where given - the model is not touched -, else what the preceding {what}_train() filed under `module`."""
        if tapes is None:
            tapes = self._tapes.get(module)
        if tapes is None:
            raise RuntimeError("%s_backward needs a preceding %s_train()%s: the tape of the forward's maps is missing" % (what, what, of))
        return tapes

    def _backward(self, tapes, upstream, need, fn, nhwc=False):
        """The per-image backward of one module from `tapes` (one per image).  upstream: per output (its name, its gradient [B,c,h,w] or
        None = zero, its (c, h, w)); need: the workspace's bytes; fn(tape, [image b's NHWC gradient or None per output], grads=,
        accumulate=, workspace=) -> (the input's gradient [h,w,c] or None, grads).  The parameters' gradients are summed by the library in
        image order: the first image overwrites, the later ones add.  Returns (the input's gradient [B,c,h,w] or None, grads).
        nhwc=True (forward_backward(encoder=True)'s private route): every gradient is given in the memory the library reads - a
        contiguous [B,h,w,c] tensor or a list of B [h,w,c] tensors, handed on untouched - and the input's gradient comes back as the
        list of the B [h,w,c] tensors the library wrote: no copy on either side."""
        dev, B = self._device(), len(tapes)
        gs = []
        for name, g, shape in upstream:
            if g is not None and nhwc:
                c, h, w = shape
                if len(g) != B or any(tuple(t.shape) != (h, w, c) for t in g):
                    raise ValueError("%s %s against the output's %s in NHWC" % (name, [tuple(t.shape) for t in g][:2], (B, h, w, c)))
            elif g is not None:
                if tuple(g.shape) != (B,) + shape:
                    raise ValueError("%s %s against the output's %s" % (name, tuple(g.shape), (B,) + shape))
                g = g.detach().to(dev, torch.float32).permute(0, 2, 3, 1).contiguous()
            gs.append(g)
        # (one workspace for every module: the calls are enqueued on the current stream in order)
        if self._train_ws is None or self._train_ws.numel() < need or self._train_ws.device != dev:
            self._train_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        grads, dxs = None, []
        for b in range(B):
            dx, grads = fn(tapes[b], [None if g is None else g[b] for g in gs], grads=grads, accumulate=b > 0, workspace=self._train_ws)
            dxs.append(dx)
        if nhwc:
            return (None if dxs[0] is None else dxs), grads
        return (None if dxs[0] is None else torch.stack(dxs, 0).permute(0, 3, 1, 2)), grads

    # ------------------------------------------------------------------ super-resolution gradients
    _SR_F16 = ("super-resolution gradients: --encoder_precision f16 (net->parts == 1) has no backward: training runs the fp32-grade "
               "forward")

    def _sr_native(self):
        W = self._encoder_weights()
        if W.reduced:
            raise RuntimeError(self._SR_F16)
        return encoder._native_net(W).net, W.scale

    def _sr_param_set(self):
        return self._param_set("sr")

    def sr_parameters(self):
        """The cached OrderedDict of torch.nn.Parameter over the plain fp32 device copies of every super_resolution.* convolution and
        image_filter_hr.conv5 (state_dict() order, no sub_mean / add_mean): the tensors super_res_backward() reads, what an optimiser
        steps and autograd.super_res_features hands gradients to.  The FORWARD runs on PACKED copies: after an optimiser step,
        commit() repacks them on the device from these tensors (load_state_dict() drops this cache, as it drops the classifiers')."""
        return self._param_set("sr")[1]

    def super_res_train(self, images):
        """super_res(images) followed by filter_hr(feature_hr) - the same kernels and bits in im_SR, feature_lr, feature_hr and
        im_feat_list_hr - with every map the backward reads kept on this object, one tape per image of the batch
        (surs_encoder_super_res_train).  Returns (img_SR, feature_lr, feature_hr) as super_res() does."""
        net, scale = self._sr_native()
        self._last_images = images
        self._sharded_encode = None

        def one(x):
            encoder.check_image_size(x.h, x.w, scale)
            return native.sr_train_forward(net, x, scale)
        outs = self._train(self.SR_TAPES, one, images)
        cat = lambda i: _cat_views([o[i] for o in outs])
        self.im_SR, self.feature_lr, self.feature_hr = cat(0), cat(1), cat(2)
        self._sr_out = (self.feature_lr.data_ptr(), self.feature_hr.data_ptr())
        self._lr_from = None
        self._feat_hr_imgs = [[o[3] for o in outs]]
        self.im_feat_list_hr = [cat(3)]
        self._hr_from = self.im_feat_list_hr[0].data_ptr()
        return self.im_SR, self.feature_lr, self.feature_hr

    def super_res_backward(self, grad_img_SR=None, grad_feature_lr=None, grad_feat_hr=None, tapes=None):
        """The gradients of <grad_img_SR, img_SR> + <grad_feature_lr, feature_lr> + <grad_feat_hr, im_feat_list_hr[0]> with respect to
        every super_resolution.* convolution and image_filter_hr.conv5 (surs_encoder_super_res_backward), from the tapes of the
        preceding super_res_train().  The arguments are NCHW tensors of those outputs' shapes, or None (zero; at least one is
        needed).  Returns an OrderedDict in state_dict() order (sr_parameters()'s keys): float32 device tensors of the parameters'
        shapes, summed over the images of the batch.  fp32 matrix products whatever --precision says, deterministic.  The gradient of
        feature_lr through image_filter_lr (the hourglass) is not part of this: whoever owns that network supplies
        grad_feature_lr.  tapes: what an earlier super_res_train() filed in _tapes[SR_TAPES], to go back through THAT forward
        whatever ran since; the model's own entry is neither read nor changed."""
        return self._super_res_backward(grad_img_SR, grad_feature_lr, grad_feat_hr, tapes)

    def _super_res_backward(self, grad_img_SR, grad_feature_lr, grad_feat_hr, tapes=None, nhwc=False):
        """super_res_backward; nhwc: _backward's private NHWC route."""
        h, w, tapes = self._kept_tapes(self.SR_TAPES, tapes, "super_res")
        net, scale = self._sr_native()
        params = self._param_set("sr")[0]
        H2, W2 = scale * h, scale * w
        upstream = (("grad_img_SR", grad_img_SR, (3, H2, W2)), ("grad_feature_lr", grad_feature_lr, (256, H2 // 4, W2 // 4)),
                    ("grad_feat_hr", grad_feat_hr, (net.conv5.cout, H2, W2)))
        if all(g is None for _, g, _ in upstream):
            raise ValueError("super_res_backward: no upstream gradient (all three are None)")
        return self._backward(tapes, upstream, native.sr_backward_workspace_bytes(net, h, w),
                              lambda tape, g, **kw: (None, native.sr_backward(net, params, tape, h, w, *g, scale=scale, **kw)),
                              nhwc=nhwc)[1]

    # ------------------------------------------------------------------ hourglass gradients
    def _hg_check_norm(self):
        if weights.check_norm(getattr(self.opt, "norm", "group")) == "batch":
            raise NotImplementedError("hourglass gradients: --norm group only (a BatchNorm encoder runs in eval mode and has no backward)")

    def _hg_native(self):
        self._hg_check_norm()
        W = self._encoder_weights()
        if W.reduced:
            raise RuntimeError("hourglass gradients: --encoder_precision f16 (net->parts == 1) has no backward: training runs the "
                               "fp32-grade forward")
        return encoder._native_net(W).net

    def _hg_param_set(self):
        return self._param_set("hg")

    def hg_parameters(self):
        """The cached OrderedDict of torch.nn.Parameter over the plain fp32 device copies of every image_filter_lr.* tensor the forward
        reads (state_dict() order: the ConvBlocks' conv1-3.weight and bn1-3.weight / .bias - not bn4 -, conv_last, bn_end, l, bl, al):
        what conv_block_backward() / hourglass_backward() read and autograd.conv_block / autograd.hourglass hand gradients to.  The
        FORWARD runs on PACKED copies: commit() repacks them from these tensors after an optimiser step (load_state_dict() drops this
        cache, as it drops sr_parameters()'s)."""
        return self._param_set("hg")[1]

    def _hg_module(self, which):
        """(the library's net, the module's handle, its ConvBlock prefixes, its key in _tapes) of a stack index (its hourglass m{s},
        filed under the index) or a ConvBlock's prefix (filed under the full prefix)."""
        net = self._hg_native()
        if isinstance(which, (int, np.integer)) and not isinstance(which, bool):
            if not 0 <= which < self.opt.num_stack_lr:
                raise ValueError("stack %d of %d" % (which, self.opt.num_stack_lr))
            return net, int(which), native.hg_block_prefixes(int(which), self.opt.hg_depth), int(which)
        prefix = which if which.endswith(".") else which + "."
        if not prefix.startswith(native.HG):
            prefix = native.HG + prefix
        return net, native.hg_block_of(net, prefix, self.opt.hg_depth), [prefix], prefix

    def _hg_train(self, which, x):
        net, handle, _, module = self._hg_module(which)
        if x.dim() != 4 or x.shape[1] != 256:
            raise ValueError("a [B,256,h,w] tensor is expected, not %s" % (tuple(x.shape),))
        return _cat_views([o[0] for o in self._train(module, lambda img: native.hg_train_forward(net, handle, img), x)])

    def _hg_backward(self, which, grad_out, what, tapes):
        net, handle, prefixes, module = self._hg_module(which)
        h, w, tapes = self._kept_tapes(module, tapes, what, " of the same module")
        params = self._param_set("hg")[0].tensors
        return self._backward(tapes, [("grad_out", grad_out, (256, h, w))], native.hg_backward_workspace_bytes(net, h, w, len(prefixes) > 1),
                              lambda tape, g, **kw: native.hg_backward(net, handle, prefixes, params, tape, h, w, g[0], **kw))

    def conv_block_train(self, prefix, x):
        """ConvBlock `prefix` (image_filter_lr.conv2. / .top_m_{s}. / .m{s}.b1_{l}. ...; 'image_filter_lr.' may be left out) on x
        [B,256,h,w]: encoder.conv_block's values, with what the backward reads kept on this object, one tape per image
        (surs_encoder_convblock_train)."""
        return self._hg_train(prefix, x)

    def conv_block_backward(self, prefix, grad_out, tapes=None):
        """(d <grad_out, out> / d x [B,256,h,w], OrderedDict of the gradients of the block's nine parameters summed over the batch in
        image order) from the tapes of the preceding conv_block_train(prefix, x), or from `tapes`: what an earlier one filed in
        _tapes[the block's full prefix] (the model's own entry is neither read nor changed)."""
        return self._hg_backward(prefix, grad_out, "conv_block", tapes)

    def hourglass_train(self, stack, x):
        """image_filter_lr.m{stack} on x [B,256,h,w] (h, w multiples of 2^hg_depth): encoder.hourglass's values, tapes kept
        (surs_encoder_hourglass_train)."""
        return self._hg_train(int(stack), x)

    def hourglass_backward(self, stack, grad_out, tapes=None):
        """(d <grad_out, out> / d x, OrderedDict of the gradients of every parameter of m{stack}, blocks in module order) from the
        tapes of the preceding hourglass_train(stack, x), or from `tapes`: what an earlier one filed in _tapes[stack]."""
        return self._hg_backward(int(stack), grad_out, "hourglass", tapes)

    # ------------------------------------------------------------------ stack-tail gradients, and the whole low-resolution filter
    def stack_tail_train(self, stack, ll, previous=None):
        """The tail of stack `stack` - conv_last -> bn_end -> ReLU -> l, and next = previous + bl(.) + al(l(.)) on the merged next{s} -
        on ll [B,256,h,w] and, for every stack but the last, previous [B,256,h,w]: filter_lr()'s launches and bits, tapes kept
        (surs_encoder_tail_train).  Returns (out [B,hg_dim,h,w], next [B,256,h,w] or None for the last stack)."""
        self._hg_check_norm()
        stack, S = int(stack), self.opt.num_stack_lr
        if not 0 <= stack < S:
            raise ValueError("stack %d of %d" % (stack, S))
        if (stack == S - 1) != (previous is None):
            raise RuntimeError("stack_tail_train: previous goes with every stack but the last (stack %d of %d)" % (stack, S))
        if ll.dim() != 4 or ll.shape[1] != 256 or (previous is not None and tuple(previous.shape) != tuple(ll.shape)):
            raise ValueError("[B,256,h,w] tensors of one shape are expected, not %s" % (tuple(ll.shape),))
        net = self._hg_native()
        outs = self._train(("tail", stack), lambda l, p: native.tail_train_forward(net, stack, l, p), ll, previous)
        return _cat_views([o[0] for o in outs]), (None if previous is None else _cat_views([o[1] for o in outs]))

    def stack_tail_backward(self, stack, grad_out=None, grad_next=None, tapes=None):
        """(d L / d ll, d L / d previous - grad_next itself; None for the last stack or without grad_next -, OrderedDict of the gradients
        of conv_last{s}, bn_end{s}, l{s} and, for a stack that is not the last, bl{s}, al{s} (.weight, .bias each; the UN-MERGED
        parameters), summed over the batch in image order) for L = <grad_out, out> + <grad_next, next>, from the tapes of the preceding
        stack_tail_train(stack, ...), or from `tapes`: what an earlier one filed in _tapes[("tail", stack)].  Either gradient may be
        None (zero), not both."""
        self._hg_check_norm()
        stack = int(stack)
        if grad_out is None and grad_next is None:
            raise RuntimeError("stack_tail_backward: no upstream gradient (both are None)")
        if grad_next is not None and stack == self.opt.num_stack_lr - 1:
            raise RuntimeError("stack_tail_backward: the last stack has no next")
        h, w, tapes = self._kept_tapes(("tail", stack), tapes, "stack_tail", " of the same stack")
        net = self._hg_native()
        params = self._param_set("hg")[0].tensors
        d_ll, grads = self._backward(tapes, [("grad_out", grad_out, (net.l[stack].cout, h, w)), ("grad_next", grad_next, (256, h, w))],
                                     native.tail_backward_workspace_bytes(net, h, w),
                                     lambda tape, g, **kw: native.tail_backward(net, stack, params, tape, h, w, *g, **kw))
        return d_ll, grad_next, grads

    def filter_lr_train(self, feature_lr):
        """HGFilter.forward on feature_lr [B,256,h,w] with every map the backward reads kept, one tape per image
        (surs_encoder_filter_lr_train): the list of every stack's output [B,hg_dim,h,w], filter_lr()'s values."""
        self._hg_check_norm()
        if feature_lr.dim() != 4 or feature_lr.shape[1] != 256:
            raise ValueError("a [B,256,h,w] tensor is expected, not %s" % (tuple(feature_lr.shape),))
        net = self._hg_native()
        outs = self._train("filter_lr", lambda x: native.filter_lr_train_forward(net, x), feature_lr)
        return [_cat_views([o[0][s] for o in outs]) for s in range(len(outs[0][0]))]

    def filter_lr_backward(self, grad_outs, tapes=None):
        """(d L / d feature_lr, OrderedDict over hg_parameters()'s keys) for L = sum_s <grad_outs[s], outs[s]> from the tapes of the
        preceding filter_lr_train(), or from `tapes`: what an earlier one filed in _tapes["filter_lr"].  grad_outs holds one
        [B,hg_dim,h,w] tensor or None (zero) per stack, not all None.  Summed over the batch in image order; the parameters of a stack
        no gradient reaches get zeros."""
        return self._filter_lr_backward(grad_outs, tapes)

    def _filter_lr_backward(self, grad_outs, tapes=None, nhwc=False):
        """filter_lr_backward; nhwc: _backward's private NHWC route."""
        self._hg_check_norm()
        S = self.opt.num_stack_lr
        if len(grad_outs) != S:
            raise ValueError("one gradient (or None) per stack: %d for %d stacks" % (len(grad_outs), S))
        if all(g is None for g in grad_outs):
            raise RuntimeError("filter_lr_backward: no upstream gradient (all are None)")
        h, w, tapes = self._kept_tapes("filter_lr", tapes, "filter_lr")
        net = self._hg_native()
        hp = self._param_set("hg")[0]
        return self._backward(tapes, [("grad_outs[%d]" % s, g, (net.l[s].cout, h, w)) for s, g in enumerate(grad_outs)],
                              native.filter_lr_backward_workspace_bytes(net, h, w),
                              lambda tape, g, **kw: native.filter_lr_backward(net, self.opt.hg_depth, hp.keys, hp.tensors, tape, h, w, g, **kw),
                              nhwc=nhwc)

    def reencode_wide(self):
        """Runs the encoder again on the images of the last super_res() call with every fp32-grade product on three bf16 parts
        (native.wide_operands): what reconstruction() / query_* do when the features came out non-finite (an activation beyond
        the f16 range of the default two-part split).  Returns False - and leaves everything as it is - unless the CURRENT features
        are provably those of that call: filter_lr / filter_hr ran on its outputs and im_feat_list_* still hold what they produced.
        Features that came another way (encode_image / features=, external feature maps, im_feat_list_* assigned directly) belong
        to images this object has never seen; re-encoding the last image it did see would return a finite but wrong result."""
        if self._last_images is None or not self.im_feat_list_lr or not self.im_feat_list_hr:
            return False
        if self._lr_from is None or self._hr_from is None or self.im_feat_list_lr[-1].data_ptr() != self._lr_from \
                or self.im_feat_list_hr[0].data_ptr() != self._hr_from:
            return False
        with native.wide_operands():
            _, f_lr, f_hr = self.super_res(self._last_images)
            self.filter_hr(f_hr)
            self.filter_lr(f_lr)
        return True

    def encode_image(self, image):
        """super_res -> filter_hr -> filter_lr of ONE view without touching the model's state: returns the two feature maps
        (Img feat_lr, Img feat_hr) the query kernels read.  gen_mesh_pipelined runs it for the next subject on a second
        stream while the current subject's features are still in use."""
        W = self._encoder_weights()
        # (the graphed forms run eagerly off the device's default stream: gen_mesh_pipelined's second encoder keeps its own buffers)
        _, f_lr, f_hr = encoder.super_res_g(W, _as_img(image[0:1]), want_image=False)
        return encoder.filter_lr_g(W, f_lr)[-1], encoder.filter_hr(W, f_hr)[0]

    def features(self, b=0):
        """(Img feat_lr, Img feat_hr) of image b of the encoded batch, last stack: what the query kernels read."""
        if not self.im_feat_list_lr or not self.im_feat_list_hr:
            raise RuntimeError("filter_lr / filter_hr must run before a query")
        if b >= self.im_feat_list_lr[-1].shape[0] or b >= self.im_feat_list_hr[0].shape[0]:
            raise RuntimeError("the encoder ran on %d images, the query asks for image %d" % (self.im_feat_list_lr[-1].shape[0], b))
        # (feature maps assigned by hand as NCHW tensors are converted once, not once per query: the reference's loop asks 2 684
        #  times per 512^3 grid; the encoder's own outputs are NHWC views and cost nothing either way)
        # The cache entry HOLDS the two source tensors and a hit requires them to be the same objects (`is`, as _calib_rows does): a
        # freed tensor's address and version cannot come back under another tensor while the entry keeps it alive.  Only device
        # tensors are cached - a CPU tensor made by torch.from_numpy can be edited through the numpy array without its version
        # counter moving -; an in-place edit of a cached DEVICE tensor through `.data` is the one case no counter sees:
        # invalidate_feature_cache() is for that.
        tl, th = self.im_feat_list_lr[-1], self.im_feat_list_hr[0]
        cacheable = tl.is_cuda and th.is_cuda and not tl.is_inference() and not th.is_inference()
        key = (b, tl.data_ptr(), th.data_ptr(), tuple(tl.shape), tuple(th.shape), tl.stride(), th.stride(),
               tl._version if cacheable else None, th._version if cacheable else None)
        hit = self._feat_cache
        if cacheable and hit is not None and hit[0] == key and hit[1] is tl and hit[2] is th:
            return hit[3]
        out = _as_img(tl[b:b + 1]), _as_img(th[b:b + 1])
        self._feat_cache = (key, tl, th, out) if cacheable else None
        return out

    def stack_features(self, b=0):
        """([Img feat_lr of every kept stack], Img feat_hr) of image b of the encoded batch: what the stacks entries read - one pass per
        entry of im_feat_list_lr, every pass on im_feat_list_hr[0] (SuRSNet.py:149-157, 175-185).  One map: features(b).  Cached as
        features() caches, on the identity and version of every map."""
        if len(self.im_feat_list_lr) <= 1:
            fl, fh = self.features(b)
            return [fl], fh
        if not self.im_feat_list_hr:
            raise RuntimeError("filter_lr / filter_hr must run before a query")
        tls, th = list(self.im_feat_list_lr), self.im_feat_list_hr[0]
        if any(b >= t.shape[0] for t in tls) or b >= th.shape[0]:
            raise RuntimeError("the encoder ran on %d images, the query asks for image %d" % (tls[-1].shape[0], b))
        ts = tls + [th]
        cacheable = all(t.is_cuda and not t.is_inference() for t in ts)
        key = (b,) + tuple((t.data_ptr(), tuple(t.shape), t.stride(), t._version if cacheable else None) for t in ts)
        hit = self._stack_feat_cache
        if cacheable and hit is not None and hit[0] == key and len(hit[1]) == len(ts) and all(x is y for x, y in zip(hit[1], ts)):
            return hit[2]
        out = [_as_img(t[b:b + 1]) for t in tls], _as_img(th[b:b + 1])
        self._stack_feat_cache = (key, ts, out) if cacheable else None
        return out

    def views_features(self):
        """(feat_lr [V,hl,wl,hg_dim], feat_hr [V,hh,wh,64]) contiguous NHWC device tensors of every view: what the multi-view evaluator of
        classifiers of any shape reads.  Cached as features() caches (same key rules, invalidate_feature_cache): the octree walk and
        the reference's sweep loop ask for them once per batch."""
        if not self.im_feat_list_lr or not self.im_feat_list_hr:
            raise RuntimeError("filter_lr / filter_hr must run before a query")
        tl, th = self.im_feat_list_lr[-1], self.im_feat_list_hr[0]
        if tl.shape[0] != self.num_views or th.shape[0] != self.num_views:
            raise RuntimeError("the encoder ran on %d views, num_views is %d" % (tl.shape[0], self.num_views))
        cacheable = tl.is_cuda and th.is_cuda and not tl.is_inference() and not th.is_inference()
        key = (tl.data_ptr(), th.data_ptr(), tuple(tl.shape), tuple(th.shape), tl.stride(), th.stride(),
               tl._version if cacheable else None, th._version if cacheable else None)
        hit = getattr(self, "_views_feat_cache", None)
        if cacheable and hit is not None and hit[0] == key and hit[1] is tl and hit[2] is th:
            return hit[3]
        dev = self._device()
        out = tl.to(dev, torch.float32).permute(0, 2, 3, 1).contiguous(), th.to(dev, torch.float32).permute(0, 2, 3, 1).contiguous()
        self._views_feat_cache = (key, tl, th, out) if cacheable else None
        return out

    def _views_calibs(self, rows, dev):
        """Host calibration rows [V,12] (_calib_rows' cached array) as a device tensor, copied once per rows array; one row serves
        every view (gen_mesh's single diag(2, -2, 2, 1) calibration)."""
        hit = getattr(self, "_views_cal_cache", None)
        if hit is not None and hit[0] is rows:
            return hit[1]
        cal = np.ascontiguousarray(rows, np.float32)
        cal = torch.from_numpy(np.repeat(cal, self.num_views, 0) if cal.shape[0] == 1 else cal).to(dev)
        self._views_cal_cache = (rows, cal)
        return cal

    def invalidate_feature_cache(self):
        """Forget the converted copy of hand-assigned feature maps (see features(): needed only after an edit no version counter sees)."""
        self._feat_cache = None
        self._views_feat_cache = None
        self._stack_feat_cache = None

    # ------------------------------------------------------------------ query
    def _zscale(self):
        return float(self.opt.loadSize // 2), float(self.opt.z_size)

    def _calib_rows(self, calibs, transforms):
        """calibs [B,4,4] -> host rows [B,12] of [R|t], with the image-space `transforms` [B,2,3] (or one [2,3] for every image)
        folded in.  lib/geometry.py:27-30 / 43-46 apply xy' = S xy + s after the projection; both compose into the first two rows
        of the calibration: orthogonal  rows01' = S rows01, t01' = S t01 + s;  perspective (xy = h01 / h2)  rows01' = S rows01 +
        s (x) row2, so that h01' / h2 = S xy + s.  (The reference slices `transforms[:2, :2]` - of a [B,2,3] tensor that is not
        the 2x2 scale its baddbmm needs, and of a [2,3] matrix baddbmm refuses the rank -, so this follows the evident meaning,
        which is PIFu's `transforms[:, :2, :2]`; the eval path never passes transforms.)"""
        # (the reference's sweep loop passes the same device tensors 2 684 times per 512^3 grid: a device-to-host copy - a host
        #  synchronisation - per call is what the loop then spends its time in; cached on the tensors' identity and version)
        # Limits of that key: a write through `.data` or through a numpy alias of a CPU tensor does not bump the version - callers that
        # edit calibrations that way pass a new tensor or call invalidate_calib_cache(); inference-mode tensors have no version counter
        # (reading it raises): they are converted on every call.
        try:
            key = (calibs.data_ptr(), calibs._version, tuple(calibs.shape),
                   None if transforms is None else (transforms.data_ptr(), transforms._version), self.projection_mode)
        except RuntimeError:
            return self._calib_rows_uncached(calibs, transforms)
        hit = getattr(self, "_calib_cache", None)
        if hit is not None and hit[0] == key and hit[1] is calibs and hit[2] is transforms:
            return hit[3]
        rows = self._calib_rows_uncached(calibs, transforms)
        self._calib_cache = (key, calibs, transforms, rows)
        return rows

    def invalidate_calib_cache(self):
        """Forget the cached host copy of the last calibration (see _calib_rows: needed only after an edit that no version counter sees)."""
        self._calib_cache = None

    def _calib_rows_uncached(self, calibs, transforms):
        cal = calibs.detach().to("cpu", torch.float64).numpy()[:, :3, :].copy()
        if transforms is not None:
            tr = transforms.detach().to("cpu", torch.float64).numpy()
            if tr.ndim == 2:
                tr = np.broadcast_to(tr, (cal.shape[0],) + tr.shape)
            if tr.shape[0] != cal.shape[0] or tr.shape[1] < 2 or tr.shape[2] < 3:
                raise ValueError("transforms must be [B,2,3] (scale | shift) for calibs [B,4,4]")
            for b in range(cal.shape[0]):
                S, sh = tr[b, :2, :2], tr[b, :2, 2]
                top = S @ cal[b, :2, :]
                if self.projection_mode == "orthogonal":
                    top[:, 3] += sh
                else:
                    top += np.outer(sh, cal[b, 2, :])
                cal[b, :2, :] = top
        return cal.reshape(cal.shape[0], 12).astype(np.float32)

    def _query(self, points, calibs, transforms, p_lr=None):
        """Both classifiers on `points` (p_lr None), or the hr classifier alone with the lr occupancies p_lr [B,1,N] given."""
        dev = self._device()
        zmul, zdiv = self._zscale()
        V = self.num_views
        g = self.generic_mlp()
        if g is not None and self.projection_mode != "orthogonal":
            raise NotImplementedError("classifiers of a shape other than the released one: orthogonal models only")
        if g is not None and V > 1:
            # one subject seen by V views (SurfaceClassifier.py:70-76): the fused multi-view evaluator, one launch per call
            if points.shape[0] != V or calibs.shape[0] not in (1, V):
                raise NotImplementedError("one subject per call: points must be [num_views,3,N] and calibs [num_views,4,4] (or one "
                                          "[1,4,4] for every view)")
            pts = points.to(dev, torch.float32).contiguous()
            cal = self._views_calibs(self._calib_rows(calibs, transforms), dev)
            pl = None if p_lr is None else p_lr.to(dev, torch.float32).reshape(V, -1).contiguous()
            run = lambda: native.query_points_generic_views(pts, cal, zmul, zdiv, *self.views_features(), g, p_lr=pl)
            with native.reduced_point_operands(self.precision in ("bf16", "fp16")):
                first = run()
            phr, plr = self._finite_or_wide(run, first=first)
            return phr.view(V, 1, -1), plr.view(V, 1, -1)
        if g is not None:
            # the fused evaluator, one launch per image of the batch; --precision bf16 | fp16: one f16 product per MAC
            B = points.shape[0]
            if calibs.shape[0] != B:
                raise ValueError("points [%d,3,N] and calibs [%d,4,4] disagree" % (B, calibs.shape[0]))
            cal = self._calib_rows(calibs, transforms)
            outs = []
            for b in range(B):
                pts = points[b].to(dev, torch.float32).contiguous()
                pl = None if p_lr is None else p_lr[b].to(dev, torch.float32).reshape(-1).contiguous()
                run = lambda: native.query_points_generic(pts, cal[b], zmul, zdiv, *self.features(b), g, p_lr=pl)
                with native.reduced_point_operands(self.precision in ("bf16", "fp16")):
                    first = run()
                outs.append(self._finite_or_wide(run, b, first=first))
            if B == 1:
                return outs[0][0].view(1, 1, -1), outs[0][1].view(1, 1, -1)
            return torch.stack([o[0] for o in outs]).view(B, 1, -1), torch.stack([o[1] for o in outs]).view(B, 1, -1)
        if V == 1 and self.projection_mode == "orthogonal":
            # a batch of B subjects (one image each): image b's features serve points[b] (geometry.index pairs them the same way)
            B = points.shape[0]
            if calibs.shape[0] != B:
                raise ValueError("points [%d,3,N] and calibs [%d,4,4] disagree" % (B, calibs.shape[0]))
            cal = self._calib_rows(calibs, transforms)
            outs = []
            for b in range(B):
                pts = points[b].to(dev, torch.float32).contiguous()
                if p_lr is None:
                    run = lambda: native.query_points(pts, cal[b], zmul, zdiv, *self.features(b), self._mlp_blob(), self._workspace())
                else:
                    pl = p_lr[b].to(dev, torch.float32).reshape(-1).contiguous()
                    run = lambda: (native.query_points_hr(pts, cal[b], zmul, zdiv, *self.features(b), self._mlp_blob(),
                                                          self._workspace(), pl), pl)
                # --precision bf16 | fp16: the points go through the one-product f16 layer kernels (the reference's MLP in half
                # precision); non-finite results are repeated fp32-grade on three bf16 parts like every other overflow
                # points that come as runs of equal (x, y) - the reference's sweep loop: consecutive grid points, z fastest - are
                # columns: the restated column kernels take them (same arithmetic as reconstruction()'s sweep in this precision)
                # (which evaluator an array gets is a function of the array alone: the run finder looks at every array - ~ 0.1 ms for
                #  nothing on random samples, 1.1 -> 1.2 ms per 50 000 points - instead of backing off after refusals, which made the
                #  same points' last bits depend on the calls before them)
                first = None
                if p_lr is None:
                    first = native.query_points_columns(pts, cal[b], zmul, zdiv, *self.features(b), self._mlp_blob(), self.precision,
                                                        self._workspace())
                if first is None:
                    with native.reduced_point_operands(self.precision in ("bf16", "fp16")):
                        first = run()
                outs.append(self._finite_or_wide(run, b, first=first))
            if B == 1:   # (no copy: the reference's sweep loop comes through here 2 684 times per 512^3 grid)
                return outs[0][0].view(1, 1, -1), outs[0][1].view(1, 1, -1)
            phr = torch.stack([o[0] for o in outs]).view(B, 1, -1)
            plr = torch.stack([o[1] for o in outs]).view(B, 1, -1)
            return phr, plr
        if p_lr is not None:
            raise NotImplementedError("query_sr on points other than the preceding query_mr's: single-view orthogonal models only")
        # multi-view and / or perspective: the view mean of SurfaceClassifier.py:70-76 needs every view of the one subject
        # in the call: points [V,3,N] as reshape_sample_tensor (train_util.py:40-51) lays them out, calibs [V,4,4]
        if points.shape[0] != V or calibs.shape[0] != V:
            raise NotImplementedError("one subject per call: points must be [num_views,3,N] and calibs [num_views,4,4]")
        if not self.im_feat_list_lr or not self.im_feat_list_hr:
            raise RuntimeError("filter_lr / filter_hr must run before a query")
        fl = self.im_feat_list_lr[-1].to(dev).permute(0, 2, 3, 1).contiguous()
        fh = self.im_feat_list_hr[0].to(dev).permute(0, 2, 3, 1).contiguous()
        if fl.shape[0] != V or fh.shape[0] != V:
            raise RuntimeError("the encoder ran on %d views, num_views is %d" % (fl.shape[0], V))
        pts = points.to(dev, torch.float32).contiguous()
        cal = self._calib_rows(calibs, transforms)
        def run():
            fl = self.im_feat_list_lr[-1].to(dev).permute(0, 2, 3, 1).contiguous()
            fh = self.im_feat_list_hr[0].to(dev).permute(0, 2, 3, 1).contiguous()
            return native.query_points_views(pts, cal, self.projection_mode, zmul, zdiv, fl, fh, self._mlp_blob(), self._workspace())
        phr, plr = self._finite_or_wide(run)
        return phr.view(V, 1, -1), plr.view(V, 1, -1)

    def _finite_or_wide(self, run, b=0, first=None):
        """run() -> (pred_hr, pred_lr).  The fp32 point kernels carry their operands as two f16 parts (|x| < 65504); the reference
        is plain fp32.  Non-finite predictions (the callers copy them to the host next, so the check costs no extra
        synchronisation) are computed again on three bf16 parts - fp32's exponent range -, after re-running the encoder the same
        way if its features are what overflowed."""
        phr, plr = run() if first is None else first
        # (one small launch and a 4-byte read-back: surs_nonfinite; until round 6 two torch reductions and an addition)
        if phr is None:   # (the lr-only pass of the stacks route)
            finite = not native.any_nonfinite(plr)
        elif phr.numel() == plr.numel() and phr.dtype == plr.dtype == torch.float32 and phr.is_cuda:
            finite = not native.any_nonfinite(phr, plr)
        else:
            finite = math.isfinite((phr.sum() + plr.sum()).item())
        if finite:
            return phr, plr
        import warnings
        warnings.warn("query: non-finite predictions from the two-part f16 operand split; repeating on three bf16 parts", stacklevel=3)
        with native.wide_operands():
            fl, fh = self.features(b) if self.num_views == 1 else (self.im_feat_list_lr[-1], self.im_feat_list_hr[0])
            feats_ok = bool(torch.isfinite(fl.buf if hasattr(fl, "buf") else fl).all()) and bool(torch.isfinite(fh.buf if hasattr(fh, "buf") else fh).all())
            if feats_ok and self.num_views == 1 and len(self.im_feat_list_lr) > 1:   # (the stacks route read every kept map)
                feats_ok = all(bool(torch.isfinite(f.buf).all()) for f in self.stack_features(b)[0][:-1])
            if not feats_ok and not self.reencode_wide():
                raise native._lib.NonFiniteVolumeError("the feature maps hold non-finite values and the images they were encoded "
                                                       "from are not known to this object (set by hand or by another call chain)")
            return run()

    _STACKS_LIMIT = ("every kept hourglass stack (len(im_feat_list_lr) > 1, i.e. features filtered in training mode) and forward(): "
                     "num_views == 1 and orthogonal projection only")

    def _query_stacks(self, points, calibs, transforms, p_lr=None, lr_only=False):
        """One pass per entry of im_feat_list_lr (SuRSNet.py:149-157, 175-185), each on im_feat_list_hr[0]: both classifiers, the hr
        classifier alone fed stack by stack with p_lr (a list of S tensors [B,1,N]), or the lr classifier alone (lr_only).  One
        library call per image for all stacks.  Returns (list of S pred_hr [B,1,N] - None with lr_only -, list of S pred_lr)."""
        if self.num_views != 1 or self.projection_mode != "orthogonal":
            raise NotImplementedError(self._STACKS_LIMIT)
        dev = self._device()
        zmul, zdiv = self._zscale()
        g = self.generic_mlp()
        S, B = len(self.im_feat_list_lr), points.shape[0]
        if S == 0 or not self.im_feat_list_hr:
            raise RuntimeError("filter_lr / filter_hr must run before a query")
        if calibs.shape[0] != B:
            raise ValueError("points [%d,3,N] and calibs [%d,4,4] disagree" % (B, calibs.shape[0]))
        if p_lr is not None and len(p_lr) < S:
            raise ValueError("query_sr: %d feature maps against the lr predictions of %d stacks (SuRSNet.py:180 indexes them by stack)"
                             % (S, len(p_lr)))
        cal = self._calib_rows(calibs, transforms)
        outs = []
        for b in range(B):
            pts = points[b].to(dev, torch.float32).contiguous()
            pl = None if p_lr is None else torch.stack([p[b].to(dev, torch.float32).reshape(-1) for p in p_lr[:S]])
            if g is not None:
                run = lambda: native.query_points_generic_stacks(pts, cal[b], zmul, zdiv, *self.stack_features(b), g, p_lr=pl,
                                                                 lr_only=lr_only)
            else:
                # (the layer kernels whatever the point order: the column kernels of the single-map route have no per-stack form)
                run = lambda: native.query_points_stacks(pts, cal[b], zmul, zdiv, *self.stack_features(b), self._mlp_blob(),
                                                         self._workspace(), p_lr=pl, lr_only=lr_only)
            # --precision bf16 | fp16: one f16 product per MAC, as the single-map query of that precision
            with native.reduced_point_operands(self.precision in ("bf16", "fp16")):
                first = run()
            outs.append(self._finite_or_wide(run, b, first=first))

        def per_stack(i):
            if outs[0][i] is None:
                return None
            if B == 1:
                return [outs[0][i][s].view(1, 1, -1) for s in range(S)]
            return [torch.stack([o[i][s] for o in outs]).view(B, 1, -1) for s in range(S)]
        return per_stack(0), per_stack(1)

    def query_mr(self, points, calibs, transforms=None, labels=None):
        """Evaluates both classifiers in one fused pass, once per entry of im_feat_list_lr (SuRSNet.py:131-159); the hr predictions
        are kept for the following query_sr.  labels: stored as labels_lr (what get_error_lr holds the lr predictions against)."""
        self._query_mr(points, calibs, transforms, labels, lr_only=False)

    def _query_mr(self, points, calibs, transforms, labels, lr_only):
        if labels is not None:
            self.labels_lr = labels
        if len(self.im_feat_list_lr) > 1 or lr_only:
            phr, plr = self._query_stacks(points, calibs, transforms, lr_only=lr_only)
        else:
            phr, plr = self._query(points, calibs, transforms)
            phr, plr = [phr], [plr]
        self._mr_points, self._mr_hr, self._mr_version = points, phr, points._version
        self._mr_args = (calibs, transforms)
        self.intermediate_preds_list_lr = plr
        self.preds_lr = plr[-1]

    def query_sr(self, points, calibs, transforms=None, labels=None):
        """SuRSNet.py:161-187.  With the points (and calibs / transforms) of the preceding query_mr - the reference's eval_func and
        gen_mesh - the fused pass has already produced preds_hr.  Any other point set of the same N goes through the hr classifier
        alone, fed with query_mr's lr predictions index by index (and stack by stack), exactly as the reference concatenates them.
        labels: stored as labels_hr."""
        if labels is not None:
            self.labels_hr = labels
        if self._mr_points is None:
            raise RuntimeError("query_sr needs the preceding query_mr (it consumes its lr predictions, SuRSNet.py:179)")
        self._sr_points, self._sr_args = points, (calibs, transforms)
        # the same points as the preceding query_mr?  Decided without touching the data (a full-tensor compare is a device
        # synchronisation per call): the same tensor object, or the same storage / view / version
        ref, ver = self._mr_points, self._mr_version
        have = self._mr_hr is not None and len(self._mr_hr) == len(self.im_feat_list_lr)   # (not after forward()'s lr-only pass)
        same = have and ((points is ref and points._version == ver) or (
            points.data_ptr() == ref.data_ptr() and points.shape == ref.shape and points.stride() == ref.stride()
            and points.dtype == ref.dtype and points._version == ver and ref._version == ver))
        if have and not same and points is not ref and ref._version == ver:
            # another tensor: the fused result stands if it holds the same values (this comparison synchronises; callers that
            # pass the tensor they gave query_mr never get here)
            same = points.shape == ref.shape and bool(torch.equal(points.to(ref.device), ref))
        c0, t0 = self._mr_args
        same = same and (calibs is c0 or (calibs.shape == c0.shape and bool(torch.equal(calibs.cpu(), c0.cpu()))))
        same = same and ((transforms is None and t0 is None) or (transforms is not None and t0 is not None
                                                                 and transforms.shape == t0.shape
                                                                 and bool(torch.equal(transforms.cpu(), t0.cpu()))))
        if same:
            phr = self._mr_hr
        else:
            if points.shape[-1] != self.preds_lr.shape[-1] or points.shape[0] != self.preds_lr.shape[0]:
                raise ValueError("query_sr: %s points against lr predictions %s (SuRSNet.py:179 concatenates them channel-wise)"
                                 % (tuple(points.shape), tuple(self.preds_lr.shape)))
            if len(self.im_feat_list_lr) > 1:
                phr, _ = self._query_stacks(points, calibs, transforms, p_lr=self.intermediate_preds_list_lr)
            else:
                phr, _ = self._query(points, calibs, transforms, p_lr=self.intermediate_preds_list_lr[0])
                phr = [phr]
        self.intermediate_preds_list_hr = phr
        self.preds_hr = phr[-1]

    def get_preds(self):
        return self.preds_hr, self.preds_lr

    # ------------------------------------------------------------------ the validation forward: losses
    def _stacked(self, preds):
        """[S,M] device tensor of a list of S predictions [B,1,N] (M = B N)."""
        dev = self._device()
        return torch.stack([p.to(dev, torch.float32).reshape(-1) for p in preds])

    def _labels(self, which):
        lab = self.labels_lr if which == "lr" else self.labels_hr
        if lab is None:
            raise RuntimeError("labels_%s is not set: pass labels= to query_%s (SuRSNet.py:134-136, 164-165)"
                               % (which, "mr" if which == "lr" else "sr"))
        return lab.to(self._device(), torch.float32).reshape(-1).contiguous()

    def get_error_lr(self):
        """SuRSNet.py:196-204: the mean over stacks of MSE(intermediate_preds_list_lr[s], labels_lr); 0-dim float32 device tensor."""
        if not self.intermediate_preds_list_lr:
            raise RuntimeError("get_error_lr needs a preceding query_mr")
        return native.forward_losses(pred_lr=self._stacked(self.intermediate_preds_list_lr), lab_lr=self._labels("lr"))[0][0]

    def get_error_hr(self):
        """SuRSNet.py:206-214: the same of intermediate_preds_list_hr and labels_hr."""
        if not self.intermediate_preds_list_hr:
            raise RuntimeError("get_error_hr needs a preceding query_sr")
        return native.forward_losses(pred_hr=self._stacked(self.intermediate_preds_list_hr), lab_hr=self._labels("hr"))[0][1]

    def get_errorSR(self, image_SR, images_hr):
        """SuRSNet.py:216-226: the L1 mean of image_SR - images_hr (nn.L1Loss)."""
        self.images_HR = images_hr
        dev = self._device()
        if tuple(image_SR.shape) != tuple(images_hr.shape):
            raise ValueError("get_errorSR: image_SR %s against images_hr %s" % (tuple(image_SR.shape), tuple(images_hr.shape)))
        return native.forward_losses(img_sr=image_SR.to(dev, torch.float32), img_hr=images_hr.to(dev, torch.float32))[0][2]

    def get_error_disp_1(self):
        """SuRSNet.py:228-236: MSE(labels_hr - labels_lr, preds_hr - preds_lr), the last stack's predictions."""
        if not self.intermediate_preds_list_lr or not self.intermediate_preds_list_hr:
            raise RuntimeError("get_error_disp_1 needs a preceding query_mr and query_sr")
        return native.forward_losses(pred_lr=self._stacked(self.intermediate_preds_list_lr[-1:]), lab_lr=self._labels("lr"),
                                     pred_hr=self._stacked(self.intermediate_preds_list_hr[-1:]), lab_hr=self._labels("hr"))[0][3]

    def loss_terms(self, image_SR, images_hr):
        """(terms, total): the four terms above as one [4] float32 device tensor - get_error_lr, get_error_hr, get_errorSR,
        get_error_disp_1 - and their sum weighted with opt.mlp1, opt.mlp2, opt.srweight, opt.dispweight (SuRSNet.py:265), from ONE
        deterministic reduction (surs_forward_losses) and without a host synchronisation."""
        dev = self._device()
        if not self.intermediate_preds_list_lr or len(self.intermediate_preds_list_lr) != len(self.intermediate_preds_list_hr):
            raise RuntimeError("loss_terms needs a preceding query_mr and query_sr on the same feature maps")
        if tuple(image_SR.shape) != tuple(images_hr.shape):
            raise ValueError("get_errorSR: image_SR %s against images_hr %s" % (tuple(image_SR.shape), tuple(images_hr.shape)))
        self.images_HR = images_hr
        w = (self.opt.mlp1, self.opt.mlp2, self.opt.srweight, self.opt.dispweight)
        return native.forward_losses(pred_lr=self._stacked(self.intermediate_preds_list_lr), lab_lr=self._labels("lr"),
                                     pred_hr=self._stacked(self.intermediate_preds_list_hr), lab_hr=self._labels("hr"),
                                     img_sr=image_SR.to(dev, torch.float32), img_hr=images_hr.to(dev, torch.float32), weights=w)

    def forward(self, images_lr, images_hr, points_lr, points_hr, calibs, transforms=None, labels_lr=None, labels_hr=None):
        """The reference's forward (SuRSNet.py:240-266) as a VALIDATION forward: (res_hr, error, res_lr) computed on the device
        without an autograd graph - error is a 0-dim float32 device tensor with no grad_fn; error.backward() fails with torch's own
        message.  super_res -> filter_lr -> filter_hr -> query_mr(points_hr, labels=labels_hr) -> query_sr(points_lr,
        labels=labels_lr) - the reference's own crossing of the two label arguments, kept -, then opt.mlp1 get_error_lr() + opt.mlp2
        get_error_hr() + opt.srweight get_errorSR(img_SR, images_hr) + opt.dispweight get_error_disp_1().  In training mode every
        kept stack is evaluated (intermediate_preds_list_lr / _hr: one [B,1,N] entry per stack), in eval mode the last one.
        --norm batch normalises with the running statistics in EITHER mode, as every other call of this package does: train() keeps
        the stacks, it never switches to batch statistics and updates nothing.  num_views == 1 and orthogonal projection only.
        images_lr [B,3,H,W], images_hr [B,3,sH,sW], points_* [B,3,N], calibs [B,4,4], labels_* [B,1,N]."""
        if self.num_views != 1 or self.projection_mode != "orthogonal":
            raise NotImplementedError(self._STACKS_LIMIT)
        if labels_lr is None or labels_hr is None:
            raise ValueError("forward needs labels_lr and labels_hr (the loss terms are taken against them)")
        img_SR, feature_lr, feature_hr = self.super_res(images_lr)
        self.filter_lr(feature_lr)
        self.filter_hr(feature_hr)
        # query_sr runs on other points than query_mr: nothing reads the hr classifier on points_hr - an lr-only pass, then an hr-only one
        self._query_mr(points_hr, calibs, transforms, labels_hr, lr_only=True)
        self.query_sr(points_lr, calibs, transforms=transforms, labels=labels_lr)
        res_hr, res_lr = self.get_preds()
        self.loss_values, error = self.loss_terms(img_SR, images_hr)
        return res_hr, error, res_lr

    # ------------------------------------------------------------------ classifier gradients
    _GRADS_LIMIT = ("classifier gradients (forward_backward(), classifier_grads()): num_views == 1 and orthogonal projection only")

    def _mlp_params(self):
        return self._param_set("mlp")[0]

    def classifier_grads(self, features=False):
        """d error / d (every mlp_lr.* and mlp_hr.* parameter) of forward()'s loss - opt.mlp1 get_error_lr() + opt.mlp2 get_error_hr()
        + opt.dispweight get_error_disp_1(); the super-resolution term does not depend on these parameters - from what the preceding
        query_mr(labels=...) + query_sr(labels=...) left on this object: their points, calibrations, transforms and labels, the
        feature maps of im_feat_list_lr (every kept stack in training mode, the last one in eval mode) and im_feat_list_hr[0].
        Returns an OrderedDict in state_dict() key order holding every mlp_* key: float32 device tensors of the parameters' shapes
        ([out,in,1] weights), summed over stacks and over the images of the batch.  The encoder is frozen: mlp_lr's gradient
        has its three sources (its own term, the displacement term, mlp_hr's last input channel), and there are no gradients for the
        encoder / super-resolution parameters (out of scope).  features=True returns (grads, feat_grads): the same grads, bit for
        bit, and d error / d (the feature maps) - feat_grads["lr"]: a list with one float32 device tensor per entry of
        im_feat_list_lr, each of that entry's shape [B,D,hl,wl]; feat_grads["hr"]: of im_feat_list_hr[0]'s shape [B,64,hh,wh] -,
        what an encoder's backward starts from (autograd.point_loss hands them to torch autograd).  An image whose points all fall
        outside gets exact zeros.  fp32-grade whatever --precision says, deterministic (two calls give the same bits).  num_views
        == 1 and orthogonal projection only."""
        if self.num_views != 1 or self.projection_mode != "orthogonal":
            raise NotImplementedError(self._GRADS_LIMIT)
        if self._mr_points is None:
            raise RuntimeError("classifier_grads needs a preceding query_mr(labels=...): its points are not known")
        if self._sr_points is None:
            raise RuntimeError("classifier_grads needs a preceding query_sr(labels=...): its points are not known")
        if self.labels_lr is None:
            raise RuntimeError("classifier_grads: labels_lr is not set: pass labels= to query_mr (SuRSNet.py:134-136)")
        if self.labels_hr is None:
            raise RuntimeError("classifier_grads: labels_hr is not set: pass labels= to query_sr (SuRSNet.py:164-165)")
        dev = self._device()
        pm, ps = self._mr_points, self._sr_points
        if tuple(pm.shape) != tuple(ps.shape):
            raise ValueError("classifier_grads: query_mr's points %s against query_sr's %s (SuRSNet.py:179 pairs them index by index)"
                             % (tuple(pm.shape), tuple(ps.shape)))
        B, N = pm.shape[0], pm.shape[2]
        lab = [l.to(dev, torch.float32).reshape(B, -1) for l in (self.labels_lr, self.labels_hr)]
        if any(l.shape[1] != N for l in lab):
            raise ValueError("classifier_grads: labels %s / %s against %d points per image"
                             % (tuple(self.labels_lr.shape), tuple(self.labels_hr.shape), N))
        if not self.im_feat_list_lr or not self.im_feat_list_hr:
            raise RuntimeError("filter_lr / filter_hr must run before a query")
        cal_mr, cal_sr = self._calib_rows(*self._mr_args), self._calib_rows(*self._sr_args)
        if cal_mr.shape[0] != B or cal_sr.shape[0] != B:
            raise ValueError("points [%d,3,N] and calibs [%d,4,4] / [%d,4,4] disagree" % (B, cal_mr.shape[0], cal_sr.shape[0]))
        zmul, zdiv = self._zscale()
        params = self._mlp_params()
        need = (native.mlp_grad_features_workspace_bytes if features else native.mlp_grad_workspace_bytes)(params.shapes)
        if self._grad_ws is None or self._grad_ws[0] != params.shapes or self._grad_ws[1].numel() * 4 < need:
            self._grad_ws = (params.shapes, torch.empty(need // 4, dtype=torch.float32, device=dev))
        w = (self.opt.mlp1, self.opt.mlp2, self.opt.dispweight)
        grads = None
        if features:
            # NCHW-shaped like the model's maps, NHWC in memory: image b of each is the contiguous [h,w,C] block the library writes
            like = lambda t: torch.empty((t.shape[0], t.shape[2], t.shape[3], t.shape[1]), dtype=torch.float32, device=dev)
            g_lr, g_hr = [like(t) for t in self.im_feat_list_lr], like(self.im_feat_list_hr[0])
        for b in range(B):
            feats, fh = self.stack_features(b)
            fg = native.FeatGrads([t[b] for t in g_lr], g_hr[b]) if features else None
            out = native.mlp_grads(pm[b].to(dev, torch.float32).contiguous(), ps[b].to(dev, torch.float32).contiguous(), cal_mr[b],
                                   cal_sr[b], zmul, zdiv, feats, fh, params, lab[0][b], lab[1][b], w, B * N, grads=grads,
                                   accumulate=b > 0, workspace=self._grad_ws[1], feat_grads=fg)
            grads = out[0] if features else out
        if features:
            return grads, dict(lr=[t.permute(0, 3, 1, 2) for t in g_lr], hr=g_hr.permute(0, 3, 1, 2))
        return grads

    def forward_backward(self, images_lr, images_hr, points_lr, points_hr, calibs, transforms=None, labels_lr=None, labels_hr=None,
                         features=False, encoder=False):
        """forward() and the gradients of its loss: (res_hr, error, res_lr, grads).

        encoder=False (the default): the first three are exactly forward()'s (it is called; error still has no autograd graph), grads
        is classifier_grads()'s OrderedDict: every mlp_lr.* / mlp_hr.* key in state_dict() order, float32 device tensors of the
        parameters' shapes.  features=True: (res_hr, error, res_lr, grads, feat_grads) with classifier_grads(features=True)'s
        feat_grads and feat_grads["img_SR"] = opt.srweight sign(img_SR - images_hr) / numel (torch's L1 backward, 0 at equality) -
        everything the loss hands back to the encoder.

        encoder=True: the FULL gradient, what one iteration of the reference's training loop computes (apps/train_SuRS.py:122-148).
        grads is one OrderedDict over every key of mlp_parameters(), sr_parameters() and hg_parameters(), in state_dict() order:
        float32 device tensors of the parameters' shapes, summed over the batch in image order, the same bits on every call - what
        optim.Optimizer.step() takes.  ONE taped forward, no second one: super_res_train(images_lr) -> filter_lr_train(feature_lr) ->
        the stacks queries, with the reference's crossing of the label arguments as forward() does them -> the loss with the gradient
        of its image term (surs_forward_losses_grad) -> classifier_grads(features=True) -> filter_lr_backward(d im_feat_list_lr) ->
        one super_res_backward(d img_SR, d feature_lr, d im_feat_list_hr[0]).  The gradients between these calls stay in the NHWC
        memory the library writes and reads: no clone and no layout change of a map.  res_hr, error, res_lr, loss_values, im_SR and
        im_feat_list_* are forward()'s bit for bit on the same input (the taped forwards run the inference launch lists; the loss keeps
        surs_forward_losses' partition); in eval mode only the last stack is queried, as forward() does, and the other stacks get zero
        gradients.  features does not apply (ValueError).  Non-finite FEATURES are not retried on wide operands here - the tapes would
        no longer be those of the features -: the query raises NonFiniteVolumeError; non-finite GRADIENTS are what
        Optimizer.step(guard=True) looks for.  Refused, by the checks of the calls above: --norm batch (NotImplementedError: no
        backward), --encoder_precision f16 (RuntimeError: net->parts == 1 has no backward).

        Either way: num_views == 1 and orthogonal projection only (NotImplementedError)."""
        if self.num_views != 1 or self.projection_mode != "orthogonal":
            raise NotImplementedError(self._GRADS_LIMIT)
        if encoder:
            if features:
                raise ValueError("forward_backward(encoder=True) returns the parameters' gradients; features=True goes with encoder=False")
            return self._forward_backward_full(images_lr, images_hr, points_lr, points_hr, calibs, transforms, labels_lr, labels_hr)
        res_hr, error, res_lr = self.forward(images_lr, images_hr, points_lr, points_hr, calibs, transforms=transforms,
                                             labels_lr=labels_lr, labels_hr=labels_hr)
        if not features:
            return res_hr, error, res_lr, self.classifier_grads()
        grads, feat_grads = self.classifier_grads(features=True)
        img_SR = self.im_SR.to(self._device(), torch.float32)
        # (an fp32 division, as the backward of torch's mean: the bits of opt.srweight * l1_loss(img_SR, images_hr).backward())
        scale = torch.full((), float(self.opt.srweight), dtype=torch.float32, device=img_SR.device) / img_SR.numel()
        feat_grads["img_SR"] = torch.sign(img_SR - images_hr.to(img_SR.device, torch.float32)) * scale
        return res_hr, error, res_lr, grads, feat_grads

    def _check_full_gradient(self):
        """forward_backward(encoder=True)'s refusals, before anything runs: the checks of the calls it is made of."""
        self._hg_check_norm()
        if getattr(self.opt, "encoder_precision", "auto") == "f16":
            raise RuntimeError(self._SR_F16)

    def _forward_backward_full(self, images_lr, images_hr, points_lr, points_hr, calibs, transforms, labels_lr, labels_hr):
        self._check_full_gradient()
        if labels_lr is None or labels_hr is None:
            raise ValueError("forward needs labels_lr and labels_hr (the loss terms are taken against them)")
        dev = self._device()
        img_SR, feature_lr, _ = self.super_res_train(images_lr)
        outs = self.filter_lr_train(feature_lr)
        S = len(outs)
        # (forward()'s filter_lr(keep_all=self.training): every stack in training mode, the last one in eval mode)
        self.im_feat_list_lr = list(outs) if self.training else outs[-1:]
        self._lr_from = None      # (reencode_wide must not replace these maps: the tapes are theirs)
        self._query_mr(points_hr, calibs, transforms, labels_hr, lr_only=True)
        self.query_sr(points_lr, calibs, transforms=transforms, labels=labels_lr)
        res_hr, res_lr = self.get_preds()
        if tuple(img_SR.shape) != tuple(images_hr.shape):
            raise ValueError("get_errorSR: image_SR %s against images_hr %s" % (tuple(img_SR.shape), tuple(images_hr.shape)))
        self.images_HR = images_hr
        w = (self.opt.mlp1, self.opt.mlp2, self.opt.srweight, self.opt.dispweight)
        def nhwc(t):
            """The [B,h,w,C] tensor behind an NCHW-shaped map of the library: a view, never a copy - the promise of this route."""
            t = t.permute(0, 2, 3, 1)
            assert t.is_contiguous(), "a map of the training step is not NHWC in memory: %s, strides %s" % (tuple(t.shape), t.stride())
            return t
        self.loss_values, error, d_img = native.forward_losses_grad(
            self._stacked(self.intermediate_preds_list_lr), self._labels("lr"), self._stacked(self.intermediate_preds_list_hr),
            self._labels("hr"), nhwc(img_SR), images_hr.detach().to(dev, torch.float32).contiguous(), w)
        g_mlp, fg = self.classifier_grads(features=True)
        g_lr = [None] * (S - len(fg["lr"])) + [nhwc(t) for t in fg["lr"]]
        d_feature_lr, g_hg = self._filter_lr_backward(g_lr, nhwc=True)
        g_sr = self._super_res_backward(d_img, d_feature_lr, nhwc(fg["hr"]), nhwc=True)
        merged = {}
        for g in (g_mlp, g_sr, g_hg):
            merged.update(g)
        grads = OrderedDict((k, merged[k]) for k in self._sd if k in merged)
        assert len(grads) == len(merged)
        return res_hr, error, res_lr, grads
