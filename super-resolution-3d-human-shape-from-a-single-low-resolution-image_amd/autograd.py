"""The point path as a torch.autograd.Function: gather, both classifiers on every kept stack and the three classifier terms of
SuRSNet.forward's loss, differentiable with respect to the feature maps.  An encoder that has a backward of its own - a torch encoder
under autograd - trains against this library's point evaluator through it.  super_res_features, conv_block and hourglass are the
Functions over the parts of the encoder that have a backward here; nothing else in the package grows an autograd graph."""
import torch

from . import native


class _PointLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, n_lr, points_mr, points_sr, calibs, labels_lr, labels_hr, transforms, *maps):
        feats = [m.detach() for m in maps]
        net.im_feat_list_lr, net.im_feat_list_hr = feats[:n_lr], [feats[n_lr]]
        net.query_mr(points_mr, calibs, transforms=transforms, labels=labels_lr)
        net.query_sr(points_sr, calibs, transforms=transforms, labels=labels_hr)
        w = (net.opt.mlp1, net.opt.mlp2, 0.0, net.opt.dispweight)
        _, total = native.forward_losses(pred_lr=net._stacked(net.intermediate_preds_list_lr), lab_lr=net._labels("lr"),
                                         pred_hr=net._stacked(net.intermediate_preds_list_hr), lab_hr=net._labels("hr"), weights=w)
        # the gradients are taken now: backward() may run after other queries have replaced what this one left on net
        grads, fg = net.classifier_grads(features=True)
        net.last_classifier_grads = grads
        ctx.n_fixed = 8
        ctx.save_for_backward(*(fg["lr"] + [fg["hr"]]))
        return total.clone()

    @staticmethod
    def backward(ctx, grad_output):
        return (None,) * ctx.n_fixed + tuple(grad_output * g for g in ctx.saved_tensors)


def point_loss(net, feat_lr_list, feat_hr, points_mr, points_sr, calibs, labels_lr, labels_hr, transforms=None):
    """opt.mlp1 get_error_lr() + opt.mlp2 get_error_hr() + opt.dispweight get_error_disp_1() of SuRSNet `net` on the feature maps
    feat_lr_list (a list of [B,D,hl,wl] tensors, one per kept stack) and feat_hr [B,64,hh,wh], as a 0-dim float32 device tensor
    with a grad_fn: its backward gives grad_output times d error / d (every map) - classifier_grads(features=True)'s tensors - to
    the maps that require grad.  The maps are assigned to net.im_feat_list_lr / im_feat_list_hr (detached), the points are evaluated
    as query_mr(points_mr, labels=labels_lr) and query_sr(points_sr, labels=labels_hr) do - forward() passes (points_hr, labels_hr)
    to the first and (points_lr, labels_lr) to the second -, and the classifiers' parameter gradients of the same loss are left in
    net.last_classifier_grads (not scaled by grad_output).  num_views == 1 and orthogonal projection only."""
    if net.num_views != 1 or net.projection_mode != "orthogonal":
        raise NotImplementedError(net._GRADS_LIMIT)
    feat_lr_list = list(feat_lr_list)
    return _PointLoss.apply(net, len(feat_lr_list), points_mr, points_sr, calibs, labels_lr, labels_hr, transforms, *feat_lr_list,
                            feat_hr)


class _SuperResFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, images_lr, *params):
        img_SR, feature_lr, _ = net.super_res_train(images_lr)
        ctx.net, ctx.tapes, ctx.n_params = net, net._sr_tapes, len(params)
        ctx.set_materialize_grads(False)   # an output nothing differentiates arrives as None, not as a map of zeros
        out = (img_SR, feature_lr, net.im_feat_list_hr[0])
        # (fresh tensors for autograd to own: the model keeps its NHWC views)
        return tuple(o.clone() for o in out)

    @staticmethod
    def backward(ctx, g_img, g_lr, g_hr):
        net = ctx.net
        if g_img is None and g_lr is None and g_hr is None:
            return (None,) * (2 + ctx.n_params)
        kept, net._sr_tapes = net._sr_tapes, ctx.tapes   # the tapes of THIS forward, whatever ran on the net since
        try:
            grads = net.super_res_backward(g_img, g_lr, g_hr)
        finally:
            net._sr_tapes = kept
        return (None, None) + tuple(grads.values())


def super_res_features(net, images_lr, params=None):
    """(img_SR, feature_lr, feat_hr) of SuRSNet `net` on images_lr [B,3,H,W] - super_res_train()'s values, feat_hr =
    im_feat_list_hr[0] -, each with a grad_fn: their backward is net.super_res_backward() with whatever gradients arrive (an output
    that receives none costs nothing) and hands every entry of `params` - default net.sr_parameters() - its gradient.  So
        img_SR, feature_lr, feat_hr = autograd.super_res_features(net, images_lr)
        loss = autograd.point_loss(net, torch_hg_filter(feature_lr), feat_hr, ...) + srweight * l1_loss(img_SR, images_hr)
        loss.backward()
    trains the super-resolution network on this package, the hourglass being a torch module with a backward of its own.
    The VALUES are those of the PACKED weights the forward runs on, not of `params`: after an optimiser step on sr_parameters(), call
    net.commit() before the next forward (as the examples of INTEGRATION.md do): it repacks them on the device from the parameters.
    Nothing else in the package grows a graph: forward()'s error.grad_fn stays None."""
    if params is None:
        params = net.sr_parameters()
    keys = list(net.sr_parameters())
    if list(params) != keys:
        raise ValueError("params must hold net.sr_parameters()'s keys in their order")
    return _SuperResFeatures.apply(net, images_lr, *params.values())


class _HgModule(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, which, keys, x, *params):
        hourglass = isinstance(which, int)
        out = net.hourglass_train(which, x) if hourglass else net.conv_block_train(which, x)
        key = which   # (an hourglass is filed under its stack, a block under its full prefix: net._hg_train)
        ctx.net, ctx.which, ctx.keys, ctx.key, ctx.tapes = net, which, keys, key, net._hg_tapes[key]
        return out.clone()   # (a fresh tensor for autograd to own)

    @staticmethod
    def backward(ctx, g):
        net = ctx.net
        kept = net._hg_tapes.get(ctx.key)
        net._hg_tapes[ctx.key] = ctx.tapes   # the tapes of THIS forward, whatever ran on the net since
        try:
            fn = net.hourglass_backward if isinstance(ctx.which, int) else net.conv_block_backward
            dx, grads = fn(ctx.which, g)
        finally:
            if kept is None:
                del net._hg_tapes[ctx.key]
            else:
                net._hg_tapes[ctx.key] = kept
        return (None, None, None, dx) + tuple(grads[k] for k in ctx.keys)


def _hg_apply(net, which, prefixes, x, params):
    from . import native
    own = net.hg_parameters()
    keys = [k for p in prefixes for k in native.hg_block_keys(p)]
    if params is None:
        params = own
    missing = [k for k in keys if k not in params]
    if missing:
        raise ValueError("params lacks %s" % missing[:3])
    return _HgModule.apply(net, which, keys, x, *[params[k] for k in keys])


def conv_block(net, prefix, x, params=None):
    """ConvBlock `prefix` of image_filter_lr (conv2. / top_m_{s}. / m{s}.b1_{l}. ...) of SuRSNet `net` on x [B,256,h,w], with a grad_fn:
    its backward is net.conv_block_backward() and hands x its gradient and the block's nine entries of `params` - default
    net.hg_parameters() - theirs, summed over the batch in image order.  The VALUES are those of the PACKED weights the forward runs on: net.commit()
    after an optimiser step (see super_res_features)."""
    _, _, prefixes = net._hg_module(prefix)
    return _hg_apply(net, prefixes[0], prefixes, x, params)


def hourglass(net, stack, x, params=None):
    """The HourGlass module image_filter_lr.m{stack} on x [B,256,h,w] (h, w multiples of 2^hg_depth), with a grad_fn: its backward is
    net.hourglass_backward() and hands x and every parameter of the module its gradient.  With conv_block and stack_tail this
    composes a trainable filter_lr; filter_lr below is that composition as one call ("Hourglass gradients")."""
    _, _, prefixes = net._hg_module(int(stack))
    return _hg_apply(net, int(stack), prefixes, x, params)


class _StackTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, stack, keys, ll, previous, *params):
        out, nxt = net.stack_tail_train(stack, ll, previous)
        ctx.net, ctx.stack, ctx.keys, ctx.tapes = net, stack, keys, net._hg_tapes[("tail", stack)]
        ctx.set_materialize_grads(False)
        if nxt is None:
            return out.clone()
        return out.clone(), nxt.clone()

    @staticmethod
    def backward(ctx, g_out, g_next=None):
        net, key = ctx.net, ("tail", ctx.stack)
        kept = net._hg_tapes.get(key)
        net._hg_tapes[key] = ctx.tapes   # the tapes of THIS forward, whatever ran on the net since
        try:
            d_ll, d_prev, grads = net.stack_tail_backward(ctx.stack, g_out, g_next)
        finally:
            if kept is None:
                del net._hg_tapes[key]
            else:
                net._hg_tapes[key] = kept
        return (None, None, None, d_ll, d_prev) + tuple(grads[k] for k in ctx.keys)


def _hg_keys(net, keys, params):
    if params is None:
        params = net.hg_parameters()
    missing = [k for k in keys if k not in params]
    if missing:
        raise ValueError("params lacks %s" % missing[:3])
    return params


def stack_tail(net, stack, ll, previous=None, params=None):
    """The tail of stack `stack` of image_filter_lr on ll [B,256,h,w] (and previous, for every stack but the last), with a grad_fn:
    returns out, or (out, next) for a stack that is not the last; its backward is net.stack_tail_backward() and hands ll, previous
    and the tail's entries of `params` - default net.hg_parameters() - their gradients.  The VALUES are those of the PACKED weights,
    the merged next{s} included: net.commit() after an optimiser step."""
    from . import native
    stack = int(stack)
    keys = native.hg_tail_keys(stack, net.opt.num_stack_lr)
    params = _hg_keys(net, keys, params)
    return _StackTail.apply(net, stack, keys, ll, previous, *[params[k] for k in keys])


class _FilterLr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, keys, x, *params):
        outs = net.filter_lr_train(x)
        ctx.net, ctx.keys, ctx.tapes = net, keys, net._hg_tapes["filter_lr"]
        ctx.set_materialize_grads(False)
        return tuple(o.clone() for o in outs)

    @staticmethod
    def backward(ctx, *gs):
        net = ctx.net
        kept = net._hg_tapes.get("filter_lr")
        net._hg_tapes["filter_lr"] = ctx.tapes
        try:
            dx, grads = net.filter_lr_backward(list(gs))
        finally:
            if kept is None:
                del net._hg_tapes["filter_lr"]
            else:
                net._hg_tapes["filter_lr"] = kept
        return (None, None, dx) + tuple(grads[k] for k in ctx.keys)


def filter_lr(net, feature_lr, params=None):
    """HGFilter.forward of SuRSNet `net` on feature_lr [B,256,h,w] with a grad_fn: the list of every stack's output; its backward is
    net.filter_lr_backward() - ONE call for the whole filter - and hands feature_lr and every entry of `params` (default
    net.hg_parameters(), all of its keys) their gradients.  net.commit() after an optimiser step, as for the modules."""
    keys = list(net.hg_parameters())
    params = _hg_keys(net, keys, params)
    return list(_FilterLr.apply(net, keys, feature_lr, *[params[k] for k in keys]))
