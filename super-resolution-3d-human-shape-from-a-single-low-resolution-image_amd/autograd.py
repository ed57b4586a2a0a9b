"""The point path as a torch.autograd.Function: gather, both classifiers on every kept stack and the three classifier terms of
SuRSNet.forward's loss, differentiable with respect to the feature maps.  An encoder that has a backward of its own - a torch encoder
under autograd - trains against this library's point evaluator through it.  super_res_features, conv_block, hourglass,
stack_tail and filter_lr are the parts of the encoder that have a backward here, each through the one Function _Taped; nothing else in
the package grows an autograd graph."""
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


class _Taped(torch.autograd.Function):
    """One taped module of the encoder: train(*inputs) -> its outputs, the tapes it files under `module` in net._tapes kept HERE;
    backward(the outputs' gradients - None where none arrived -, those tapes) -> (every input's gradient ..., key -> parameter
    gradient).  The first n_in of `tensors` are the inputs, the others the parameters behind `keys`."""
    @staticmethod
    def forward(ctx, net, module, train, backward, keys, n_in, *tensors):
        outs = train(*tensors[:n_in])
        ctx.backward_fn, ctx.keys, ctx.tapes = backward, keys, net._tapes[module]   # the tapes of THIS forward, whatever runs on net later
        ctx.set_materialize_grads(False)   # an output nothing differentiates arrives as None, not as a map of zeros
        # (fresh tensors for autograd to own: the model keeps its NHWC views)
        return tuple(o.clone() for o in outs)

    @staticmethod
    def backward(ctx, *gs):
        *d_inputs, grads = ctx.backward_fn(gs, ctx.tapes)
        return (None,) * 6 + tuple(d_inputs) + tuple(grads[k] for k in ctx.keys)


def _taped(net, module, train, backward, keys, inputs, params, own):
    if params is None:
        params = own
    missing = [k for k in keys if k not in params]
    if missing:
        raise ValueError("params lacks %s" % missing[:3])
    return _Taped.apply(net, module, train, backward, keys, len(inputs), *inputs, *[params[k] for k in keys])


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
    own = net.sr_parameters()
    keys = list(own)
    if params is not None and list(params) != keys:
        raise ValueError("params must hold net.sr_parameters()'s keys in their order")

    def train(x):
        img_SR, feature_lr, _ = net.super_res_train(x)
        return img_SR, feature_lr, net.im_feat_list_hr[0]

    def backward(gs, tapes):
        if all(g is None for g in gs):      # (nothing to go back through, and super_res_backward() refuses the call)
            return None, dict.fromkeys(keys)
        return None, net.super_res_backward(*gs, tapes=tapes)
    return _taped(net, net.SR_TAPES, train, backward, keys, (images_lr,), params, own)


def _hg_module(net, which, train, backward, x, params):
    _, _, prefixes, module = net._hg_module(which)
    keys = [k for p in prefixes for k in native.hg_block_keys(p)]
    return _taped(net, module, lambda x: (train(which, x),), lambda gs, tapes: backward(which, gs[0], tapes=tapes), keys, (x,), params,
                  net.hg_parameters())[0]


def conv_block(net, prefix, x, params=None):
    """ConvBlock `prefix` of image_filter_lr (conv2. / top_m_{s}. / m{s}.b1_{l}. ...) of SuRSNet `net` on x [B,256,h,w], with a grad_fn:
    its backward is net.conv_block_backward() and hands x its gradient and the block's nine entries of `params` - default
    net.hg_parameters() - theirs, summed over the batch in image order.  The VALUES are those of the PACKED weights the forward runs on: net.commit()
    after an optimiser step (see super_res_features)."""
    return _hg_module(net, prefix, net.conv_block_train, net.conv_block_backward, x, params)


def hourglass(net, stack, x, params=None):
    """The HourGlass module image_filter_lr.m{stack} on x [B,256,h,w] (h, w multiples of 2^hg_depth), with a grad_fn: its backward is
    net.hourglass_backward() and hands x and every parameter of the module its gradient.  With conv_block and stack_tail this
    composes a trainable filter_lr; filter_lr below is that composition as one call ("Hourglass gradients")."""
    return _hg_module(net, int(stack), net.hourglass_train, net.hourglass_backward, x, params)


def stack_tail(net, stack, ll, previous=None, params=None):
    """The tail of stack `stack` of image_filter_lr on ll [B,256,h,w] (and previous, for every stack but the last), with a grad_fn:
    returns out, or (out, next) for a stack that is not the last; its backward is net.stack_tail_backward() and hands ll, previous
    and the tail's entries of `params` - default net.hg_parameters() - their gradients.  The VALUES are those of the PACKED weights,
    the merged next{s} included: net.commit() after an optimiser step."""
    stack = int(stack)
    outs = _taped(net, ("tail", stack), lambda ll, previous: [o for o in net.stack_tail_train(stack, ll, previous) if o is not None],
                  lambda gs, tapes: net.stack_tail_backward(stack, *gs, tapes=tapes), native.hg_tail_keys(stack, net.opt.num_stack_lr),
                  (ll, previous), params, net.hg_parameters())
    return outs if len(outs) > 1 else outs[0]


def filter_lr(net, feature_lr, params=None):
    """HGFilter.forward of SuRSNet `net` on feature_lr [B,256,h,w] with a grad_fn: the list of every stack's output; its backward is
    net.filter_lr_backward() - ONE call for the whole filter - and hands feature_lr and every entry of `params` (default
    net.hg_parameters(), all of its keys) their gradients.  net.commit() after an optimiser step, as for the modules."""
    own = net.hg_parameters()
    return list(_taped(net, "filter_lr", net.filter_lr_train, lambda gs, tapes: net.filter_lr_backward(list(gs), tapes=tapes), list(own),
                       (feature_lr,), params, own))
