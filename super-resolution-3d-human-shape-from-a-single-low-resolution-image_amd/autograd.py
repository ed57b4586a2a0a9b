"""The point path as a torch.autograd.Function: gather, both classifiers on every kept stack and the three classifier terms of
SuRSNet.forward's loss, differentiable with respect to the feature maps.  An encoder that has a backward of its own - a torch encoder
under autograd - trains against this library's point evaluator through it.  Nothing else in the package grows an autograd graph."""
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
