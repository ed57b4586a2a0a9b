"""gen_mesh: the per-subject driver (/root/reference/lib/train_util.py:53-85), same signature and side effects:
encoder (super_res -> filter_hr -> filter_lr), calib diag(2,-2,2,1), reconstruction, two OBJ files."""
import numpy as np
import torch

from .mesh_util import reconstruction, save_obj_mesh


def gen_calib():
    m = np.identity(4) * 2
    m[1, 1] = -2
    m[3, 3] = 1
    return torch.from_numpy(m.astype(np.float32)).unsqueeze(0)


def gen_mesh(opt, net, cuda, data, save_path, use_octree=True):
    image_tensor = data["img_LR"].to(device=cuda)
    img_sr, feature_lr, feature_hr = net.super_res(image_tensor)
    net.filter_hr(feature_hr)
    net.filter_lr(feature_lr)
    calib_tensor = gen_calib().to(device=cuda)   # the dataset's own calib is ignored, as in the reference
    verts_hr, faces_hr, _, _, verts_lr, faces_lr, _, _ = reconstruction(
        opt, net, cuda, calib_tensor, opt.resolution, data["b_min"], data["b_max"], use_octree=use_octree,
        num_samples=opt.num_samples, want_normals=False)   # normals / values are discarded here, as in the reference
    save_obj_mesh(save_path[:-4] + "_HR.obj", verts_hr, faces_hr)
    save_obj_mesh(save_path[:-4] + "_LR.obj", verts_lr, faces_lr)
    return verts_hr, faces_hr, verts_lr, faces_lr


def gen_mesh_metrics(opt, net, cuda, data, save_path=None, use_octree=True, n=10000, seed=0, gt_hr=None, gt_lr=None,
                     normal_views=None, normal_size=512):
    """gen_mesh's reconstruction of one item, scored against the item's ground-truth scans: {"HR": metrics.mesh_metrics(the HR
    volume's mesh, the HR scan), "LR": (the LR volume's mesh, the LR scan)}, each from n surface samples per mesh.  The predicted
    vertices are taken into the scans' frame first (metrics.pred_to_gt_transform(data['calib']): the identity without a calib), so
    the distances are in the dataset's units.  The scans are data['mesh_path_HR'] / ['mesh_path_LR'] (OBJ files) unless gt_hr /
    gt_lr hand in meshes (native.Mesh or (verts, faces)).  With a save_path the two OBJ files of gen_mesh are written as well.
    normal_views: a tuple of turntable degrees, e.g. (0, 90, 180, 270), adds the normal reprojection error to each of the two
    (metrics.normal_error at normal_size through metrics.turntable_views(data['calib'][0], degrees, the centre of the scan's
    bounding box); the item needs its calib then): normal_error, normal_per_view, mask_iou.  None: today's keys."""
    from . import metrics
    from .mesh_util import load_obj_mesh
    n = metrics.check_samples(n)
    for key, given in (("mesh_path_HR", gt_hr), ("mesh_path_LR", gt_lr)):
        if given is None and key not in data:
            raise ValueError("gen_mesh_metrics: the item has no %r and no ground-truth mesh was handed in" % key)
    if normal_views is not None and data.get("calib") is None:
        raise ValueError("gen_mesh_metrics: normal_views needs the item's calib")
    to_gt = metrics.pred_to_gt_transform(data.get("calib"))
    image_tensor = data["img_LR"].to(device=cuda)
    img_sr, feature_lr, feature_hr = net.super_res(image_tensor)
    net.filter_hr(feature_hr)
    net.filter_lr(feature_lr)
    calib_tensor = gen_calib().to(device=cuda)
    verts_hr, faces_hr, _, _, verts_lr, faces_lr, _, _ = reconstruction(
        opt, net, cuda, calib_tensor, opt.resolution, data["b_min"], data["b_max"], use_octree=use_octree,
        num_samples=opt.num_samples, want_normals=False)
    if save_path is not None:
        save_obj_mesh(save_path[:-4] + "_HR.obj", verts_hr, faces_hr)
        save_obj_mesh(save_path[:-4] + "_LR.obj", verts_lr, faces_lr)
    gt_hr = load_obj_mesh(data["mesh_path_HR"]) if gt_hr is None else gt_hr
    gt_lr = load_obj_mesh(data["mesh_path_LR"]) if gt_lr is None else gt_lr
    scores = {}
    for key, verts, faces, gt in (("HR", verts_hr, faces_hr, gt_hr), ("LR", verts_lr, faces_lr, gt_lr)):
        pred = (metrics.transform_verts(to_gt, verts), faces)
        if normal_views is None:
            scores[key] = metrics.mesh_metrics(pred, gt, n=n, seed=seed)
            continue
        pred, gt = metrics.as_mesh(pred), metrics.as_mesh(gt)
        scores[key] = metrics.mesh_metrics(pred, gt, n=n, seed=seed)
        views = metrics.turntable_views(data["calib"], tuple(normal_views), metrics.box_centre(gt))
        ne = metrics.normal_error(pred, gt, views, size=normal_size)
        scores[key].update(normal_error=ne["normal_error"], normal_per_view=ne["per_view"], mask_iou=ne["mask_iou"])
    return scores


def gen_mesh_pipelined(opt, net, cuda, dataset, indices, save_path_of, use_octree=True, write=True):
    """gen_mesh for a run of subjects (the loop of /root/reference/apps/eval_SuRS.py:74-80) as a pipeline: while the GPU sweeps
    subject i, (1) a host thread decodes subject i+1's image and mask, (2) its pixels are uploaded and normalised / masked
    on the device (data.DeviceInputStage) and its encoder is enqueued on a second stream - behind subject i's sweep launches,
    before the host starts driving subject i's mesh extraction, so it fills the sweep's gaps and tail - and (3) another host
    thread writes subject i-1's OBJ files.  Same files and meshes as calling gen_mesh per subject.
    dataset: get_raw_item(index) -> {'name', 'b_min', 'b_max', 'rgb' uint8 [H,W,3], 'mask' uint8 [H,W]}.
    Returns [(verts_hr, faces_hr, verts_lr, faces_lr)] in order."""
    from concurrent.futures import ThreadPoolExecutor
    from .data import DeviceInputStage
    indices = list(indices)
    if not indices:
        return []
    dev = torch.device(cuda)
    stage = DeviceInputStage(dev)
    enc_stream = torch.cuda.Stream(device=dev)
    main = torch.cuda.current_stream(dev)
    calib_tensor = gen_calib().to(device=dev)
    decoder, writer = ThreadPoolExecutor(1), ThreadPoolExecutor(1)
    results, writes = [], []

    def encode(raw):
        # everything here is allocated, written and read on enc_stream (the caching allocator keeps per-stream pools); the
        # feature maps are handed to the main stream through `ev` + record_stream
        with torch.cuda.stream(enc_stream):
            feats = net.encode_image(stage.prepare(raw["rgb"], raw["mask"]))
            ev = torch.cuda.Event()
            ev.record(enc_stream)
        return feats, ev

    try:
        pending = decoder.submit(dataset.get_raw_item, indices[0])
        raw = pending.result()
        pending = decoder.submit(dataset.get_raw_item, indices[1]) if len(indices) > 1 else None
        feats, ready = encode(raw)
        for n, idx in enumerate(indices):
            cur_raw, cur_feats = raw, feats
            main.wait_event(ready)
            for f in cur_feats:
                f.buf.record_stream(main)
            nxt = {}

            def enqueue_next():
                if pending is not None:
                    nxt["raw"] = pending.result()
                    nxt["feats"], nxt["ready"] = encode(nxt["raw"])

            verts_hr, faces_hr, _, _, verts_lr, faces_lr, _, _ = reconstruction(
                opt, net, dev, calib_tensor, opt.resolution, cur_raw["b_min"], cur_raw["b_max"], use_octree=use_octree,
                num_samples=opt.num_samples, want_normals=False, features=cur_feats, after_enqueue=enqueue_next)
            if pending is not None:
                raw, feats, ready = nxt["raw"], nxt["feats"], nxt["ready"]
                pending = decoder.submit(dataset.get_raw_item, indices[n + 2]) if n + 2 < len(indices) else None
            results.append((verts_hr, faces_hr, verts_lr, faces_lr))
            if write:
                path = save_path_of(cur_raw)
                writes.append(writer.submit(save_obj_mesh, path[:-4] + "_HR.obj", verts_hr, faces_hr))
                writes.append(writer.submit(save_obj_mesh, path[:-4] + "_LR.obj", verts_lr, faces_lr))
        for w in writes:
            w.result()
    finally:
        decoder.shutdown(wait=True)
        writer.shutdown(wait=True)
    return results


def adjust_learning_rate(optimizer, epoch, lr, schedule, gamma):
    """The step schedule of the reference's training loop (/root/reference/lib/train_util.py:89-95), same signature: at an epoch listed
    in `schedule` the rate becomes lr * gamma and is written into every group of optimizer.param_groups - a torch.optim optimiser's or
    optim.Optimizer's, which reads it at its next step; any other epoch changes nothing.  Returns the rate to carry on with."""
    if epoch not in schedule:
        return lr
    lr = lr * gamma
    for group in optimizer.param_groups:
        group["lr"] = lr
    return lr


def reshape_multiview_tensors(image_tensor_hr, image_tensor_lr, calib_tensor):
    """The loader's [B, num_views, ...] tensors flattened to [B num_views, ...], as /root/reference/lib/train_util.py:14-38 does and in
    its argument order: (image_tensor_hr [B V,C,H,W], image_tensor_lr [B V,C,h,w], calib_tensor [B V,4,4]) - views, no copies."""
    flat = lambda t: t.view((t.shape[0] * t.shape[1],) + tuple(t.shape[2:]))
    if image_tensor_hr.dim() != 5 or image_tensor_lr.dim() != 5 or calib_tensor.dim() != 4:
        raise ValueError("reshape_multiview_tensors: [B,V,C,H,W] images and [B,V,4,4] calibrations are expected, not %s, %s, %s" % (
            tuple(image_tensor_hr.shape), tuple(image_tensor_lr.shape), tuple(calib_tensor.shape)))
    return flat(image_tensor_hr), flat(image_tensor_lr), flat(calib_tensor)


def reshape_sample_tensor(sample_tensor, num_views):
    """sample_tensor [B,3,N] repeated once per view, view-minor: [B num_views,3,N] (/root/reference/lib/train_util.py:41-51); the
    tensor itself for one view."""
    if num_views == 1:
        return sample_tensor
    B, c, n = sample_tensor.shape
    return sample_tensor.unsqueeze(1).repeat(1, num_views, 1, 1).view(B * num_views, c, n)
