"""Training driver: the flags, flow and files of the reference's apps/train_SuRS.py:27-222 on this package.

    python -m surs_amd.apps.train_SuRS --residual --dataroot D --loadSize 512 --name run --batch_size 2 --num_sample_inout 6000 \
        --checkpoints_path C --results_path R [--optimizer ADAM] [--load_netG_checkpoint_path W] [--continue_train 0 --resume_epoch 3]

Per step: optimizerG.zero_grad(); netG.forward_backward(..., encoder=True) - one taped forward and the gradients of every trained
parameter -; optimizerG.step(grads, guard=True), which applies nothing when a gradient is not finite.  Files, as the reference writes
them: <checkpoints_path>/<name>/netG_latest and netG_epoch_<e> (torch.save of netG.state_dict(): the reference loads them, and this
package's eval driver does), <results_path>/<name>/<e>pred.ply, <e>pred_gt.ply, <e>pred_lr.ply every --freq_save_ply steps, and per
epoch test_eval_epoch<e>_<subject>_{HR,LR}.obj / train_eval_epoch<e>_... unless --no_gen_mesh.  --continue_train 0 resumes from
netG_latest, or from netG_epoch_<--resume_epoch>, at epoch max(resume_epoch, 0) - the reference's own reading of the two flags.

Differences: the dataset builds its items on the device (data.TrainDataset(images="device")) and refuses DataLoader workers, so
--num_threads is not read; --seed drives the dataset's samples, the loader's shuffle and the host generators the augmentations
draw from, so that a run repeats bit for bit; error.item() - a synchronisation - is taken only every --freq_plot steps; a step whose
features or gradients are not finite is skipped and counted on that line; --num_views 1 only (forward_backward's limit); at the
end of an epoch netG_latest is written together with netG_epoch_<e> (the reference writes only the numbered file there, and
netG_latest every --freq_save steps), so that --continue_train 0 finds the newest weights also when an epoch has fewer steps than that;
--no_octree makes the per-epoch meshes by the dense sweep, as in the eval driver (the octree's first level is a 64^3 lattice, in the
reference too: a --resolution below 64 evaluates nothing and has no surface).

Data-parallel (--world_size N, one node): N processes train ONE model, rank r on GPU r % device_count.  --world_size N without --rank
starts the N ranks as fresh child processes (the parent never touches a GPU and only waits for them); with --rank r this process IS
rank r (a launcher of your own).  --dist_backend nccl | gloo, --dist_url and --dist_timeout go to init_process_group: nothing is read
from the environment.  Per step every rank runs forward_backward on its OWN batch - the epoch's batches are dealt by
dist.shard_indices, the tail that does not fill a round is dropped - and dist.TrainGroup.step all-gathers the gradients and applies
their rank-ordered mean in one launch, the same bits on every rank.  THE EFFECTIVE BATCH IS world_size x --batch_size AND THE
LEARNING RATE IS THE USER'S: nothing is rescaled.  The host generators are seeded from (seed, rank), so the augmentations differ per
rank; the dataset's item seeds are per index already.  The plotted error is the mean over the ranks (one small all-gather, only where
the .item() synchronises anyway); rank 0 alone writes checkpoints and PLY dumps; the per-epoch meshes are dealt round-robin over the
ranks under their usual names; the replicas' masters are compared once per epoch (TrainGroup.assert_replicas_equal).  A peer that
dies ends the run with an error after --dist_timeout seconds instead of a hang.  --world_size 1 is the run described above, byte for
byte."""
import gc
import os
import random
import sys
import time

import numpy as np
import torch
from torch.utils.data import DataLoader

from .. import optim
from .._lib import NonFiniteVolumeError
from ..data import TrainDataset
from ..model import SuRSNet
from ..options import BaseOptions
from ..sample_util import save_samples_truncted_prob
from ..train_util import adjust_learning_rate, gen_mesh, reshape_multiview_tensors, reshape_sample_tensor


def checkpoint_paths(opt, epoch):
    """(netG_latest, netG_epoch_<epoch>) under <checkpoints_path>/<name>."""
    base = "%s/%s" % (opt.checkpoints_path, opt.name)
    return base + "/netG_latest", base + "/netG_epoch_%d" % epoch


def resume_plan(opt):
    """(the checkpoint --continue_train / --resume_epoch ask for, or None; the first epoch): apps/train_SuRS.py:84-107 - 0 means
    resume; any other value starts at epoch 0 from whatever --load_netG_checkpoint_path loaded."""
    if opt.continue_train != 0:
        return None, 0
    latest, numbered = checkpoint_paths(opt, opt.resume_epoch)
    return (latest if opt.resume_epoch < 0 else numbered), max(opt.resume_epoch, 0)


def save_ply_dumps(opt, epoch, res_hr, sample_hr, label_hr, sample_lr, label_lr):
    """The three point clouds of image 0: the hr prediction and the hr labels on the hr samples, the lr labels on the lr samples."""
    base = "%s/%s/%d" % (opt.results_path, opt.name, epoch)
    pts = lambda t: t[0].transpose(0, 1).detach().cpu().numpy()
    val = lambda t: t[0].detach().cpu().numpy()
    save_samples_truncted_prob(base + "pred.ply", pts(sample_hr), val(res_hr))
    save_samples_truncted_prob(base + "pred_gt.ply", pts(sample_hr), val(label_hr))
    save_samples_truncted_prob(base + "pred_lr.ply", pts(sample_lr), val(label_lr))


def _init_ranks(opt):
    """(world, rank, whether this call initialised the process group) of --world_size / --rank."""
    import datetime
    import torch.distributed as tdist
    world, rank = int(getattr(opt, "world_size", 1) or 1), int(getattr(opt, "rank", -1))
    if world <= 1:
        return 1, 0, False
    if tdist.is_initialized():
        return tdist.get_world_size(), tdist.get_rank(), False
    if not 0 <= rank < world:
        raise ValueError("--world_size %d needs --rank 0 .. %d in a process that trains (main() starts the ranks without it)" % (world, world - 1))
    tdist.init_process_group(opt.dist_backend, init_method=opt.dist_url, rank=rank, world_size=world,
                             timeout=datetime.timedelta(seconds=float(opt.dist_timeout)))
    return world, rank, True


def _epoch_loader(opt, dataset, seed, epoch, rank, world):
    """Rank `rank`'s DataLoader of one data-parallel epoch: every rank forms the same item order (seeded by (seed, epoch); the
    dataset's own with --serial_batches) and the same batches of --batch_size, and takes dist.shard_indices' share of them."""
    from ..dist import shard_indices
    n = len(dataset)
    order = list(range(n)) if opt.serial_batches else torch.randperm(n, generator=torch.Generator().manual_seed(seed + epoch)).tolist()
    batches = [order[i:i + opt.batch_size] for i in range(0, n, opt.batch_size)]
    mine = [batches[i] for i in shard_indices(len(batches), rank, world, seed=seed + epoch, shuffle=not opt.serial_batches)]
    return DataLoader(dataset, batch_sampler=mine, num_workers=0)


def train(opt, datasets=None, net=None, log=print, device=None):
    """The reference's train(opt).  datasets: (train, test) TrainDataset-like objects built by the caller instead of the two this
    function builds from opt; net: a SuRSNet-like object instead of a new SuRSNet(opt); device: instead of cuda:<--gpu_id> (of
    cuda:<rank % device_count> with --world_size above 1).  Returns a dict of what happened: first_epoch, steps, skipped, the last
    learning rate, the plotted errors [(epoch, step, error)], world, rank and - data-parallel - the digest the replicas agreed on
    at the end of the last epoch."""
    world, rank, own_group = _init_ranks(opt)
    try:
        return _train(opt, datasets, net, log if rank == 0 else (lambda *a, **k: None), device, world, rank)
    finally:
        if own_group:
            import torch.distributed as tdist
            tdist.destroy_process_group()


def _train(opt, datasets, net, log, device, world, rank):
    if device is not None:
        cuda = torch.device(device)
    elif world > 1:
        cuda = torch.device("cuda:%d" % (rank % torch.cuda.device_count()))
    else:
        cuda = torch.device("cuda:%d" % opt.gpu_id)
    seed = int(getattr(opt, "seed", 0))
    random.seed(seed + 7919 * rank)        # (rank 0, and the only rank of world 1: the seed itself)
    np.random.seed(seed + 7919 * rank)
    if datasets is None:
        torch.cuda.set_device(cuda)
        datasets = (TrainDataset(opt, "train", seed=seed, images="device"), TrainDataset(opt, "test", seed=seed, images="device"))
    train_dataset, test_dataset = datasets
    # (num_workers=0: the dataset makes its items on the GPU of this process and refuses workers)
    shuffle = torch.Generator().manual_seed(seed)
    train_data_loader = DataLoader(train_dataset, batch_size=opt.batch_size, shuffle=not opt.serial_batches, num_workers=0, generator=shuffle)
    if world > 1:
        torch.cuda.set_device(cuda)
        train_data_loader = _epoch_loader(opt, train_dataset, seed, 0, rank, world)
    log("train data size: ", len(train_data_loader))
    log("test data size: ", len(test_dataset))

    netG = SuRSNet(opt, train_dataset.projection_mode).to(device=cuda) if net is None else net
    log("Using Network: ", netG.name)
    if opt.load_netG_checkpoint_path is not None:
        log("loading for net G ...", opt.load_netG_checkpoint_path)
        netG.load_state_dict(torch.load(opt.load_netG_checkpoint_path, map_location="cpu"))
    model_path, start_epoch = resume_plan(opt)
    if model_path is not None:
        log("Resuming from ", model_path)
        netG.load_state_dict(torch.load(model_path, map_location="cpu"))
    # (after the weights: an Optimizer holds the masters of the state dict it was built on)
    optimizerG = optim.from_options(netG, opt)
    lr = opt.learning_rate
    group = None
    if world > 1:
        from ..dist import TrainGroup
        group = TrainGroup(netG, optimizerG)
        group.broadcast_state(0)           # one set of weights and one optimiser state, whatever each rank initialised or loaded

    for d in (opt.checkpoints_path, opt.results_path, "%s/%s" % (opt.checkpoints_path, opt.name), "%s/%s" % (opt.results_path, opt.name)):
        os.makedirs(d, exist_ok=True)

    done = dict(first_epoch=start_epoch, steps=0, skipped=0, lr=lr, errors=[], world=world, rank=rank, digest=None)
    for epoch in range(start_epoch, opt.num_epoch):
        epoch_start_time = time.time()
        gc.collect()
        netG.train()
        iter_data_time = time.time()
        if world > 1:
            train_data_loader = _epoch_loader(opt, train_dataset, seed, epoch, rank, world)
        for train_idx, train_data in enumerate(train_data_loader):
            iter_start_time = time.time()
            image_tensor_hr, image_tensor_lr, calib_tensor = reshape_multiview_tensors(
                train_data["img_HR"].to(device=cuda), train_data["img_LR"].to(device=cuda), train_data["calib"].to(device=cuda))
            sample_tensor_lr = reshape_sample_tensor(train_data["samples_LR"].to(device=cuda), opt.num_views)
            sample_tensor_hr = reshape_sample_tensor(train_data["samples_HR"].to(device=cuda), opt.num_views)
            label_tensor_hr = train_data["labels_HR"].to(device=cuda)
            label_tensor_lr = train_data["labels_disp"].to(device=cuda)

            optimizerG.zero_grad()
            try:
                res_hr, error, res_lr, grads = netG.forward_backward(image_tensor_lr, image_tensor_hr, sample_tensor_lr, sample_tensor_hr,
                                                                     calib_tensor, labels_lr=label_tensor_lr, labels_hr=label_tensor_hr,
                                                                     encoder=True)
                stepped = optimizerG.step(grads, guard=True) if group is None else group.step(grads, guard=True)
            except NonFiniteVolumeError:      # (non-finite feature maps: nothing was stepped - on any rank: the peers skip with this one)
                res_hr, error, stepped = None, None, False
                if group is not None:
                    group.fail()
            done["steps"] += 1
            if stepped is False:
                done["skipped"] += 1

            iter_net_time = time.time()
            eta = ((iter_net_time - epoch_start_time) / (train_idx + 1)) * len(train_data_loader) - (iter_net_time - epoch_start_time)
            if train_idx % opt.freq_plot == 0:
                err = float("nan") if error is None else error.item()
                if group is not None:
                    err = group.mean_over_ranks(err)
                done["errors"].append((epoch, train_idx, err))
                log("Name: {0} | Epoch: {1} | {2}/{3} | Err: {4:.06f}  | LR: {5:.06f} | Sigma: {6:.02f} | dataT: {7:.05f} | netT: {8:.05f} | "
                    "ETA: {9:02d}:{10:02d} | skipped: {11}".format(opt.name, epoch, train_idx, len(train_data_loader), err, lr, opt.sigma,
                                                                   iter_start_time - iter_data_time, iter_net_time - iter_start_time,
                                                                   int(eta // 60), int(eta - 60 * (eta // 60)), done["skipped"]))
            if train_idx % opt.freq_save == 0 and train_idx != 0 and rank == 0:
                for path in checkpoint_paths(opt, epoch):
                    torch.save(netG.state_dict(), path)
            if train_idx % opt.freq_save_ply == 0 and res_hr is not None and rank == 0:
                save_ply_dumps(opt, epoch, res_hr, sample_tensor_hr, label_tensor_hr, sample_tensor_lr, label_tensor_lr)
            iter_data_time = time.time()
        # the end of an epoch: its numbered checkpoint, and netG_latest with it, so that --continue_train 0 finds the newest weights
        if group is not None:
            done["digest"] = group.assert_replicas_equal()
        for path in checkpoint_paths(opt, epoch) if rank == 0 else ():
            torch.save(netG.state_dict(), path)
        lr = adjust_learning_rate(optimizerG, epoch, lr, opt.schedule, opt.gamma)
        done["lr"] = lr

        with torch.no_grad():
            netG.eval()
            if not opt.no_gen_mesh:
                log("generate mesh (test) ...")
                for ev in range(opt.num_gen_mesh_test):
                    if ev % world != rank:             # (the meshes are dealt round-robin over the ranks)
                        continue
                    test_data = test_dataset[ev]
                    gen_mesh(opt, netG, cuda, test_data, "%s/%s/test_eval_epoch%d_%s.obj" % (opt.results_path, opt.name, epoch,
                                                                                             test_data["name"][0]),
                             use_octree=not opt.no_octree)
                log("generate mesh (train) ...")
                train_dataset.is_train = False
                try:
                    for ev in range(opt.num_gen_mesh_test):
                        if (opt.num_gen_mesh_test + ev) % world != rank:
                            continue
                        item = train_dataset[ev]
                        gen_mesh(opt, netG, cuda, item, "%s/%s/train_eval_epoch%d_%s.obj" % (opt.results_path, opt.name, epoch,
                                                                                            item["name"][0]),
                                 use_octree=not opt.no_octree)
                finally:
                    train_dataset.is_train = True
    return done


def launch(opt, argv):
    """--world_size N without --rank: start the N ranks as fresh child processes running main(argv + --rank r) and wait for them.  This
    process initialises no GPU and replaces no program.  A rank that fails ends the others (they would otherwise wait for it until
    --dist_timeout); returns the first non-zero exit status, or 0."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(sys.modules[__package__.split(".")[0]].__file__)))
    code = "import sys; sys.path.insert(0, %r); from %s.train_SuRS import main; main(sys.argv[1:])" % (root, __package__)
    procs = [subprocess.Popen([sys.executable, "-c", code] + list(argv) + ["--rank", str(r)]) for r in range(opt.world_size)]
    status = 0
    try:
        while any(p.poll() is None for p in procs):
            time.sleep(0.2)
            bad = [p.returncode for p in procs if p.poll() not in (None, 0)]
            if bad:
                status = bad[0]
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    return status or next((p.returncode for p in procs if p.returncode), 0)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    opt = BaseOptions().parse(argv)
    if opt.world_size > 1 and opt.rank < 0:
        status = launch(opt, argv)
        if status:
            raise SystemExit("train_SuRS: a rank ended with status %d" % status)
        return
    train(opt)


if __name__ == "__main__":
    main(sys.argv[1:])
