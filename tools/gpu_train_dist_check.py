"""dist.TrainGroup end to end on ONE GPU: `world` processes share cuda:0 (gloo with host staging, as tools/gpu_slab_check.py: RCCL does
not allow two ranks on one device) and train one model data-parallel.  What is checked is exact: bits, counts and file names - and,
in `fixture`, the reference's float64 errors of tests/golden/train_step_tiny.npz within the fixture's own resolution.

    python tools/gpu_train_dist_check.py WORLD MODE

MODE (all on the `tiny` case of tests/train_step_common.py: 4 x 8 images, 300 points):
  same     every rank is fed the same item; three steps of SGD with momentum and of ADAM: every rank's masters and optimiser state
           equal, bit for bit, a single process's three steps on that item ((g + g) * 0.5 == g exactly, for any world that is a power of 2)
  fixture  world 2: the fixture's two images one per rank, one plain SGD step on set `all` of variant w1111 with the fixture's learning
           rate: the batch error before and after within train_step_common.resolution of the reference's float64 values
  odd      distinct items per rank, two ADAM steps: replicas_digest() and the sha256 of the gathered slab identical on all ranks
  poison   rank world - 1 writes a NaN into one gradient on step 2 of 3: every rank returns False, nothing moved, step 3 applies; the
           same through fail()
  app      apps/train_SuRS.train() with --world_size WORLD on a synthetic dataroot of five yaws, batch size 1, one epoch, --no_gen_mesh;
           then --world_size 1 twice in rank 0: explicit and by default, byte-identical checkpoints
  launch   apps/train_SuRS.main() with --world_size WORLD and no --rank, in THIS process, which never touches the GPU: it starts the
           ranks as child processes, they form the group, build datasets, net and optimiser, broadcast rank 0's state and leave
           (--num_epoch 0: the dataroot holds five of the 360 yaws the dataset lists, enough to build it, not to run an epoch);
           then an unknown --dist_backend, which every rank refuses before it touches a device: main() raises SystemExit

Every rank asserts; a failed assertion ends the run with a non-zero status.  Prints one 'ok:' line per mode on success."""
import hashlib
import json
import os
import socket
import sys
import tempfile
from collections import OrderedDict

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASE = "tiny"
STEPS = 3


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _net(variant="w1111"):
    import train_step_common as ts
    from surs_amd import model
    net = model.SuRSNet(ts.opt(CASE, variant)).to(device=torch.device("cuda:0"))
    net.load_state_dict(OrderedDict((k, torch.from_numpy(np.array(v))) for k, v in ts.state_dict(CASE).items()))
    net.train()
    return net


def _inputs():
    import train_step_common as ts
    return {k: torch.from_numpy(v).to("cuda:0") for k, v in ts.inputs(CASE).items()}


def _item(x, image, points=None):
    """forward_backward's arguments for ONE item: image `image` with the points and labels of item `points`."""
    points = image if points is None else points
    i, p = slice(image, image + 1), slice(points, points + 1)
    return ((x["images_lr"][i], x["images_hr"][i], x["points_lr"][p], x["points_hr"][p], x["calibs"][i]),
            dict(labels_lr=x["labels_lr"][p], labels_hr=x["labels_hr"][p]))


def _grads(net, item):
    args, kw = item
    return net.forward_backward(*args, encoder=True, **kw)[3]


def _snapshot(o):
    """The bits a step may move: masters, state slabs, step count, stepped keys."""
    return ([m.detach().clone() for m in o._masters.values()], {n: o._slab(n).clone() for n in o._state_names()}, o._t, set(o._seen))


def _assert_snapshot(o, snap, what):
    masters, slabs, t, seen = snap
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(o._masters.values(), masters)), what + ": masters"
    assert all(torch.equal(_bits(o._slab(n)), _bits(s)) for n, s in slabs.items()), what + ": state"
    assert (o._t, set(o._seen)) == (t, seen), what + ": step count"


def _optimizer(net, kind):
    from surs_amd import optim
    return optim.Optimizer(net, kind, lr=1e-3, momentum=0.9)      # (momentum: SGD's; the other kinds have none)


def mode_same(rank, world):
    from surs_amd import dist as sdist
    x = _inputs()
    for kind in ("SGD", "ADAM"):
        ref = _net()
        o_ref = _optimizer(ref, kind)
        for _ in range(STEPS):
            assert o_ref.step(_grads(ref, _item(x, 0)), guard=True) is True
        net = _net()
        o = _optimizer(net, kind)
        tg = sdist.TrainGroup(net, o)
        tg.broadcast_state(0)
        for _ in range(STEPS):
            assert tg.step(_grads(net, _item(x, 0)), guard=True) is True
        _assert_snapshot(o, _snapshot(o_ref), "same %s rank %d" % (kind, rank))
        sa, sb = o_ref.state_dict(), o.state_dict()
        assert list(sa["state"]) == list(sb["state"]) and len(sa["state"]) == len(o._keys)
        for i in sa["state"]:
            assert all(torch.equal(sa["state"][i][n], sb["state"][i][n]) for n in sa["state"][i]), (kind, i)
        tg.assert_replicas_equal()
    return "%d ranks x %d steps of SGD with momentum and of ADAM equal one process's, bit for bit" % (world, STEPS)


def mode_fixture(rank, world):
    import train_step_common as ts
    from surs_amd import dist as sdist, optim
    assert world == 2
    row = ts.load_fixture(os.path.join(ROOT, "tests", "golden"), CASE)[("w1111", "all")]
    x = _inputs()
    both = ((x["images_lr"], x["images_hr"], x["points_lr"], x["points_hr"], x["calibs"]), dict(labels_lr=x["labels_lr"], labels_hr=x["labels_hr"]))
    net = _net("w1111")
    before = float(net.forward(*both[0], **both[1])[1])
    o = optim.Optimizer(net, "SGD", lr=row["lr"], momentum=0)
    tg = sdist.TrainGroup(net, o)
    tg.broadcast_state(0)
    assert tg.step(_grads(net, _item(x, rank)), guard=True) is True
    after = float(net.forward(*both[0], **both[1])[1])
    r = ts.resolution(row)
    ratios = [abs(e - e64) / r for e, e64 in zip((before, after), row["e64"])]
    if rank == 0:
        print("fixture: error %.9g -> %.9g, reference %.9g -> %.9g, r %.3g, |e - e64| / r = %.3f %.3f, step / r = %.0f" % (
            before, after, row["e64"][0], row["e64"][1], r, ratios[0], ratios[1], row["ratio"]), flush=True)
    assert ratios[0] <= 1.0 and ratios[1] <= 1.0, (before, after, row["e64"], r)
    tg.assert_replicas_equal()
    return "one image per rank, one SGD step: |e - e64| / r = %.3f before, %.3f after" % tuple(ratios)


def mode_odd(rank, world):
    from surs_amd import dist as sdist
    x = _inputs()
    net = _net()
    o = _optimizer(net, "ADAM")
    tg = sdist.TrainGroup(net, o)
    tg.broadcast_state(0)
    item = _item(x, rank % 2, (rank + 1) // 2 % 2)     # 0: (0, 0)  1: (1, 1)  2: (0, 1)  3: (1, 0)
    for _ in range(2):
        assert tg.step(_grads(net, item), guard=True) is True
    digests = tg.replicas_digest()
    assert len(digests) == world and len(set(digests)) == 1, digests
    tg.assert_replicas_equal()
    sha = hashlib.sha256(tg._gathered.cpu().numpy().tobytes()).hexdigest()
    shas = [None] * world
    dist.all_gather_object(shas, sha)
    assert len(set(shas)) == 1, shas
    rows = tg._gathered.cpu().numpy()
    assert all(not np.array_equal(rows[0], rows[r]) for r in range(1, world))      # (the ranks did offer different gradients)
    return "%d ranks on distinct items, two ADAM steps: one digest, one gathered slab" % world


def mode_poison(rank, world):
    from surs_amd import dist as sdist
    x = _inputs()
    net = _net()
    o = _optimizer(net, "ADAM")
    tg = sdist.TrainGroup(net, o)
    tg.broadcast_state(0)
    bad = world - 1
    item = _item(x, rank % 2)
    for leg in ("nan", "fail"):
        skipped = o.skipped
        for step in (1, 2, 3):
            snap = _snapshot(o)
            if step == 2 and rank == bad and leg == "fail":
                stepped = tg.fail()
            else:
                grads = _grads(net, item)
                if step == 2 and rank == bad:
                    grads = OrderedDict((k, v.clone()) for k, v in grads.items())
                    list(grads.values())[3].reshape(-1)[-1] = float("nan")
                stepped = tg.step(grads, guard=True)
            if step == 2:
                assert stepped is False and o.skipped == skipped + 1 and o.last_skipped_rank == bad, (leg, rank, stepped, o.skipped)
                _assert_snapshot(o, snap, "%s rank %d" % (leg, rank))
            else:
                assert stepped is True and o._t == snap[2] + 1, (leg, rank, step)
                assert any(not torch.equal(_bits(a), _bits(b)) for a, b in zip(o._masters.values(), snap[0]))
        tg.assert_replicas_equal()
    return "a NaN of rank %d, and its fail(): every rank skipped step 2 untouched and applied step 3" % bad


# ------------------------------------------------------------------ the app
YAWS = (0, 1, 2, 3, 4)
UNIT = ["--b_min", "-0.5", "-0.5", "-0.5", "--b_max", "0.5", "0.5", "0.5", "--sigma", "0.05", "--z_size", "12.5", "--learning_rate", "1e-6"]


def _app_opt(root, out, name, more=()):
    import train_data_common as tdc
    return tdc.opt(root, size=64, n=200, more=[
        "--residual", "--batch_size", "1", "--num_epoch", "1", "--resolution", "32", "--name", name, "--no_gen_mesh",
        "--checkpoints_path", os.path.join(out, "ck"), "--results_path", os.path.join(out, "res"), "--freq_plot", "1", "--freq_save_ply", "1",
        "--seed", "5", "--no_octree"] + UNIT + list(more))


def _app_run(opt):
    from surs_amd import data
    from surs_amd.apps import train_SuRS
    sets = []
    for phase in ("train", "test"):
        d = data.TrainDataset(opt, phase, seed=opt.seed, images="device")
        d.yaw_list = list(YAWS)
        sets.append(d)
    assert len(sets[0]) == len(YAWS)
    return train_SuRS.train(opt, datasets=tuple(sets), log=lambda *a: None)


def mode_app(rank, world, port, work):
    from surs_amd import model
    root, out = os.path.join(work, "data"), os.path.join(work, "out")
    opt = _app_opt(root, out, "dp", ["--world_size", str(world), "--rank", str(rank), "--dist_backend", "gloo",
                                     "--dist_url", "tcp://127.0.0.1:%d" % port, "--dist_timeout", "120"])
    done = _app_run(opt)
    assert not dist.is_initialized()                  # (train() made the group and took it down)
    with open(os.path.join(work, "done_%d.json" % rank), "w") as f:
        json.dump(done, f)
    assert done["steps"] == len(YAWS) // world and done["skipped"] == 0 and done["digest"] is not None, done
    assert (done["world"], done["rank"]) == (world, rank)
    if rank != 0:
        return None
    ck = os.path.join(out, "ck", "dp")
    assert sorted(os.listdir(ck)) == ["netG_epoch_0", "netG_latest"], os.listdir(ck)
    fresh = model.SuRSNet(opt).to(device=torch.device("cuda:0"))
    fresh.load_state_dict(torch.load(os.path.join(ck, "netG_latest"), map_location="cpu"))
    assert sorted(os.listdir(os.path.join(out, "res", "dp"))) == ["0pred.ply", "0pred_gt.ply", "0pred_lr.ply"]
    assert len(done["errors"]) == done["steps"] and all(np.isfinite(e) and e > 0 for _, _, e in done["errors"])
    # one process: --world_size 1 spelled out is the default run, byte for byte
    _app_run(_app_opt(root, out, "w1", ["--world_size", "1", "--dist_backend", "gloo"]))
    _app_run(_app_opt(root, out, "w0"))
    for name in ("netG_epoch_0", "netG_latest"):
        a, b = (open(os.path.join(out, "ck", n, name), "rb").read() for n in ("w1", "w0"))
        assert a == b, name
    return "%d ranks x %d steps, one batch dropped, one set of checkpoints that loads; --world_size 1 is the default run" % (
        world, done["steps"])


def mode_launch(world, port, work):
    from surs_amd.apps import train_SuRS
    root, out = os.path.join(work, "data"), os.path.join(work, "out")
    flags = ["--dataroot", root, "--loadSize", "64", "--num_sample_inout", "200", "--residual", "--batch_size", "1", "--num_epoch", "0",
             "--name", "launch", "--no_gen_mesh", "--checkpoints_path", os.path.join(out, "ck"), "--results_path", os.path.join(out, "res"),
             "--world_size", str(world), "--dist_url", "tcp://127.0.0.1:%d" % port, "--dist_timeout", "120"] + UNIT
    assert train_SuRS.main(flags + ["--dist_backend", "gloo"]) is None
    assert os.path.isdir(os.path.join(out, "ck", "launch")) and not os.listdir(os.path.join(out, "ck", "launch"))
    try:
        train_SuRS.main(flags + ["--dist_backend", "no_such_backend"])
    except SystemExit as e:
        assert "a rank ended with status" in str(e), e
    else:
        raise AssertionError("main() returned although every rank failed")
    return "main() started %d ranks and waited for them; failing ranks end it with SystemExit" % world


MODES = dict(same=mode_same, fixture=mode_fixture, odd=mode_odd, poison=mode_poison)


def worker(rank, world, port, mode, work):
    torch.cuda.set_device(0)
    if mode == "app":
        msg = mode_app(rank, world, port, work)
    else:
        import datetime
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world,
                                timeout=datetime.timedelta(seconds=120))
        try:
            msg = MODES[mode](rank, world)
        finally:
            dist.destroy_process_group()
    if rank == 0:
        print("ok: %s world %d: %s" % (mode, world, msg), flush=True)


def main():
    world, mode = int(sys.argv[1]), sys.argv[2]
    if mode not in MODES and mode not in ("app", "launch") or not 1 <= world <= 4:
        raise SystemExit(__doc__)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with tempfile.TemporaryDirectory() as work:
        if mode in ("app", "launch"):       # (host work only: this process never touches the GPU)
            import mesh_ref as mr
            import train_data_common as tdc
            torus = dict(major=0.25, minor=0.1, center=(0.0, 0.0, 0.0))
            tdc.make_dataroot(os.path.join(work, "data"), mr.torus(24, 12, **torus), mr.torus(12, 6, **torus), size=64, yaws=YAWS,
                              param=dict(ortho_ratio=1.0, scale=64.0, center=np.zeros(3), R=np.eye(3)))
        if mode == "launch":
            print("ok: launch world %d: %s" % (world, mode_launch(world, port, work)), flush=True)
            return
        mp.spawn(worker, args=(world, port, mode, work), nprocs=world, join=True)
        if mode == "app":
            done = [json.load(open(os.path.join(work, "done_%d.json" % r))) for r in range(world)]
            assert len(set(d["steps"] for d in done)) == 1 and len(set(d["digest"] for d in done)) == 1, done
            print("ok: app: every rank took %d steps and the replicas agreed (digest %d)" % (done[0]["steps"], done[0]["digest"]), flush=True)


if __name__ == "__main__":
    main()
