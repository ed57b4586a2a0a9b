"""dist.reconstruction_sharded end to end on ONE GPU for a SurfaceClassifier shape other than the released one (s1: the fused
evaluator sweeps each rank's slab): `world` processes share cuda:0 (gloo with host staging), rank 0 compares the assembled meshes with
the single-process reconstruction - vertices and faces bit-identical - for both precisions, twice (the first reconstruction of a
workspace extracts each slab in one piece, the second pipelines the extraction into the sweep), and with want_normals=True.

    python tools/gpu_slab_check_shapes.py WORLD [R]
"""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

S1 = ["--mlp_dim_lr", "321", "512", "256", "128", "1", "--mlp_dim_hr", "322", "512", "256", "128", "1",
      "--mlp_res_layers_lr", "1", "2", "3", "--mlp_res_layers_hr", "1", "2", "3"]


def worker(rank, world, port, R):
    import common
    from surs_amd import dist as sdist, mesh_util, model, options, weights
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    fl, fh = common.synth_features()
    calib = torch.from_numpy(common.CALIB[None].copy())
    b_min, b_max = np.array([-0.55] * 3), np.array([0.55] * 3)   # (past the image: the masked zeros close the surface)
    for prec in ("fp32", "bf16"):
        opt = options.BaseOptions().parse(common.FLAGS + S1 + ["--precision", prec])
        sd = weights.synthetic_state_dict(opt, seed=0)

        def make():
            net = model.SuRSNet(opt).to(device=dev)
            net.load_state_dict(sd)
            net.eval()
            net.im_feat_list_lr = [torch.from_numpy(fl[None]).to(dev)]
            net.im_feat_list_hr = [torch.from_numpy(fh[None]).to(dev)]
            assert net.generic_mlp() is not None
            return net
        net = make()
        ref = None
        if rank == 0:
            ref = mesh_util.reconstruction(opt, make(), dev, calib, R, b_min, b_max, use_octree=False, want_normals=False)
        for it in range(2):
            got = sdist.reconstruction_sharded(opt, net, calib, R, b_min, b_max)
            if rank == 0:
                ok = all(np.array_equal(got[i], ref[i]) and got[i].dtype == ref[i].dtype for i in (0, 1, 4, 5))
                print("%s world %d R %d pass %d: %s  (%d / %d vertices, %d / %d faces)" %
                      (prec, world, R, it, "slab == one piece" if ok else "MISMATCH", len(got[0]), len(got[4]), len(got[1]), len(got[5])),
                      flush=True)
            else:
                assert got is None
        got = sdist.reconstruction_sharded(opt, net, calib, R, b_min, b_max, want_normals=True)
        if rank == 0:
            refn = mesh_util.reconstruction(opt, make(), dev, calib, R, b_min, b_max, use_octree=False, want_normals=True)
            ok = all(np.array_equal(got[i], refn[i]) for i in (0, 1, 3, 4, 5, 7))                      # vertices, faces, values
            ok = ok and all(np.abs(got[i] - refn[i]).max() < 1e-4 for i in (2, 6))                      # normals: float atomics
            print("%s normals world %d R %d: %s" % (prec, world, R, "slab == one piece" if ok else "MISMATCH"), flush=True)
        else:
            assert got is None
    dist.destroy_process_group()


def main():
    world = int(sys.argv[1])
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    mp.spawn(worker, args=(world, port, R), nprocs=world, join=True)


if __name__ == "__main__":
    main()
