"""apps/train_SuRS.py on the GPU: two epochs on a synthetic dataroot (tests/train_data_common.py, the procedural meshes of
tests/mesh_ref.py; 64 x 64 renders, 200 samples, batch size 2, four yaws of the one training subject = two steps per epoch): the loss
is finite, the checkpoints load into a fresh SuRSNet with exactly the reference's keys, the PLY and OBJ files are there, the same seed
gives byte-identical checkpoints, and a resumed run starts at the right epoch from the saved weights."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_ref as mr
import train_data_common as tdc

pytestmark = pytest.mark.gpu

YAWS = (0, 1, 2, 3)
# unit-cube geometry: the dataset's calibration is then gen_mesh's own diag(2, -2, 2, 1) (scale / ortho_ratio / (loadSize / 2) = 2), the
# meshes lie inside --b_min / --b_max = -+0.5, and --z_size 12.5 gives the depth feature the scale it has at the released options.
# --no_octree: the octree's first level is a 64^3 lattice (the reference's too), so --resolution 32 needs the dense sweep.
# --learning_rate 1e-6: the seeded weights' occupancy spans about 0.2 .. 0.8 in the box; ADAM at 1e-4 moved the whole field across 0.5
# within one step (measured: hr 0.53 .. 0.97 after the first), and marching cubes then has no surface to extract
PARAM = dict(ortho_ratio=1.0, scale=64.0, center=np.zeros(3), R=np.eye(3))
TORUS = dict(major=0.25, minor=0.1, center=(0.0, 0.0, 0.0))
UNIT = ["--b_min", "-0.5", "-0.5", "-0.5", "--b_max", "0.5", "0.5", "0.5", "--sigma", "0.05", "--z_size", "12.5", "--learning_rate", "1e-6"]


def _opt(root, out, name, more=()):
    return tdc.opt(root, size=64, n=200, more=[
        "--residual", "--batch_size", "2", "--num_epoch", "2", "--resolution", "32", "--num_gen_mesh_test", "1", "--name", name,
        "--checkpoints_path", os.path.join(out, "ck"), "--results_path", os.path.join(out, "res"), "--freq_plot", "1", "--freq_save_ply", "1",
        "--seed", "5", "--no_octree"] + UNIT + list(more))


def _run(opt):
    from surs_amd import data
    from surs_amd.apps import train_SuRS
    sets = []
    for phase in ("train", "test"):
        d = data.TrainDataset(opt, phase, seed=opt.seed, images="device")
        d.yaw_list = list(YAWS)                      # (the dataroot holds these four renders per subject, not the reference's 360)
        sets.append(d)
    assert len(sets[0]) == 4 and len(sets[1]) == 4
    lines = []
    done = train_SuRS.train(opt, datasets=tuple(sets), log=lambda *a: lines.append(" ".join(str(x) for x in a)))
    return done, lines


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_two_epochs_checkpoints_resume_and_repeat(tmp_path, golden_dir):
    from surs_amd import model, native
    root = tdc.make_dataroot(tmp_path / "data", mr.torus(24, 12, **TORUS), mr.torus(12, 6, **TORUS), size=64, yaws=YAWS, param=PARAM)
    out = str(tmp_path / "out")
    opt = _opt(root, out, "a")
    done, lines = _run(opt)
    print("\n".join(l for l in lines if l.startswith("Name:")))
    assert done["first_epoch"] == 0 and done["steps"] == 4 and done["skipped"] == 0
    errs = [e for _, _, e in done["errors"]]
    assert len(errs) == 4 and all(np.isfinite(e) and e > 0 for e in errs)
    ck, res = os.path.join(out, "ck", "a"), os.path.join(out, "res", "a")
    assert sorted(os.listdir(ck)) == ["netG_epoch_0", "netG_epoch_1", "netG_latest"]
    want = [k for k, _ in json.load(open(os.path.join(golden_dir, "state_dict_keys.json")))]
    sds = {}
    for name in os.listdir(ck):
        sds[name] = torch.load(os.path.join(ck, name), map_location="cpu")
        assert list(sds[name]) == want, name
        fresh = model.SuRSNet(opt).to(device=native.require_gpu())
        fresh.load_state_dict(sds[name])             # (strict: a missing or unexpected key raises)
    # (torch.save names the archive's records after the file, so two files of one state dict differ in bytes: the tensors are compared)
    assert all(torch.equal(sds["netG_latest"][k], sds["netG_epoch_1"][k]) for k in want)
    changed = [k for k in want if not torch.equal(sds["netG_epoch_0"][k], sds["netG_epoch_1"][k])]
    assert any(k.startswith("mlp_") for k in changed) and any(k.startswith("super_resolution.") for k in changed) \
        and any(k.startswith("image_filter_lr.") for k in changed)
    files = set(os.listdir(res))
    for e in (0, 1):
        assert {"%d%s.ply" % (e, s) for s in ("pred", "pred_gt", "pred_lr")} <= files
        for phase, subject in (("test", tdc.SUBJECTS[1]), ("train", tdc.SUBJECTS[0])):
            for tag in ("HR", "LR"):
                path = os.path.join(res, "%s_eval_epoch%d_%s_%s.obj" % (phase, e, subject, tag))
                assert os.path.getsize(path) > 0, path
    assert _read(os.path.join(res, "1pred.ply")).startswith(b"ply\nformat ascii 1.0\nelement vertex 200\n")

    # the same seed again: byte-identical checkpoints
    done_b, _ = _run(_opt(root, out, "b"))
    for name in ("netG_epoch_0", "netG_epoch_1", "netG_latest"):
        assert _read(os.path.join(out, "ck", "b", name)) == _read(os.path.join(ck, name)), name
    assert done_b["errors"] == done["errors"]

    # resumed at epoch 1 with a zero learning rate: the run starts there, from netG_epoch_0's weights, and saves them back unchanged
    saved = torch.load(os.path.join(ck, "netG_epoch_0"), map_location="cpu")
    os.replace(os.path.join(ck, "netG_epoch_0"), os.path.join(ck, "netG_epoch_1"))
    done_c, lines_c = _run(_opt(root, out, "a", ["--continue_train", "0", "--resume_epoch", "1", "--learning_rate", "0", "--no_gen_mesh"]))
    assert done_c["first_epoch"] == 1 and done_c["steps"] == 2
    assert any(l.startswith("Resuming from") and l.endswith("netG_epoch_1") for l in lines_c)
    again = torch.load(os.path.join(ck, "netG_epoch_1"), map_location="cpu")
    assert all(torch.equal(saved[k], again[k]) for k in want)
