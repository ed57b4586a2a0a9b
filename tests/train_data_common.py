"""A synthetic dataroot in the layout of the reference's TrainDataset_LR_v2 (RENDER / MASK / PARAM / GEO/OBJ / val.txt), for
the training-dataset tests: seeded pixels, one subject for each phase, procedural meshes."""
import os

import numpy as np

from surs_amd import options, prng

PARAM = dict(ortho_ratio=0.4, scale=1.7, center=np.array([3.0, 100.0, -2.0]),
             R=np.array([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]]))
SUBJECTS = ("alpha", "beta")      # beta is the validation subject


def write_obj(path, v, f):
    with open(path, "w") as fh:
        fh.write("".join("v %r %r %r\n" % tuple(float(x) for x in p) for p in v))
        fh.write("".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in f))


def make_dataroot(root, mesh_hr, mesh_lr, size=64, yaws=(0,), param=PARAM):
    from PIL import Image
    root = str(root)
    for d in ("RENDER", "MASK", "PARAM"):
        for s in SUBJECTS:
            os.makedirs(os.path.join(root, d, s), exist_ok=True)
    os.makedirs(os.path.join(root, "GEO", "OBJ"), exist_ok=True)
    for k, s in enumerate(SUBJECTS):
        for yaw in yaws:
            stem = "%d_0_00" % yaw
            rgb = (prng.uniform01("train_rgb8", 1 + k + 10 * yaw, size * size * 3) * 256.0).astype(np.uint8).reshape(size, size, 3)
            mask = np.zeros((size, size), np.uint8)
            mask[size // 8: 7 * size // 8, size // 4: 3 * size // 4] = 255
            Image.fromarray(rgb).save(os.path.join(root, "RENDER", s, stem + ".png"))
            Image.fromarray(mask).save(os.path.join(root, "MASK", s, stem + ".png"))
            np.save(os.path.join(root, "PARAM", s, stem + ".npy"), param, allow_pickle=True)
        write_obj(os.path.join(root, "GEO", "OBJ", s + "_HR.obj"), *mesh_hr)
        write_obj(os.path.join(root, "GEO", "OBJ", s + "_LR.obj"), *mesh_lr)
    with open(os.path.join(root, "val.txt"), "w") as fh:
        fh.write(SUBJECTS[1] + "\n")
    return root


def opt(root, size=64, n=256, more=()):
    return options.BaseOptions().parse(["--dataroot", str(root), "--loadSize", str(size), "--num_sample_inout", str(n)] + list(more))
