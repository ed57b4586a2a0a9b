"""Render a folder of textured scans into the dataroot data.TrainDataset reads - on the device, PRT lighting, no OpenGL.

    python -m surs_amd.apps.render_data -i SCAN_DIR -o DATAROOT [--size 512] [--yaws 0:360:1] [--pitch 0] [--ms_rate 2]
        [--n_prt 40] [--env_sh FILE.npy] [--seed S] [--prt_cache DIR] [--device cuda:0|cpu]

A subject is SCAN_DIR/<name>.obj or SCAN_DIR/<name>/<name>.obj (one material, with texture coordinates) with its texture beside it
(<name>.jpg / .jpeg / .png, or the only image in a folder of its own).  Written per subject and view:

    DATAROOT/RENDER/<name>/<yaw>_<pitch>_00.jpg     DATAROOT/MASK/<name>/<yaw>_<pitch>_00.png
    DATAROOT/PARAM/<name>/<yaw>_<pitch>_00.npy      {'ortho_ratio', 'scale', 'center', 'R', 'sh'}
    DATAROOT/GEO/OBJ/<name>_HR.obj                  a copy of the scan

<name>_LR.obj - a decimated scan - is the user's to make: one lying beside the scan is copied, otherwise one line says which file
training will miss.  A view whose three files exist is skipped, so an interrupted run is resumed by running it again.  The
subject's PRT is computed once (and kept under --prt_cache).  --device cpu runs the library's host twins: the same bytes, slowly."""
import argparse
import os
import shutil
import sys
import time

import numpy as np

from .. import render

_IMAGES = (".jpg", ".jpeg", ".png")


def parse_yaws(text):
    """'a:b:c' (range(a, b, c)), 'a:b', or a comma-separated list."""
    if ":" in text:
        part = [int(x) for x in text.split(":")]
        if len(part) not in (2, 3) or (len(part) == 3 and part[2] <= 0):
            raise argparse.ArgumentTypeError("--yaws %r: start:stop[:step] with a positive step is needed" % text)
        return list(range(*part))
    return [int(x) for x in text.split(",") if x]


def find_subjects(scan_dir):
    """[(name, obj_path)] sorted by name: <name>.obj in scan_dir or in scan_dir/<name>/ (files ending in _LR.obj are not subjects)."""
    found = {}
    for entry in sorted(os.listdir(scan_dir)):
        path = os.path.join(scan_dir, entry)
        if os.path.isdir(path):
            inner = os.path.join(path, entry + ".obj")
            if os.path.isfile(inner):
                found.setdefault(entry, inner)
        elif entry.endswith(".obj") and not entry.endswith("_LR.obj"):
            found.setdefault(entry[:-4], path)
    return sorted(found.items())


def find_texture(obj_path, name):
    folder = os.path.dirname(obj_path)
    for ext in _IMAGES:
        if os.path.isfile(os.path.join(folder, name + ext)):
            return os.path.join(folder, name + ext)
    images = [f for f in sorted(os.listdir(folder)) if f.lower().endswith(_IMAGES)]
    objs = [f for f in os.listdir(folder) if f.endswith(".obj") and not f.endswith("_LR.obj")]
    if len(images) == 1 and len(objs) == 1:
        return os.path.join(folder, images[0])
    raise SystemExit("%s: no texture %s.{jpg,jpeg,png} beside it" % (obj_path, name))


def load_texture(path):
    """uint8 [h, w, 3] with sides that are multiples of 8 (an image of other sides is resized down to the next ones, bilinear)."""
    from PIL import Image
    img = Image.open(path).convert("RGB")
    w, h = img.size
    w8, h8 = max(8, w // 8 * 8), max(8, h // 8 * 8)
    if (w8, h8) != (w, h):
        print("%s: %d x %d resized to %d x %d (texture sides must be multiples of 8)" % (path, w, h, w8, h8))
        img = img.resize((w8, h8), Image.BILINEAR)
    return np.ascontiguousarray(np.asarray(img, np.uint8))


def view_done(root, name, yaw, pitch):
    return all(os.path.isfile(p) for p in render.view_paths(root, name, yaw, pitch))


def light_seed(seed, sid, yaw, pitch):
    return (int(seed) * 1000003 + sid * 7919 + int(yaw) * 31 + int(pitch)) & (2 ** 63 - 1)


def subject_prt(sub, name, args):
    dirs = render.prt_directions(args.n_prt, args.seed)
    cache = os.path.join(args.prt_cache, "%s_n%d_s%d.npy" % (name, args.n_prt, args.seed)) if args.prt_cache else None
    nv = len(sub.normals)
    if cache and os.path.isfile(cache):
        prt = np.load(cache)
        if prt.shape == (nv, 9) and prt.dtype == np.float32:
            return prt
        print("%s: %s does not fit the scan (%s); computed again" % (name, cache, prt.shape))
    t0 = time.time()
    prt = sub.prt(dirs)
    prt = prt if isinstance(prt, np.ndarray) else prt.cpu().numpy()
    print("%s: PRT of %d vertices x %d directions in %.1f s" % (name, nv, len(dirs), time.time() - t0))
    if cache:
        os.makedirs(args.prt_cache, exist_ok=True)
        np.save(cache, prt)
    return prt


def render_subject(sid, name, obj_path, args):
    """Render what is missing of one subject; returns the number of views written."""
    root = args.output
    todo = [y for y in args.yaws if not view_done(root, name, y, args.pitch)]
    os.makedirs(os.path.join(root, "GEO", "OBJ"), exist_ok=True)
    hr = os.path.join(root, "GEO", "OBJ", name + "_HR.obj")
    if not os.path.isfile(hr):
        shutil.copyfile(obj_path, hr)
    lr_src, lr = obj_path[:-4] + "_LR.obj", os.path.join(root, "GEO", "OBJ", name + "_LR.obj")
    if os.path.isfile(lr_src):
        if not os.path.isfile(lr):
            shutil.copyfile(lr_src, lr)
    elif not os.path.isfile(lr):
        print("%s: no %s beside the scan - training will miss %s (a decimated scan; make it and put it there)" % (name, lr_src, lr))
    if not todo:
        return 0
    mesh = render.load_textured_obj(obj_path)
    sub = render.Subject(mesh, load_texture(find_texture(obj_path, name)), args.device)
    prt = subject_prt(sub, name, args)
    center, scale = render.subject_frame(mesh[0])
    env = np.load(args.env_sh) if args.env_sh else None
    for k in range(0, len(todo), args.batch):
        yaws = todo[k:k + args.batch]
        params = [render.view_param(y, args.pitch, args.size, center, scale)[0] for y in yaws]
        lights = np.stack([render.sample_light(light_seed(args.seed, sid, y, args.pitch), env) for y in yaws])
        images, masks = render.render_views(sub, None, prt, params, lights, args.size, ms=args.ms_rate)
        for y, image, mask, param, light in zip(yaws, images, masks, params, lights):
            render.write_view(root, name, y, args.pitch, image, mask, param, light)
    return len(todo)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-i", "--input", required=True, help="folder of scans")
    ap.add_argument("-o", "--output", required=True, help="dataroot to write")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--yaws", type=parse_yaws, default=list(range(0, 360, 1)))
    ap.add_argument("--pitch", type=int, default=0)
    ap.add_argument("--ms_rate", type=int, default=2, help="sub-samples along a pixel's side (1 .. 8)")
    ap.add_argument("--n_prt", type=int, default=40, help="n x n PRT directions")
    ap.add_argument("--env_sh", default=None, help=".npy of [K, 9, 3] environment lights")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--prt_cache", default=None, help="folder that keeps each subject's PRT")
    ap.add_argument("--device", default="cuda:0", help="cuda:N, or cpu for the host twins")
    ap.add_argument("--batch", type=int, default=36, help="views rendered between two writes")
    args = ap.parse_args(argv)
    if not 1 <= args.ms_rate <= 8 or args.size < 2 or args.size % 2:
        raise SystemExit("--ms_rate must be in 1 .. 8 and --size an even number")
    subjects = find_subjects(args.input)
    if not subjects:
        raise SystemExit("%s: no <name>.obj found" % args.input)
    total = 0
    for sid, (name, obj_path) in enumerate(subjects):
        t0 = time.time()
        n = render_subject(sid, name, obj_path, args)
        total += n
        print("%s: %d views written, %d already there (%.1f s)" % (name, n, len(args.yaws) - n, time.time() - t0))
    return total


if __name__ == "__main__":
    main(sys.argv[1:])
