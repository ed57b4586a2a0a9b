"""Input stage of the test path: the output contract of the reference's EvalDataset_LR_v2
(/root/reference/lib/data/EvalDataset_LR_v2.py:134-180,185-254,389-410):

    dataroot/image_final/<subject>.{jpg,png}   RGB image
    dataroot/mask_final/<subject>.{png,jpg}    8-bit mask
    item = {'name': (stem, ext), 'b_min', 'b_max', 'img_LR': [V,3,H,W] float32 = mask * ((rgb/255 - 0.5)/0.5),
            'calib': [V,4,4] diag(2,-2,2,1)}

File decoding (PIL) stays on the host.  `get_render` is the plain host statement of the contract (numpy); the serving path
(`get_raw` + `DeviceInputStage`, used by train_util.gen_mesh_pipelined) uploads the decoded uint8 pixels and does ToTensor +
Normalize + mask multiply in one kernel (surs_image_prepare): the same float32 operations, bit-identical img_LR, written
straight into the encoder's NHWC layout.  No resizing at eval, exactly as the reference.
"""
import os

import numpy as np
import torch


class EvalDataset:
    def __init__(self, opt, phase="test"):
        self.opt = opt
        self.projection_mode = "orthogonal"
        self.root = opt.dataroot
        self.RENDER = os.path.join(self.root, "image_final")
        self.MASK = os.path.join(self.root, "mask_final")
        self.B_MIN = np.array(opt.b_min, dtype=float)
        self.B_MAX = np.array(opt.b_max, dtype=float)
        self.is_train = phase == "train"
        self.num_views = opt.num_views
        self.subjects = sorted(os.listdir(self.RENDER))

    def __len__(self):
        return len(self.subjects)

    @staticmethod
    def _first_existing(*paths):
        for p in paths:
            if os.path.isfile(p):
                return p
        return paths[-1]

    def get_raw(self, subject):
        """Decoded pixels only: (rgb uint8 [H,W,3], mask uint8 [H,W])."""
        from PIL import Image
        render_path = self._first_existing(os.path.join(self.RENDER, subject + ".jpg"), os.path.join(self.RENDER, subject + ".png"))
        mask_path = self._first_existing(os.path.join(self.MASK, subject + ".png"), os.path.join(self.MASK, subject + ".jpg"))
        return (np.ascontiguousarray(np.asarray(Image.open(render_path).convert("RGB"), np.uint8)),
                np.ascontiguousarray(np.asarray(Image.open(mask_path).convert("L"), np.uint8)))

    def get_raw_item(self, index):
        """What gen_mesh_pipelined consumes: the item without its tensors, plus the decoded pixels."""
        subject = os.path.splitext(self.subjects[index])
        rgb, mask = self.get_raw(subject[0])
        return {"name": subject, "b_min": self.B_MIN, "b_max": self.B_MAX, "rgb": rgb, "mask": mask}

    def get_render(self, subject):
        rgb8, mask8 = self.get_raw(subject)
        mask = mask8.astype(np.float32) / np.float32(255.0)        # ToTensor
        rgb = rgb8.astype(np.float32) / np.float32(255.0)
        rgb = (rgb - np.float32(0.5)) / np.float32(0.5)                                               # Normalize(0.5, 0.5)
        img = np.ascontiguousarray((mask[None] * rgb.transpose(2, 0, 1)).astype(np.float32))
        calib = np.identity(4, np.float32) * 2
        calib[1, 1] = -2
        calib[3, 3] = 1
        # the reference repeats the same file for every view (get_render loops over view ids but ignores them)
        v = self.num_views
        return {"img_LR": torch.from_numpy(np.stack([img] * v, 0)), "calib": torch.from_numpy(np.stack([calib] * v, 0))}

    def get_item(self, index):
        subject = os.path.splitext(self.subjects[index])
        res = {"name": subject, "b_min": self.B_MIN, "b_max": self.B_MAX}
        res.update(self.get_render(subject[0]))
        return res

    def __getitem__(self, index):
        return self.get_item(index)


class DeviceInputStage:
    """uint8 pixels -> img_LR on the device: pinned staging buffers (reused), asynchronous upload and surs_image_prepare on the
    current stream.  Returns a [1,3,H,W] float32 tensor (channels_last strides: the encoder takes it without a copy) holding
    exactly the bytes of the reference's img_LR."""

    def __init__(self, device):
        self.device = device
        self._pin = {}

    def _staged(self, key, a):
        ent = self._pin.get((key, a.shape))
        if ent is None:
            ent = self._pin[(key, a.shape)] = [torch.empty(a.shape, dtype=torch.uint8, pin_memory=True), None]
        buf, uploaded = ent
        if uploaded is not None:
            uploaded.synchronize()   # the previous subject's upload has read the buffer: only now may the host overwrite it
        buf.numpy()[...] = a
        d = buf.to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        ent[1] = ev
        return d

    def prepare(self, rgb, mask):
        from . import native
        h, w = mask.shape
        assert rgb.shape == (h, w, 3) and rgb.dtype == np.uint8 and mask.dtype == np.uint8
        d_rgb, d_mask = self._staged("rgb", rgb), self._staged("mask", mask)
        out = torch.empty((1, h, w, 3), dtype=torch.float32, device=self.device)
        native.check(native.lib().surs_image_prepare(native._ptr(d_rgb), native._ptr(d_mask), h, w, native._ptr(out), 3, native._stream()))
        return out.permute(0, 3, 1, 2)


JITTER_OPTIONS = ("aug_bri", "aug_con", "aug_sat", "aug_hue")


def jitter_params(opt):
    """torchvision's ColorJitter.get_params for --aug_bri / --aug_con / --aug_sat / --aug_hue, drawn from torch's global generator:
    (order, b, c, s, h).  First order = torch.randperm(4); then, in the order brightness, contrast, saturation, hue, one
    float(torch.empty(1).uniform_(lo, hi)) for each op whose amount a is non-zero - [max(0, 1 - a), 1 + a] for the first three,
    [-a, a] for hue -; an op with amount 0 draws nothing and is None (skipped).  The ops are applied in `order` (0 brightness,
    1 contrast, 2 saturation, 3 hue).  0 <= a <= 0.5."""
    amounts = [float(getattr(opt, k, 0.0) or 0.0) for k in JITTER_OPTIONS]
    for k, a in zip(JITTER_OPTIONS, amounts):
        if not 0.0 <= a <= 0.5:
            raise ValueError("--%s %g: an amount in [0, 0.5] is needed" % (k, a))
    order = tuple(int(i) for i in torch.randperm(4))
    vals = []
    for k, a in enumerate(amounts):
        if a == 0.0:
            vals.append(None)
            continue
        lo, hi = (-a, a) if k == 3 else (max(0.0, 1.0 - a), 1.0 + a)
        vals.append(float(torch.empty(1).uniform_(lo, hi)))
    return (order,) + tuple(vals)


class TrainImageStage:
    """Decoded uint8 pixels of one view -> (img_HR [3,H,W], img_LR [3,H/2,W/2]) float32 through native.train_images: NHWC in
    memory, NCHW-shaped views, as DeviceInputStage gives them.  Pixels and the plan's tables go through pinned staging buffers
    (reused, grown on demand) and asynchronous uploads on the current stream; the workspace is reused.  device=None runs the host
    twins and returns host tensors."""

    def __init__(self, device):
        self.device = device
        self._pin = {}
        self._ws = None

    def _staged(self, key, a):
        a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        ent = self._pin.get(key)
        if ent is None or ent[0].numel() < a.size:
            if ent is not None and ent[1] is not None:
                ent[1].synchronize()
            ent = self._pin[key] = [torch.empty(max(a.size, 1), dtype=torch.uint8, pin_memory=True), None]
        buf, uploaded = ent
        if uploaded is not None:
            uploaded.synchronize()   # the previous view's upload has read the buffer: only now may the host overwrite it
        buf.numpy()[:a.size] = a
        d = buf[:a.size].to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        ent[1] = ev
        return d

    def empty(self, shape):
        """An uninitialised float32 tensor where run() writes: on the stage's device, or on the host."""
        return torch.empty(shape, dtype=torch.float32, device=self.device if self.device is not None else "cpu")

    def run(self, plan, rgb, mask, out=None):
        """out: (img_hr [H,W,3], img_lr [H/2,W/2,3]) contiguous float32 tensors to write into, e.g. one view's slices of an item's
        [V,H,W,3] tensors; they are returned as the [3,H,W] views."""
        from . import native
        if out is None:
            h, w = plan.size
            out = (self.empty((h, w, 3)), self.empty((h // 2, w // 2, 3)))
        if self.device is None:
            native.train_images(plan, rgb, mask, host=True, out=(out[0].numpy(), out[1].numpy()))
            return out[0].permute(2, 0, 1), out[1].permute(2, 0, 1)
        h, w = mask.shape
        assert rgb.shape == (h, w, 3) and rgb.dtype == np.uint8 and mask.dtype == np.uint8
        d_rgb, d_mask = self._staged("rgb", rgb).view(h, w, 3), self._staged("mask", mask).view(h, w)
        d_tables = self._staged("tables", plan.tables)
        nbytes = native.lib().surs_train_images_workspace_bytes(plan.plan)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        native.train_images(plan, d_rgb, d_mask, tables=d_tables, workspace=self._ws, out=out)
        return out[0].permute(2, 0, 1), out[1].permute(2, 0, 1)


class SyntheticDataset:
    """Stand-in with the same item contract when there is no dataroot (--synthetic): seeded images."""

    def __init__(self, opt, n=1, size=None):
        from . import weights
        self.opt, self.n, self.projection_mode = opt, n, "orthogonal"
        self.size = size or opt.loadSize // 2
        self._w = weights

    def __len__(self):
        return self.n

    def get_raw_item(self, i):
        """8-bit pixels of a seeded image + the rectangular mask (the decoded form of an input pair)."""
        from . import prng
        s = self.size
        rgb = (prng.uniform01("synthetic_rgb8", 1 + i, s * s * 3) * 256.0).astype(np.uint8).reshape(s, s, 3)
        mask = np.zeros((s, s), np.uint8)
        mask[s // 8: 7 * s // 8, s // 4: 3 * s // 4] = 255
        return {"name": ("synthetic_%04d" % i, ".png"), "b_min": np.array(self.opt.b_min, dtype=float),
                "b_max": np.array(self.opt.b_max, dtype=float), "rgb": rgb, "mask": mask}

    def __getitem__(self, i):
        calib = np.identity(4, np.float32) * 2
        calib[1, 1] = -2
        calib[3, 3] = 1
        return {"name": ("synthetic_%04d" % i, ".png"), "b_min": np.array(self.opt.b_min, dtype=float),
                "b_max": np.array(self.opt.b_max, dtype=float),
                "img_LR": torch.from_numpy(self._w.synthetic_image(self.size, seed=1 + i)), "calib": torch.from_numpy(calib[None])}


def param_calib(param, load_size):
    """(calib, extrinsic) float32 [4,4] of a PARAM dict as TrainDataset.get_render forms them without augmentation (phase 'test'):
    the same expressions in the same order, for whoever WRITES a dataroot (render.view_param) - tests/test_render_host.py holds the
    two to each other bit for bit."""
    ortho_ratio, scale, center, R = param.get("ortho_ratio"), param.get("scale"), param.get("center"), param.get("R")
    half = float(load_size // 2)
    translate = -np.matmul(R, center).reshape(3, 1)
    extrinsic = np.concatenate([R, translate], axis=1)
    extrinsic = np.concatenate([extrinsic, np.array([0, 0, 0, 1]).reshape(1, 4)], 0)
    scale_intrinsic = np.identity(4)
    scale_intrinsic[0, 0] = scale / ortho_ratio
    scale_intrinsic[1, 1] = -scale / ortho_ratio
    scale_intrinsic[2, 2] = scale / ortho_ratio
    uv_intrinsic = np.identity(4)
    uv_intrinsic[0, 0] = uv_intrinsic[1, 1] = uv_intrinsic[2, 2] = 1.0 / half
    trans_intrinsic = np.identity(4)
    intrinsic = np.matmul(trans_intrinsic, np.matmul(uv_intrinsic, scale_intrinsic))
    return np.matmul(intrinsic, extrinsic).astype(np.float32), extrinsic.astype(np.float32)


class TrainDataset:
    """The item contract of the reference's TrainDataset_LR_v2 (lib/data/TrainDataset_LR_v2.py):

        dataroot/RENDER/<subject>/<yaw>_<pitch>_00.{jpg,png}   dataroot/MASK/<subject>/<yaw>_<pitch>_00.{png,jpg}
        dataroot/PARAM/<subject>/<yaw>_<pitch>_00.npy          {'ortho_ratio', 'scale', 'center', 'R'}
        dataroot/GEO/OBJ/<subject>_HR.obj, <subject>_LR.obj     dataroot/val.txt
        item = {'name', 'mesh_path_HR', 'mesh_path_LR', 'sid', 'yid', 'pid', 'b_min', 'b_max',
                'img_LR' [V,3,H/2,W/2], 'img_HR' [V,3,H,W], 'calib' [V,4,4], 'extrinsic' [V,4,4]            (host tensors)
                'samples_HR' [3,N], 'samples_LR' [3,N], 'labels_HR' [1,N], 'labels_disp' [1,N]}              (DEVICE tensors)

    get_render is PIL and numpy on the host and draws from `random` / `np.random` exactly where the reference does (lines
    194-355); torchvision's ColorJitter is not available: a non-zero --aug_bri / --aug_con / --aug_sat / --aug_hue raises.
    select_sampling_method runs on the device (native.mesh_sample_pool, two native.mesh_contains, native.sample_select): the
    pool comes from the package's counter PRNG, not from numpy's generator, and inside / outside is the winding number's
    answer.  Meshes are parsed and uploaded once per subject, at their first use.  Phase 'test' draws every item's samples
    from seed 1991 (the reference re-seeds with 1991 before each item); phase 'train' derives the seed from (seed, index, how
    many items this object has drawn).  The samples are made on the GPU of the calling process, so the dataset refuses to run
    in a DataLoader worker: use --num_threads 0.  get_color_sampling is not built (SuRS trains with --num_sample_color 0).

    images=None is the PIL path above.  images='device' builds img_LR / img_HR on the device from the decoded pixels
    (native.train_images through a TrainImageStage: DEVICE tensors, NHWC in memory, NCHW-shaped), images='cpu' through the same
    chain's host twins (host tensors); both take the colour jitter, drawn by jitter_params, and with jitter 0 give the bits of the
    PIL path for the same `random` / `np.random` state."""

    _JITTER = JITTER_OPTIONS
    TEST_SEED = 1991

    def __init__(self, opt, phase="train", seed=0, images=None):
        if images not in (None, "device", "cpu"):
            raise ValueError("images=%r: None (PIL on the host), 'device' or 'cpu' (the native chain) is needed" % (images,))
        for k in self._JITTER:
            if images is None and float(getattr(opt, k, 0.0)) != 0.0:
                raise NotImplementedError("--%s %g: colour jitter (torchvision ColorJitter) is not built; only 0 is accepted"
                                          % (k, getattr(opt, k)))
        self.images = images
        self._stage = None
        self.opt = opt
        self.projection_mode = "orthogonal"
        self.root = opt.dataroot
        self.RENDER = os.path.join(self.root, "RENDER")
        self.MASK = os.path.join(self.root, "MASK")
        self.PARAM = os.path.join(self.root, "PARAM")
        self.OBJ = os.path.join(self.root, "GEO", "OBJ")
        self.B_MIN = np.array(opt.b_min, dtype=float)
        self.B_MAX = np.array(opt.b_max, dtype=float)
        self.is_train = phase == "train"
        self.load_size = opt.loadSize
        self.num_views = opt.num_views
        self.num_sample_inout = opt.num_sample_inout
        self.num_sample_color = opt.num_sample_color
        self.yaw_list = list(range(0, 360, 1))
        self.pitch_list = [0]
        self.subjects = self.get_subjects()
        self.seed = int(seed)
        self.draws = 0
        self._meshes = {}

    def get_subjects(self):
        all_subjects = os.listdir(self.RENDER)
        var_subjects = np.atleast_1d(np.loadtxt(os.path.join(self.root, "val.txt"), dtype=str))
        if len(var_subjects) == 0:
            return all_subjects
        if self.is_train:
            return sorted(list(set(all_subjects) - set(var_subjects)))
        return sorted(list(var_subjects))

    def __len__(self):
        return len(self.subjects) * len(self.yaw_list) * len(self.pitch_list)

    @staticmethod
    def _to_tensor(img):
        """transforms.ToTensor: [C,H,W] float32 in [0, 1]."""
        a = np.asarray(img, np.uint8)
        a = a[None] if a.ndim == 2 else a.transpose(2, 0, 1)
        return np.ascontiguousarray(a).astype(np.float32) / np.float32(255.0)

    def get_render(self, subject, num_views, yid=0, pid=0, random_sample=False):
        import random
        from PIL import Image, ImageOps
        from PIL.ImageFilter import GaussianBlur
        if self.images is not None:
            return self._get_render_native(subject, num_views, yid, pid, random_sample)
        pitch = self.pitch_list[pid]
        view_ids = [self.yaw_list[(yid + len(self.yaw_list) // num_views * offset) % len(self.yaw_list)] for offset in range(num_views)]
        if random_sample:
            view_ids = np.random.choice(self.yaw_list, num_views, replace=False)
        half = float(self.opt.loadSize // 2)
        out = {"img_LR": [], "img_HR": [], "calib": [], "extrinsic": []}
        for vid in view_ids:
            stem = "%d_%d_%02d" % (vid, pitch, 0)
            param_path = os.path.join(self.PARAM, subject, stem + ".npy")
            render_path = EvalDataset._first_existing(os.path.join(self.RENDER, subject, stem + ".jpg"),
                                                      os.path.join(self.RENDER, subject, stem + ".png"))
            mask_path = EvalDataset._first_existing(os.path.join(self.MASK, subject, stem + ".png"),
                                                    os.path.join(self.MASK, subject, stem + ".jpg"))
            param = np.load(param_path, allow_pickle=True).item()
            ortho_ratio, scale, center, R = param.get("ortho_ratio"), param.get("scale"), param.get("center"), param.get("R")
            translate = -np.matmul(R, center).reshape(3, 1)
            extrinsic = np.concatenate([R, translate], axis=1)
            extrinsic = np.concatenate([extrinsic, np.array([0, 0, 0, 1]).reshape(1, 4)], 0)
            scale_intrinsic = np.identity(4)            # camera space -> image pixel space
            scale_intrinsic[0, 0] = scale / ortho_ratio
            scale_intrinsic[1, 1] = -scale / ortho_ratio
            scale_intrinsic[2, 2] = scale / ortho_ratio
            uv_intrinsic = np.identity(4)               # image pixel space -> uv space
            uv_intrinsic[0, 0] = uv_intrinsic[1, 1] = uv_intrinsic[2, 2] = 1.0 / half
            trans_intrinsic = np.identity(4)
            mask_HR = Image.open(mask_path).convert("L")
            render_HR = Image.open(render_path).convert("RGB")
            if self.is_train:
                pad_size = int(0.1 * self.load_size)
                render_HR = ImageOps.expand(render_HR, pad_size, fill=0)
                mask_HR = ImageOps.expand(mask_HR, pad_size, fill=0)
                w, h = render_HR.size
                th, tw = self.load_size, self.load_size
                if self.opt.random_flip and np.random.rand() > 0.5:
                    scale_intrinsic[0, 0] *= -1
                    render_HR = render_HR.transpose(Image.FLIP_LEFT_RIGHT)
                    mask_HR = mask_HR.transpose(Image.FLIP_LEFT_RIGHT)
                if self.opt.random_scale:
                    rand_scale = random.uniform(0.9, 1.1)
                    w = int(rand_scale * w)
                    h = int(rand_scale * h)
                    render_HR = render_HR.resize((w, h), Image.BILINEAR)
                    mask_HR = mask_HR.resize((w, h), Image.NEAREST)
                    scale_intrinsic *= rand_scale
                    scale_intrinsic[3, 3] = 1
                if self.opt.random_trans:
                    dx = random.randint(-int(round((w - tw) / 10.)), int(round((w - tw) / 10.)))
                    dy = random.randint(-int(round((h - th) / 10.)), int(round((h - th) / 10.)))
                else:
                    dx = dy = 0
                trans_intrinsic[0, 3] = -dx / half
                trans_intrinsic[1, 3] = -dy / half
                x1 = int(round((w - tw) / 2.)) + dx
                y1 = int(round((h - th) / 2.)) + dy
                render_HR = render_HR.crop((x1, y1, x1 + tw, y1 + th))
                mask_HR = mask_HR.crop((x1, y1, x1 + tw, y1 + th))
                # (aug_trans: ColorJitter with all four amounts 0 is the identity; anything else was refused in __init__)
                if self.opt.aug_blur > 0.00001:
                    render_HR = render_HR.filter(GaussianBlur(np.random.uniform(0, self.opt.aug_blur)))
            intrinsic = np.matmul(trans_intrinsic, np.matmul(uv_intrinsic, scale_intrinsic))
            calib = np.matmul(intrinsic, extrinsic).astype(np.float32)
            mask_LR = mask_HR.resize([x // 2 for x in mask_HR.size], Image.NEAREST)
            render_LR = render_HR.resize([x // 2 for x in render_HR.size], Image.BICUBIC)
            pair = []
            for mask, render in ((mask_LR, render_LR), (mask_HR, render_HR)):
                m = self._to_tensor(mask)
                r = (self._to_tensor(render) - np.float32(0.5)) / np.float32(0.5)     # Normalize(0.5, 0.5)
                pair.append(torch.from_numpy(np.ascontiguousarray(m * r)))
            out["img_LR"].append(pair[0])
            out["img_HR"].append(pair[1])
            out["calib"].append(torch.from_numpy(calib))
            out["extrinsic"].append(torch.from_numpy(extrinsic.astype(np.float32)))
        return {k: torch.stack(v, dim=0) for k, v in out.items()}

    def _get_render_native(self, subject, num_views, yid=0, pid=0, random_sample=False):
        """get_render with images='device' / 'cpu': PIL decodes the files and nothing else; the draws from `random` / `np.random`
        are get_render's, same calls in the same order, the colour jitter's are jitter_params' (torch's generator, where the
        reference calls aug_trans); the pixel work is native.train_images through a TrainImageStage."""
        import random
        from PIL import Image
        from . import native
        if self._stage is None:
            self._stage = TrainImageStage(native.require_gpu() if self.images == "device" else None)
        pitch = self.pitch_list[pid]
        view_ids = [self.yaw_list[(yid + len(self.yaw_list) // num_views * offset) % len(self.yaw_list)] for offset in range(num_views)]
        if random_sample:
            view_ids = np.random.choice(self.yaw_list, num_views, replace=False)
        half = float(self.opt.loadSize // 2)
        out = {"calib": [], "extrinsic": []}
        img_hr = img_lr = None
        for vid in view_ids:
            stem = "%d_%d_%02d" % (vid, pitch, 0)
            param_path = os.path.join(self.PARAM, subject, stem + ".npy")
            render_path = EvalDataset._first_existing(os.path.join(self.RENDER, subject, stem + ".jpg"),
                                                      os.path.join(self.RENDER, subject, stem + ".png"))
            mask_path = EvalDataset._first_existing(os.path.join(self.MASK, subject, stem + ".png"),
                                                    os.path.join(self.MASK, subject, stem + ".jpg"))
            param = np.load(param_path, allow_pickle=True).item()
            ortho_ratio, scale, center, R = param.get("ortho_ratio"), param.get("scale"), param.get("center"), param.get("R")
            translate = -np.matmul(R, center).reshape(3, 1)
            extrinsic = np.concatenate([R, translate], axis=1)
            extrinsic = np.concatenate([extrinsic, np.array([0, 0, 0, 1]).reshape(1, 4)], 0)
            scale_intrinsic = np.identity(4)
            scale_intrinsic[0, 0] = scale / ortho_ratio
            scale_intrinsic[1, 1] = -scale / ortho_ratio
            scale_intrinsic[2, 2] = scale / ortho_ratio
            uv_intrinsic = np.identity(4)
            uv_intrinsic[0, 0] = uv_intrinsic[1, 1] = uv_intrinsic[2, 2] = 1.0 / half
            trans_intrinsic = np.identity(4)
            mask8 = np.ascontiguousarray(np.asarray(Image.open(mask_path).convert("L"), np.uint8))
            rgb8 = np.ascontiguousarray(np.asarray(Image.open(render_path).convert("RGB"), np.uint8))
            if mask8.shape != rgb8.shape[:2]:
                raise ValueError("%s is %s and %s is %s: a render and its mask must have one size"
                                 % (render_path, rgb8.shape[:2], mask_path, mask8.shape))
            if self.is_train:
                pad_size = int(0.1 * self.load_size)
                w, h = rgb8.shape[1] + 2 * pad_size, rgb8.shape[0] + 2 * pad_size
                th, tw = self.load_size, self.load_size
                flip = bool(self.opt.random_flip and np.random.rand() > 0.5)
                if flip:
                    scale_intrinsic[0, 0] *= -1
                if self.opt.random_scale:
                    rand_scale = random.uniform(0.9, 1.1)
                    w = int(rand_scale * w)
                    h = int(rand_scale * h)
                    scale_intrinsic *= rand_scale
                    scale_intrinsic[3, 3] = 1
                if self.opt.random_trans:
                    dx = random.randint(-int(round((w - tw) / 10.)), int(round((w - tw) / 10.)))
                    dy = random.randint(-int(round((h - th) / 10.)), int(round((h - th) / 10.)))
                else:
                    dx = dy = 0
                trans_intrinsic[0, 3] = -dx / half
                trans_intrinsic[1, 3] = -dy / half
                x1 = int(round((w - tw) / 2.)) + dx
                y1 = int(round((h - th) / 2.)) + dy
                jitter = jitter_params(self.opt)
                blur = np.random.uniform(0, self.opt.aug_blur) if self.opt.aug_blur > 0.00001 else 0.0
                plan = native.train_image_plan(mask8.shape, pad=pad_size, flip=flip, full=(h, w), window=(x1, y1, tw, th), jitter=jitter,
                                               blur=blur)
            else:
                plan = native.train_image_plan(mask8.shape, augment=False)
            intrinsic = np.matmul(trans_intrinsic, np.matmul(uv_intrinsic, scale_intrinsic))
            calib = np.matmul(intrinsic, extrinsic).astype(np.float32)
            if img_hr is None:   # [V,H,W,3] and [V,H/2,W/2,3]: every view is written into its slice, NHWC in memory
                h_hr, w_hr = plan.size
                img_hr = self._stage.empty((len(view_ids), h_hr, w_hr, 3))
                img_lr = self._stage.empty((len(view_ids), h_hr // 2, w_hr // 2, 3))
            elif plan.size != tuple(img_hr.shape[1:3]):
                raise ValueError("%s makes an image of %s, the views before it one of %s" % (render_path, plan.size, tuple(img_hr.shape[1:3])))
            self._stage.run(plan, rgb8, mask8, out=(img_hr[len(out["calib"])], img_lr[len(out["calib"])]))
            out["calib"].append(torch.from_numpy(calib))
            out["extrinsic"].append(torch.from_numpy(extrinsic.astype(np.float32)))
        res = {"img_LR": img_lr.permute(0, 3, 1, 2), "img_HR": img_hr.permute(0, 3, 1, 2)}
        res.update({k: torch.stack(v, dim=0) for k, v in out.items()})
        return res

    def item_seed(self, index=0):
        """The counter PRNG's seed of the next item's samples."""
        if not self.is_train:
            return self.TEST_SEED
        from . import prng
        return int(prng.bits64("train_item_%d_%d" % (self.seed, int(index)), self.draws, 1)[0] >> np.uint64(1))

    def _mesh(self, name):
        """native.Mesh of GEO/OBJ/<name>, parsed and uploaded at its first use."""
        if name not in self._meshes:
            from . import mesh_util, native
            v, f = mesh_util.load_obj_mesh(os.path.join(self.OBJ, name))
            self._meshes[name] = native.Mesh(v, f)
        return self._meshes[name]

    def select_sampling_method(self, subject, index=0):
        from . import native
        self._refuse_worker()
        name = subject[0] if isinstance(subject, (tuple, list)) else subject
        mesh_HR, mesh_LR = self._mesh(name + "_HR.obj"), self._mesh(name + "_LR.obj")
        n = self.num_sample_inout
        seed = self.item_seed(index)
        self.draws += 1
        pool, _ = native.mesh_sample_pool(mesh_HR, 4 * n, n // 4, self.opt.sigma, self.B_MIN, self.B_MAX, seed)
        inside_HR = native.mesh_contains(pool, mesh_HR)
        inside_LR = native.mesh_contains(pool, mesh_LR)
        s_hr, l_hr, s_lr, l_disp, _ = native.sample_select(pool, inside_HR, inside_LR, n)
        return {"samples_HR": s_hr, "samples_LR": s_lr, "labels_HR": l_hr, "labels_disp": l_disp}

    @staticmethod
    def _refuse_worker():
        import torch.utils.data
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError("TrainDataset makes its samples on the GPU of the calling process and cannot run in a DataLoader "
                               "worker: use --num_threads 0")

    def get_item(self, index):
        self._refuse_worker()
        sid = index % len(self.subjects)
        tmp = index // len(self.subjects)
        yid = tmp % len(self.yaw_list)
        pid = tmp // len(self.yaw_list)
        subject = os.path.splitext(self.subjects[sid])
        res = {"name": subject, "mesh_path_HR": os.path.join(self.OBJ, subject[0] + "_HR.obj"),
               "mesh_path_LR": os.path.join(self.OBJ, subject[0] + "_LR.obj"), "sid": sid, "yid": yid, "pid": pid,
               "b_min": self.B_MIN, "b_max": self.B_MAX}
        res.update(self.get_render(subject[0], num_views=self.num_views, yid=yid, pid=pid, random_sample=self.opt.random_multiview))
        if self.opt.num_sample_inout:
            res.update(self.select_sampling_method(subject, index))
        if self.num_sample_color:
            raise NotImplementedError("--num_sample_color %d: get_color_sampling is not built" % self.num_sample_color)
        return res

    def __getitem__(self, index):
        return self.get_item(index)
