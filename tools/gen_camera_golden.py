"""Capture tests/golden/cameras.npz from the reference's Focal_Net and Pose_Net (lib/models/tools/camera_net.py).

The two classes are imported from the reference checkout where it lies (tools/ref_import.py) and run on the CPU in float32 and in float64.
They call pytorch3d through lib.utils.transform; pytorch3d is not installed, so the two functions they need are STAND-INS WRITTEN HERE
(rotation_6d_to_matrix after Zhou et al. 2019 as pytorch3d documents it, axis_angle_to_matrix as the exponential map) and put into
lib.utils.transform before the classes run.  What the fixture pins is therefore everything AROUND the rotation formula: composition order
(M @ init_c2w), the 4x4 completion, index and duplicate handling, focal orders, initial values, parameter names / shapes / flags.  The
rotation formulas themselves are pinned by the float64 restatement in tests/test_cameras.py.

Only arrays and name lists are written, no program text.  Usage: python tools/gen_camera_golden.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_import  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cameras.npz")
STAND_INS = ["pytorch3d.transforms.rotation_6d_to_matrix", "pytorch3d.transforms.axis_angle_to_matrix"]
SERIES_THETA2 = 1e-4


def rotation_6d_to_matrix(d6):
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = torch.nn.functional.normalize(b2, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def axis_angle_to_matrix(r):
    x = (r * r).sum(-1)
    small = x < SERIES_THETA2
    xs = torch.where(small, torch.ones_like(x), x)     # (branch before the square root: autograd through sqrt(0) is NaN)
    th = xs.sqrt()
    A = torch.where(small, 1 - x / 6, torch.sin(th) / th)
    B = torch.where(small, 0.5 - x / 24, 2 * torch.sin(th / 2) ** 2 / xs)
    z = torch.zeros_like(x)
    K = torch.stack([z, -r[..., 2], r[..., 1], r[..., 2], z, -r[..., 0], -r[..., 1], r[..., 0], z], -1).reshape(r.shape[:-1] + (3, 3))
    eye = torch.eye(3, dtype=r.dtype).expand(K.shape)
    return eye + A[..., None, None] * K + B[..., None, None] * (K @ K)


def inventory(module):
    sd = module.state_dict()
    flags = dict((k, p.requires_grad) for k, p in module.named_parameters())
    keys = list(sd.keys())
    return {"keys": np.array(keys), "shapes": np.array([str(tuple(sd[k].shape)) for k in keys]), "dtypes": np.array([str(sd[k].dtype) for k in keys]),
            "requires_grad": np.array([bool(flags[k]) for k in keys])}


def main():
    _, _, _, mods = ref_import.import_reference()
    tr = mods["transform"]
    tr.rotation_6d_to_matrix, tr.axis_angle_to_matrix = rotation_6d_to_matrix, axis_angle_to_matrix
    from lib.models.tools.camera_net import Focal_Net, Pose_Net
    out = {"stand_ins": np.array(STAND_INS)}
    rng = np.random.default_rng(20240611)
    H, W = 48, 64

    # ---- Focal_Net: every row of the focal table with every supported init_focal form; the runs use values moved off the initial ones
    focal_cases = []
    for order in (2, 1):
        for fx_only in (False, True):
            for init in ("none", "one", "two"):
                if init == "two" and (fx_only or order != 2):
                    continue
                name = f"focal:o{order}:{'fxonly' if fx_only else 'fxfy'}:{init}"
                focal_cases.append(name)
                init_focal = {"none": None, "one": np.array([57.25], dtype=np.float32), "two": np.array([61.5, 44.75], dtype=np.float32)}[init]
                req = (len(focal_cases) % 2 == 1)
                net = Focal_Net(H, W, req, fx_only, order=order, init_focal=init_focal)
                for k, v in inventory(net).items():
                    out[f"{name}:{k}"] = v
                for k, v in net.state_dict().items():
                    out[f"{name}:init:{k}"] = v.numpy().copy()
                out[f"{name}:req_grad"] = np.array(req)
                out[f"{name}:HW"] = np.array([H, W], dtype=np.int64)
                if init_focal is not None:
                    out[f"{name}:init_focal"] = init_focal
                probe = rng.standard_normal(2).astype(np.float32)
                out[f"{name}:probe"] = probe
                with torch.no_grad():
                    for p in net.parameters():
                        p.mul_(float(rng.uniform(0.8, 1.25)))
                for k, v in net.state_dict().items():
                    out[f"{name}:run:{k}"] = v.numpy().copy()
                for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
                    n2 = Focal_Net(H, W, True, fx_only, order=order, init_focal=init_focal).to(dt)
                    n2.load_state_dict({k: v.to(dt) for k, v in net.state_dict().items()})
                    f = n2()
                    out[f"{name}:ref_shape"] = np.array(f.shape, dtype=np.int64)
                    (f.reshape(-1) * torch.from_numpy(probe).to(dt)).sum().backward()
                    out[f"{name}:{tag}:focal"] = f.detach().reshape(-1).numpy()
                    for k, p in n2.named_parameters():
                        out[f"{name}:{tag}:d_{k}"] = p.grad.numpy().copy()
    out["focal_cases"] = np.array(focal_cases)

    # ---- Pose_Net: 6d and 3d, with and without init_c2w, ids with duplicates and in no order
    from scipy.spatial.transform import Rotation
    pose_cases = []
    n_cams = 12
    for mode in ("6d", "3d"):
        for with_init in (True, False):
            name = f"pose:{mode}:{'init' if with_init else 'noinit'}"
            pose_cases.append(name)
            learn_R, learn_t = (mode == "6d"), with_init
            init = None
            if with_init:
                init = np.tile(np.eye(4, dtype=np.float32), (n_cams, 1, 1))
                init[:, :3, :3] = Rotation.random(n_cams, random_state=int(rng.integers(1 << 30))).as_matrix().astype(np.float32)
                init[:, :3, 3] = (3 * rng.standard_normal((n_cams, 3))).astype(np.float32)
                out[f"{name}:init_c2w"] = init
            net = Pose_Net(n_cams, learn_R, learn_t, pose_mode=mode, init_c2w=torch.from_numpy(init.copy()) if with_init else None)
            for k, v in inventory(net).items():
                out[f"{name}:{k}"] = v
            for k in ("r", "t"):
                out[f"{name}:init:{k}"] = net.state_dict()[k].numpy().copy()
            out[f"{name}:learn"] = np.array([learn_R, learn_t])
            if mode == "6d":
                r = np.tile(np.array([1, 0, 0, 0, 1, 0], dtype=np.float32), (n_cams, 1)) + (0.2 * rng.standard_normal((n_cams, 6))).astype(np.float32)
            else:
                r = (0.3 * rng.standard_normal((n_cams, 3))).astype(np.float32)
            t = (0.1 * rng.standard_normal((n_cams, 3))).astype(np.float32)
            ids = rng.integers(0, n_cams, 8)
            ids[5] = ids[1]
            ids[6] = ids[1]
            probe = rng.standard_normal((8, 4, 4)).astype(np.float32)
            out[f"{name}:r"], out[f"{name}:t"], out[f"{name}:ids"], out[f"{name}:probe"] = r, t, ids.astype(np.int64), probe
            for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
                n2 = Pose_Net(n_cams, True, True, pose_mode=mode, init_c2w=torch.from_numpy(init.copy()).to(dt) if with_init else None).to(dt)
                with torch.no_grad():
                    n2.r.copy_(torch.from_numpy(r).to(dt))
                    n2.t.copy_(torch.from_numpy(t).to(dt))
                c2w = n2(torch.from_numpy(ids))
                (c2w * torch.from_numpy(probe).to(dt)).sum().backward()
                out[f"{name}:{tag}:c2w"] = c2w.detach().numpy()
                out[f"{name}:{tag}:d_r"], out[f"{name}:{tag}:d_t"] = n2.r.grad.numpy().copy(), n2.t.grad.numpy().copy()
    out["pose_cases"] = np.array(pose_cases)

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
