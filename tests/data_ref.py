"""Host restatement of the device data path (ncnerf_amd.data / csrc/data.hip), for the tests:
the counter-based draws in Python integers, both corner modes, get_rays and the axis-angle pose
correction in fp64 (torch, differentiable)."""
import numpy as np
import torch

M64 = (1 << 64) - 1


def splitmix64_at(seed, k):
    """Output k of splitmix64 under `seed`: the state seed + k * gamma through the finaliser."""
    z = (seed + 0x9E3779B97F4A7C15 * k) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def counter_key(step, r):
    return ((step & M64) * 0x100000001B3 + r) & M64


def below(z, n):
    """Integer in [0, n): the high 64 bits of the 128-bit product z * n."""
    return (z * n) >> 64


def draw_patches(seed, step, n_images, H, W, patch, n_patches, same_image):
    """(image, corner ordinal) of every patch: ordinals in [0, (H-patch+1)(W-patch+1))."""
    seed &= M64
    n_corners = (H - patch + 1) * (W - patch + 1)
    imgs, corners = [], []
    for p in range(n_patches):
        zi = splitmix64_at(seed, counter_key(step, 0 if same_image else 1 + 2 * p))
        zc = splitmix64_at(seed, counter_key(step, 2 + 2 * p))
        imgs.append(below(zi, n_images))
        corners.append(below(zc, n_corners))
    return np.array(imgs, np.int64), np.array(corners, np.int64)


def patch_pixels(corners, H, W, patch, corner_mode):
    """Pixels (n_patches, patch^2) of patches with the given corner ordinals, cells row-major.
    "reference": offset iy W + ix added to the ordinal; "grid": to the corner the ordinal names."""
    iy, ix = np.meshgrid(np.arange(patch, dtype=np.int64), np.arange(patch, dtype=np.int64), indexing="ij")
    iy, ix = iy.reshape(-1), ix.reshape(-1)
    c = np.asarray(corners, np.int64)[:, None]
    if corner_mode == "reference":
        return c + iy[None] * W + ix[None]
    assert corner_mode == "grid"
    cw = W - patch + 1
    return (c // cw + iy[None]) * W + c % cw + ix[None]


def draw(seed, step, n_images, H, W, patch, n_patches, same_image=False, corner_mode="reference"):
    """img_idxs, pix_idxs (n_patches patch^2 int64) as ncn_batch_draw writes them."""
    imgs, corners = draw_patches(seed, step, n_images, H, W, patch, n_patches, same_image)
    return np.repeat(imgs, patch * patch), patch_pixels(corners, H, W, patch, corner_mode).reshape(-1)


def axis_angle_matrix(v):
    """The reference's axis-angle map for v (B,3), any float dtype: I + sin(t)/t K + (1-cos(t))/t^2 K^2,
    K = skew(v), t = |v| + 1e-7."""
    z = torch.zeros_like(v[:, 0])
    K = torch.stack([torch.stack([z, -v[:, 2], v[:, 1]], -1), torch.stack([v[:, 2], z, -v[:, 0]], -1),
                     torch.stack([-v[:, 1], v[:, 0], z], -1)], 1)
    t = (torch.norm(v, dim=1) + 1e-7)[:, None, None]
    eye = torch.eye(3, dtype=v.dtype)
    return eye + torch.sin(t) / t * K + (1 - torch.cos(t)) / t ** 2 * (K @ K)


def rays(poses, directions, img_idxs, pix_idxs, dR=None, dT=None):
    """rays_o, rays_d (R,3) in fp64: rays_d = (A(dR[i]) R_i) dir, rays_o = t_i + dT[i]; differentiable
    w.r.t. dR, dT (fp64 tensors).  poses (V,3,4), directions (HW,3): tensors of any float dtype."""
    P = poses.double()[img_idxs]
    d = directions.double()[pix_idxs]
    Rm, t = P[:, :, :3], P[:, :, 3]
    if dR is not None:
        Rm = axis_angle_matrix(dR[img_idxs]) @ Rm
        t = t + dT[img_idxs]
    return t, torch.einsum("nij,nj->ni", Rm, d)


def random_rotations(n, rng):
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def small_scene(V, H, W, seed=0):
    """images (V, HW, 3) uint8, poses (V,3,4) f32 (random rotations, centres in [-0.2, 0.2]^3),
    directions (HW,3) f32 unit pinhole directions."""
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, size=(V, H * W, 3), dtype=np.uint8)
    poses = np.concatenate([random_rotations(V, rng), rng.uniform(-0.2, 0.2, size=(V, 3, 1))], -1).astype(np.float32)
    u, v = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    d = np.stack([(u - W / 2) / W, (v - H / 2) / W, np.ones_like(u)], -1).reshape(-1, 3)
    directions = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return images, poses, directions
