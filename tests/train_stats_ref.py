"""What the tests of the training step's opacity / expected depth share - TEST INFRASTRUCTURE ONLY (a helper module like
tests/blend_scene.py): the definition of `stats` on the oracle's weights, the stats loss of the issue, and the numpy restatement of
composite_stats_kernel's documented summation order."""
import numpy as np
import torch

N_RAYS = 96
CONFIGS = [(64, 0), (32, 0), (128, 0), (64, 64), (64, 128)]          # (n_coarse, n_fine) of the training step


def stats_of(w_head, w_com, z, concate_bg=True):
    """stats [n, 4] = acc_head, depth_head, acc_com, depth_com from weights [n, S] and depths [n, S] (torch, differentiable):
    sums over FG = every sample but the last when concate_bg"""
    fg = slice(0, z.shape[-1] - 1) if concate_bg else slice(None)
    zz = torch.as_tensor(z)[..., fg].to(w_head.dtype)
    return torch.stack([w_head[..., fg].sum(-1), (w_head[..., fg] * zz).sum(-1), w_com[..., fg].sum(-1), (w_com[..., fg] * zz).sum(-1)], -1)


def matte(n, seed=11):
    """the random matte both acc are held against: [n, 2] in [0, 1)"""
    return torch.rand(n, 2, generator=torch.Generator().manual_seed(seed))


def stats_loss(stats, m):
    """squared error of both acc against the matte + (depth_com - 0.6 acc_com)^2, means over the rays"""
    m = m.to(stats.device, stats.dtype)
    return ((stats[:, 0] - m[:, 0]) ** 2).mean() + ((stats[:, 2] - m[:, 1]) ** 2).mean() + ((stats[:, 3] - 0.6 * stats[:, 2]) ** 2).mean()


def colour_loss(rgb_head, rgb_com, tgt):
    """the step's MSE"""
    tgt = tgt.to(rgb_head.device, rgb_head.dtype)
    return ((rgb_head - tgt) ** 2).mean() + ((rgb_com - tgt) ** 2).mean()


def ordered_sums(w, z, K, concate_bg=True):
    """composite_stats_kernel's sums in its documented order, in float32: w, z [n, S] in depth order, lane l owns the K consecutive
    positions l K ... l K + K - 1 (S <= 64 K; lanes past S idle).  A lane starts at 0 and adds its positions in index order (acc: w;
    depth: the float32 product w z), then the butterfly adds partners at XOR distance 32, 16, 8, 4, 2, 1 -> (acc [n], depth [n])"""
    w, z = np.asarray(w, np.float32), np.asarray(z, np.float32)
    n, S = w.shape
    assert S <= 64 * K
    fg = np.ones(S, bool)
    if concate_bg:
        fg[-1] = False
    pa, pd = np.zeros((n, 64), np.float32), np.zeros((n, 64), np.float32)
    for lane in range(64):
        for k in range(K):
            i = lane * K + k
            if i < S and fg[i]:
                pa[:, lane] = pa[:, lane] + w[:, i]
                pd[:, lane] = pd[:, lane] + (w[:, i] * z[:, i]).astype(np.float32)
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        pa = (pa + pa[:, lanes ^ d]).astype(np.float32)
        pd = (pd + pd[:, lanes ^ d]).astype(np.float32)
    return pa[:, 0], pd[:, 0]
