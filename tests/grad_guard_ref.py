"""What the gradient-guard tests share (test_grad_guard_host.py, test_gpu_grad_guard.py): the tensor list, the tolerance of
the norm and a numpy restatement of dfn_grad_stats' documented accumulation order (include/dfanerf.h).

Tolerance of the norm against float64.  Every element passes through one squaring and 11 f32 additions: 3 in its thread's
pairwise sum of 8, 8 in the butterfly over 256 threads.  All terms are >= 0, so 12 roundings of 2^-24 bound the relative error
of a chunk's partial by 12 * 2^-24 = 7.2e-7; the partials are then added in double (nothing at this scale).  The root halves
it (3.6e-7), its own rounding and the cast to f32 add 2^-24 each: about 5e-7.  NORM_RTOL is four times that."""
import numpy as np

CHUNK = 2048
# the chunk boundaries (2047 / 2048 / 2049), the 256-thread boundary (255 / 256), a one-element tensor, and with 700 * 2048 + 3
# more partials (714 in all) than the finishing block has threads (256) and its staging tile has entries (512)
SHAPES = [(1,), (255,), (256,), (2047,), (2048,), (2049,), (5000,), (700 * 2048 + 3,), (3, 7, 5), (64, 64)]
N_CHUNKS = sum(-(-int(np.prod(s)) // CHUNK) for s in SHAPES)
NORM_RTOL = 2e-6


def chunk_partials(grads):
    """[n_chunks] float32: per chunk of each tensor (in list order), thread t squares its elements t + 256 j (j = 0..7, zero
    beyond the end) and adds them pairwise in index order; then s = s + s[t ^ d] for d = 1, 2, ..., 128."""
    out = []
    lane = np.arange(256)
    for g in grads:
        g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
        n_ch = -(-g.size // CHUNK)
        pad = np.zeros(n_ch * CHUNK, np.float32)
        pad[:g.size] = g
        with np.errstate(over="ignore", invalid="ignore"):
            q = pad.reshape(n_ch, 8, 256)
            q = q * q
            s = ((q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])) + ((q[:, 4] + q[:, 5]) + (q[:, 6] + q[:, 7]))
            d = 1
            while d < 256:
                s = s + s[:, lane ^ d]
                d *= 2
        assert s.dtype == np.float32
        out.append(s[:, 0])
    return np.concatenate(out)


def ordered_sumsq(grads):
    """The partials added in index order in double (np.cumsum adds left to right)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.cumsum(chunk_partials(grads).astype(np.float64))[-1])


def norm64(grads):
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads)))
