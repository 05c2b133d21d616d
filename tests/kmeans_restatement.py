"""CPU restatement of libhsckmeans.so's step (include/hsckmeans.h) in numpy, float32 / float64: the oracle's 'valid'
correlation and flat arg-max for the assignment, numpy's pairwise summation written out for the patch norms, and the
sequential member sums.  `FakeContext` stands in for hsc_amd.kmeans._Context, so the learner's own host finishing
runs on top of it: the CPU rehearsal of the numerics the GPU must reproduce bit for bit."""
import numpy as np


def pairwise_sum(a):
    """numpy's pairwise summation (PW_BLOCKSIZE 128, 8 accumulators) along the last axis of a [rows, n] array,
    every row in the array's dtype."""
    n = a.shape[-1]
    dt = a.dtype.type
    if n < 8:
        res = np.zeros(a.shape[:-1], dtype=a.dtype)
        for i in range(n):
            res = res + a[..., i]
        return res
    if n <= 128:
        r = [a[..., u].copy() for u in range(8)]
        i = 8
        while i < n - n % 8:
            for u in range(8):
                r[u] = r[u] + a[..., i + u]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res = res + a[..., i]
            i += 1
        return res.astype(dt, copy=False)
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[..., :n2]) + pairwise_sum(a[..., n2:])


def patch_norms(patches):
    """normalize()'s norms of [m, W(,F)] patches: sqrt of the pairwise sum of squares, zero -> 1."""
    flat = patches.reshape((patches.shape[0], -1))
    norms = np.sqrt(pairwise_sum(flat * flat))
    return np.where(norms > 0.0, norms, np.ones_like(norms))


def sequential_sum(rows):
    """rows [m, ...] summed from the first row, one row after the other."""
    acc = rows[0].copy()
    for i in range(1, rows.shape[0]):
        acc = acc + rows[i]
    return acc


def sequential_mean(rows):
    """np.mean(rows, axis=0) as the learner forms it: the sequential sum, divided by np.intp(m) as np.mean divides."""
    S = sequential_sum(rows)
    out = np.empty_like(S)
    np.true_divide(S, np.intp(rows.shape[0]), out=out, casting='unsafe')
    return out


def assign(windows, D):
    """Flat arg-max of |'valid' correlation| (the oracle's pinned chain) of windows [N, 2W, F] with D [K, W, F]."""
    from oracle import hsc_oracle as orc
    t = np.zeros(len(windows), dtype=np.int32)
    k = np.zeros(len(windows), dtype=np.int32)
    for n in range(len(windows)):
        ip = orc.convolve1d(np.ascontiguousarray(windows[n]), np.ascontiguousarray(D), padding='valid')
        o = int(np.argmax(np.abs(ip).reshape(-1)))
        t[n], k[n] = o // ip.shape[1], o % ip.shape[1]
    return t, k


class FakeContext(object):
    """The numpy twin of hsc_amd.kmeans._Context (set_data / step)."""

    def set_data(self, x, starts, W):
        self.x, self.starts, self.W = x, starts, W
        self.B, self.T, self.F = x.shape
        self.N = starts.shape[1]
        self.dtype = x.dtype

    def step(self, D, mode):
        B, K = D.shape[0], D.shape[1]
        W, F, N = self.W, self.F, self.N
        t = np.zeros((B, N), dtype=np.int32)
        k = np.zeros((B, N), dtype=np.int32)
        count = np.zeros((B, K), dtype=np.int32)
        nonzero = np.zeros((B, K), dtype=np.int32)
        sums = np.zeros((B, K, W * F), dtype=self.dtype)
        for b in range(B):
            if mode[b] == 0:
                continue
            dt = np.float32 if mode[b] == 1 else np.float64
            idx = self.starts[b][:, None] + np.arange(2 * W)[None, :]
            windows = self.x[b][idx].astype(dt)                         # widening is exact
            t[b], k[b] = assign(windows, D[b].astype(dt))
            pidx = (self.starts[b] + t[b])[:, None] + np.arange(W)[None, :]
            patches = self.x[b][pidx].reshape((N, W * F))               # the data's dtype
            rows = patches / patch_norms(patches)[:, None]
            for c in range(K):
                members = np.flatnonzero(k[b] == c)
                count[b, c] = len(members)
                nonzero[b, c] = int(np.any(members > 0))
                if len(members):
                    sums[b, c] = sequential_sum(rows[members])
        return t, k, count, nonzero, sums, np.zeros((4,))
