"""Float64 restatement of the convolutional K-SVD learner's dictionary update (hsc/modeling.py:591-633) as
include/hscksvd.h states it, for the tests of hsc_amd.ksvd.  CPU only, no GPU library needed; the coefficient stage
of `learn` is the C oracle's CMP encoder (oracle/hsc_oracle.py).

Per atom k, in order, with the occurrences t_1 < ... < t_m (the rows of column k whose value is not 0.0):
  1. error = the overlap-add of every other column's non-zero coefficients in CSC order (np.add.at is unbuffered:
     each sample sums its terms c * D[k'] in entry order), P_i = error[t_i - (W-1)//2 : ... + W] (0 outside [0, T));
  2. SVD branch: u = top eigenvector of G = sum P_i P_i^T (numpy's eigh), c_i = P_i . u;
     PCA branch: the patches centred per component first when m >= 2;
     m = 1: u = P / |P|;
  3. zero G: u = e_0 (SVD) / e_{n-1} (PCA); zero window with PCA and m = 1: u = 0; otherwise (an eigenvector, or
     P / |P| in the SVD branch) u . D_old[k] >= 0, and the first non-zero entry of u positive when that is 0.
"""
import numpy as np
import scipy.sparse


def _orient(u, d_old):
    dot = float(np.dot(u, d_old))
    nz = np.flatnonzero(u)
    if dot < 0.0 or (dot == 0.0 and len(nz) and u[nz[0]] < 0.0):
        return -u
    return u


def sweep(D, coefficients, usePCA=False):
    """D [K,W] or [K,W,F], coefficients [T,K] sparse.  Returns (D float64 of D's shape, csc float64 with the updated
    values, stats [K,4]: n_k, lambda1, lambda2, rule), rule 0: no occurrence, 1: eigenvector, 2: P / |P|,
    3: zero G or zero window."""
    D3 = np.array(np.asarray(D).reshape((D.shape[0], D.shape[1], -1)), dtype=np.float64)
    K, W, F = D3.shape
    n, lead = W * F, (W - 1) // 2
    csc = scipy.sparse.csc_matrix(coefficients, dtype=np.float64, copy=True)
    csc.sort_indices()
    T = csc.shape[0]
    rows, indptr, data = csc.indices.astype(np.int64), csc.indptr, csc.data
    cols = np.repeat(np.arange(K), np.diff(indptr))
    taps = np.arange(W)
    stats = np.zeros((K, 4))
    for k in range(K):
        occ = np.arange(indptr[k], indptr[k + 1])
        occ = occ[data[occ] != 0.0]
        m = len(occ)
        if m == 0:
            continue
        keep = np.flatnonzero((cols != k) & (data != 0.0))
        error = np.zeros((T, F))
        if len(keep):
            pos = (rows[keep, np.newaxis] - lead + taps[np.newaxis, :]).reshape(-1)
            elems = (data[keep, np.newaxis, np.newaxis] * D3[cols[keep]]).reshape(-1, F)
            inside = (pos >= 0) & (pos < T)
            np.add.at(error, pos[inside], elems[inside])
        padded = np.concatenate([np.zeros((W, F)), error, np.zeros((W, F))])
        P = np.stack([padded[W + t - lead:W + t - lead + W].reshape(-1) for t in rows[occ]])
        d_old = D3[k].reshape(-1)
        l1 = l2 = 0.0
        if m == 1:
            nrm = np.sqrt(np.sum(np.square(P[0])))
            l1 = nrm * nrm
            if nrm > 0.0:
                u = P[0] / nrm
                rule = 2
                if not usePCA:
                    u = _orient(u, d_old)
            else:
                u = np.zeros(n)
                if not usePCA:
                    u[0] = 1.0
                rule = 3
        else:
            if usePCA:
                P = P - P.mean(axis=0)
            G = P.T @ P
            if not np.any(G):
                u = np.zeros(n)
                u[n - 1 if usePCA else 0] = 1.0
                rule = 3
            else:
                w, V = np.linalg.eigh(G)
                u = _orient(V[:, -1].copy(), d_old)
                l1, l2 = w[-1], (w[-2] if n > 1 else 0.0)
                if usePCA:
                    l1, l2 = l1 / (m - 1), l2 / (m - 1)
                rule = 1
        D3[k] = u.reshape(W, F)
        data[occ] = P @ u
        stats[k] = (m, l1, l2, rule)
    return D3.reshape(D.shape), csc, stats


def learn(x, D0, nbNonzeroCoefs=None, toleranceSnr=40.0, usePCA=False, maxIterations=100, tolerance=0.0):
    """The learner with the C oracle's CMP encoder.  Returns (D history [iterations][K,W(,F)], alphas, stats per
    iteration)."""
    from oracle import hsc_oracle as orc
    D = np.array(D0, dtype=np.float64)
    hist, alphas, stats = [], [], []
    n, alpha = 0, tolerance + 1.0
    while n < maxIterations and alpha > tolerance:
        coefficients, _, _ = orc.cmp_encode(x, D, nbNonzeroCoefs=nbNonzeroCoefs, toleranceSnr=toleranceSnr)
        newD, _, st = sweep(D, coefficients, usePCA)
        alpha = np.sqrt(np.sum(np.square(newD - D)))
        D = newD
        hist.append(D)
        alphas.append(alpha)
        stats.append(st)
        n += 1
    return hist, alphas, stats
