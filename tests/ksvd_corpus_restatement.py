"""Float64 restatement of the corpus form of the K-SVD dictionary update (hscksvd_update_corpus, include/hscksvd.h):
`tests/ksvd_restatement.sweep` on the vertical stack of the signals' coefficient matrices, with the clipping and the
masks per signal.  CPU only; the coefficient stage of `learn` is the C oracle's CMP encoder, signal by signal.

What differs from ksvd_restatement.sweep (the rest is its text):
  * an entry of signal b adds to the samples [lo_b, hi_b) of the stack only (its span is clipped at its own signal's
    ends), lo_b / hi_b the first stacked row of signal b / of signal b + 1;
  * patch P_i of an occurrence in signal b is 0 outside [lo_b, hi_b).
The entries are walked in CSC order of the stack (column, then stacked row), so every sample sums its terms in the
order the contract names; the occurrences of an atom are in ascending stacked row.
"""
import numpy as np
import scipy.sparse

from tests.ksvd_restatement import _orient


def stack(coefficients):
    """(csc [sum T_b, K] float64 with sorted indices, offsets int64 [B+1]) of a list of [T_b,K] sparse matrices."""
    offsets = np.concatenate([[0], np.cumsum([c.shape[0] for c in coefficients])]).astype(np.int64)
    csc = scipy.sparse.vstack([scipy.sparse.csc_matrix(c, dtype=np.float64) for c in coefficients], format='csc')
    csc = scipy.sparse.csc_matrix(csc, dtype=np.float64, copy=True)
    csc.sort_indices()
    return csc, offsets


def interior_only(coefficients, W):
    """True when every stored entry's atom span lies inside its own signal: (W-1)//2 <= t <= T_b - W + (W-1)//2."""
    lead = (W - 1) // 2
    for c in coefficients:
        t = scipy.sparse.coo_matrix(c).row
        if len(t) and (t.min() < lead or t.max() > c.shape[0] - W + lead):
            return False
    return True


def sweep(D, coefficients, usePCA=False):
    """D [K,W] or [K,W,F], coefficients a list of B sparse [T_b,K].  Returns (D float64 of D's shape, list of B csc
    float64 with the updated values, stats [K,4]: n_k, lambda1, lambda2, rule), rule as in ksvd_restatement.sweep."""
    D3 = np.array(np.asarray(D).reshape((D.shape[0], D.shape[1], -1)), dtype=np.float64)
    K, W, F = D3.shape
    n, lead = W * F, (W - 1) // 2
    csc, offsets = stack(coefficients)
    T = csc.shape[0]
    rows, indptr, data = csc.indices.astype(np.int64), csc.indptr, csc.data
    cols = np.repeat(np.arange(K), np.diff(indptr))
    sig = np.searchsorted(offsets, rows, side='right') - 1
    lo, hi = offsets[sig], offsets[sig + 1]                  # per entry: the stacked rows [lo, hi) of its signal
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
            pos = rows[keep, np.newaxis] - lead + taps[np.newaxis, :]
            inside = ((pos >= lo[keep, np.newaxis]) & (pos < hi[keep, np.newaxis])).reshape(-1)
            elems = (data[keep, np.newaxis, np.newaxis] * D3[cols[keep]]).reshape(-1, F)
            np.add.at(error, pos.reshape(-1)[inside], elems[inside])
        padded = np.concatenate([np.zeros((W, F)), error, np.zeros((W, F))])
        P = []
        for e in occ:
            tau = rows[e] - lead + taps
            live = (tau >= lo[e]) & (tau < hi[e])
            P.append((padded[W + tau] * live[:, np.newaxis]).reshape(-1))
        P = np.stack(P)
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
    out = [scipy.sparse.csc_matrix(csc[offsets[b]:offsets[b + 1]]) for b in range(len(coefficients))]
    return D3.reshape(D.shape), out, stats


def learn(xs, D0, nbNonzeroCoefs=None, toleranceSnr=40.0, usePCA=False, maxIterations=100, tolerance=0.0):
    """The corpus learner with the C oracle's CMP encoder, signal by signal.  xs: a list of [T_b] or [T_b,F] signals.
    Returns (D history [iterations][K,W(,F)], alphas, stats per iteration, the coefficient lists the sweeps read)."""
    from oracle import hsc_oracle as orc
    D = np.array(D0, dtype=np.float64)
    hist, alphas, stats, codes = [], [], [], []
    n, alpha = 0, tolerance + 1.0
    while n < maxIterations and alpha > tolerance:
        coefficients = [orc.cmp_encode(x, D, nbNonzeroCoefs=nbNonzeroCoefs, toleranceSnr=toleranceSnr)[0] for x in xs]
        newD, _, st = sweep(D, coefficients, usePCA)
        alpha = np.sqrt(np.sum(np.square(newD - D)))
        D = newD
        hist.append(D)
        alphas.append(alpha)
        stats.append(st)
        codes.append(coefficients)
        n += 1
    return hist, alphas, stats, codes
