"""Float64 direct-sum restatement of the reference's ConvolutionalNMF.computeCoefficients
(hsc/modeling.py:662-747), for the tests of hsc_amd.nmf.  CPU only, no library needed.

One iteration is W steps t = 0 .. W-1, each
  recon[n,f] = sum_j sum_k A[n-j,k] D[k,j,f]   (0 <= n-j <= T-W),
  R = X / |recon|,  U[s,k] = sum_f D[k,t,f] R[s+t,f] / sum_f D[k,t,f]  (R = 0 past T),  A *= U,
then residual = X - recon and the stop rules nbMaxIterations, toleranceResidualScale, toleranceSnr (in
that order; nbMaxIterations=None stops after the first iteration, as `int >= None` does in Python 2).
"""
import numpy as np

STOP_MAX_ITERATIONS, STOP_RESIDUAL_SCALE, STOP_SNR = 1, 2, 3


def reconstruct(A, D3, T):
    """A [L,K] (L = T-W+1), D3 [K,W,F] -> [T,F] in A's dtype: each P[s, j] = sum_k A[s,k] D[k,j,:] lands on sample
    s+j, the W products of a sample summed in ascending j."""
    K, W, F = D3.shape
    L = A.shape[0]
    P = A.dot(D3.reshape((K, W * F))).reshape((L, W, F))
    out = np.zeros((T, F), dtype=A.dtype)
    for j in range(W):
        out[j:j + L] += P[:, j, :]
    return out


def nmf(sequence, D, A0, nbMaxIterations=None, toleranceResidualScale=None, toleranceSnr=None, dtype=np.float64):
    """sequence [T] or [T,F], D [K,W] or [K,W,F], A0 [T,K] the initial coefficients.
    Returns (coefficientsCentered [T,K], residual [T,F], iterations, stop code, snr, residualScale), every array in
    `dtype` (float32: the same sums in numpy's float32 arithmetic, for the round-off spread of a float32 run)."""
    X = np.asarray(sequence, dtype=dtype).reshape((sequence.shape[0], -1))
    D3 = np.asarray(D, dtype=dtype).reshape((D.shape[0], D.shape[1], -1))
    T, (K, W, F) = X.shape[0], D3.shape
    if W < 2 or T < W:
        raise Exception('bad shape: T = %d, W = %d' % (T, W))
    L = T - W + 1
    A = np.array(A0[:L], dtype=dtype)
    energySignal = np.sum(np.square(X))
    maxIt = 1 if nbMaxIterations is None else nbMaxIterations
    it = 0
    while True:
        for t in range(W):
            R = X / np.abs(reconstruct(A, D3, T))
            Rt = R[t:t + L]                                          # s + t <= T-1 for every kept row
            num = np.einsum('kf,sf->sk', D3[:, t, :], Rt)
            A = A * (num / np.sum(D3[:, t, :], axis=1)[np.newaxis, :])
        residual = X - reconstruct(A, D3, T)
        rs = np.max(np.abs(residual))
        snr = 10.0 * np.log10(energySignal / np.sum(np.square(residual)))
        it += 1
        if it >= maxIt:
            stop = STOP_MAX_ITERATIONS
        elif toleranceResidualScale is not None and rs <= toleranceResidualScale:
            stop = STOP_RESIDUAL_SCALE
        elif toleranceSnr is not None and snr >= toleranceSnr:
            stop = STOP_SNR
        else:
            continue
        break
    coef = np.zeros((T, K), dtype=dtype)
    off = (W - 1) // 2
    coef[off:off + L] = A
    return coef, residual, it, stop, snr, rs
