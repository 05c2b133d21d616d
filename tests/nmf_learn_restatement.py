"""Float64 restatement of the reference's convolutional NMF dictionary learner (ConvolutionalDictionaryLearner._train_nmf,
hsc/modeling.py:330-417) with L = T-W+1 coefficient rows, for the tests of hsc_amd.nmf.ConvolutionalNMFLearner.
CPU only, no library needed.

One iteration:
  1. the W multiplicative coefficient steps of the coder (tests/nmf_restatement.py);
  2. R = X / |recon(A, D)| with the updated A and the old D;
  3. N[k,t,f] = sum_{s<L} A[s,k] R[s+t,f],  den[k] = sum_{s<L} A[s,k];
  4. D = D * (N / den), then every atom divided by its l2 norm over (W,F) when that is > 0;
  5. residual = X - recon(A, D), and the coder's stop rules in the coder's order.
The reference keeps A as [T,K] and sums coefficients[:-t]: the rows s >= L are zero after the first step t = W-1 (it
multiplies them by a zero-padded ratio), so summing over L rows is exact.
"""
import numpy as np

from tests.nmf_restatement import STOP_MAX_ITERATIONS, STOP_RESIDUAL_SCALE, STOP_SNR, reconstruct


def learn(sequence, D_init, A0, nbMaxIterations=None, toleranceResidualScale=None, toleranceSnr=None, dtype=np.float64):
    """sequence [T] or [T,F], D_init [K,W] or [K,W,F], A0 [T,K] the initial coefficients.
    Returns (D [K,W,F], iterations, stop code, snr, residualScale), D in `dtype` (float32: the same sums in numpy's
    float32 arithmetic, for the round-off spread of a float32 run)."""
    X = np.asarray(sequence, dtype=dtype).reshape((sequence.shape[0], -1))
    D3 = np.array(D_init, dtype=dtype).reshape((D_init.shape[0], D_init.shape[1], -1))
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
            num = np.einsum('kf,sf->sk', D3[:, t, :], R[t:t + L])
            A = A * (num / np.sum(D3[:, t, :], axis=1)[np.newaxis, :])
        R = X / np.abs(reconstruct(A, D3, T))
        den = np.sum(A, axis=0)
        N = np.stack([A.T.dot(R[t:t + L]) for t in range(W)], axis=1)              # [K, W, F]
        D3 = D3 * (N / den[:, np.newaxis, np.newaxis])
        norms = np.sqrt(np.sum(np.square(D3), axis=(1, 2), keepdims=True))
        D3 = D3 / np.where(norms > 0.0, norms, 1.0)
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
    return D3, it, stop, snr, rs
