"""Float64 restatement of ConvolutionalNMFLearner.trainCorpus (hscnmf_learn_corpus): ONE dictionary
learnt from B signals of different lengths.  CPU only, no library needed.

One iteration:
  1. for every signal b, the W multiplicative coefficient steps of the coder (tests/nmf_restatement.py) against the shared D;
  2. R_b = X_b / |recon(A_b, D)| with the updated A_b and the old D;
  3. N[k,t,f] = sum_b sum_{s<L_b} A_b[s,k] R_b[s+t,f],  den[k] = sum_b sum_{s<L_b} A_b[s,k]   (L_b = T_b-W+1);
  4. D = D * (N / den), then every atom divided by its l2 norm over (W,F) when that is > 0;
  5. residual_b = X_b - recon(A_b, D); the coder's stop rules in the coder's order on the corpus statistics
     max_b max|residual_b| and 10 log10(sum_b energy_b / sum_b sum residual_b^2).
The sums over b run in ascending signal order.  For one signal every line is tests/nmf_learn_restatement.learn's.

This is the reference's _train_nmf on the concatenation of the signals with the coefficient rows whose atoms would
straddle a join (rows T_b-W+1 .. T_b-1 of each signal) started at exactly zero: multiplicative updates keep them at
zero, so the reconstruction separates per signal and every sum becomes the corpus sum (tools/make_golden_nmf_corpus.py).
"""
import numpy as np

from tests.nmf_restatement import STOP_MAX_ITERATIONS, STOP_RESIDUAL_SCALE, STOP_SNR, reconstruct


def learn_corpus(signals, D_init, A0s, nbMaxIterations=None, toleranceResidualScale=None, toleranceSnr=None,
                 dtype=np.float64):
    """signals: a list of [T_b] or [T_b,F] arrays; D_init [K,W] or [K,W,F]; A0s: a list of [T_b,K] (or [L_b,K]) initial
    coefficients.  Returns (D [K,W,F], iterations, stop code, snr, residualScale, signal_snr [B], signal_residualScale [B]),
    D in `dtype` (float32: the same sums in numpy's float32 arithmetic, for the round-off spread of a float32 run)."""
    Xs = [np.asarray(x, dtype=dtype).reshape((x.shape[0], -1)) for x in signals]
    D3 = np.array(D_init, dtype=dtype).reshape((D_init.shape[0], D_init.shape[1], -1))
    K, W, F = D3.shape
    if W < 2 or any(X.shape[0] < W for X in Xs) or len(Xs) < 1:
        raise Exception('bad shape: T = %s, W = %d' % ([X.shape[0] for X in Xs], W))
    Ts = [X.shape[0] for X in Xs]
    Ls = [T - W + 1 for T in Ts]
    As = [np.array(A0[:L], dtype=dtype) for A0, L in zip(A0s, Ls)]
    energies = [np.sum(np.square(X)) for X in Xs]
    maxIt = 1 if nbMaxIterations is None else nbMaxIterations
    it = 0
    while True:
        N, den = None, None
        for b, (X, T, L) in enumerate(zip(Xs, Ts, Ls)):
            A = As[b]
            for t in range(W):
                R = X / np.abs(reconstruct(A, D3, T))
                num = np.einsum('kf,sf->sk', D3[:, t, :], R[t:t + L])
                A = A * (num / np.sum(D3[:, t, :], axis=1)[np.newaxis, :])
            As[b] = A
            R = X / np.abs(reconstruct(A, D3, T))
            den_b = np.sum(A, axis=0)
            N_b = np.stack([A.T.dot(R[t:t + L]) for t in range(W)], axis=1)          # [K, W, F]
            N, den = (N_b, den_b) if b == 0 else (N + N_b, den + den_b)
        D3 = D3 * (N / den[:, np.newaxis, np.newaxis])
        norms = np.sqrt(np.sum(np.square(D3), axis=(1, 2), keepdims=True))
        D3 = D3 / np.where(norms > 0.0, norms, 1.0)
        residuals = [X - reconstruct(A, D3, T) for X, A, T in zip(Xs, As, Ts)]
        sig_rs = np.array([np.max(np.abs(r)) for r in residuals], dtype=np.float64)
        sig_ss = [np.sum(np.square(r)) for r in residuals]
        sig_snr = np.array([10.0 * np.log10(e / s) for e, s in zip(energies, sig_ss)], dtype=np.float64)
        rs = np.max(sig_rs)
        energy, ss = energies[0], sig_ss[0]
        for e, s in zip(energies[1:], sig_ss[1:]):
            energy, ss = energy + e, ss + s
        snr = 10.0 * np.log10(energy / ss)
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
    return D3, it, stop, snr, rs, sig_snr, sig_rs
