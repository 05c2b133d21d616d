"""Golden vectors of the reference's convolutional K-SVD learner (ConvolutionalDictionaryLearner(algorithm='ksvd'),
hsc/modeling.py:528-641) -> tests/golden/ksvd.npz.

Needs the reference next to the repository (loaded read-only through oracle/ref_loader.py); run from the
repository root:  python tools/make_golden_ksvd.py

Every case stores its float64 signal x, the numpy seed under which the reference draws its initial dictionary (the
draw itself is not stored: tests redo it from the seed), the arguments of train(), and the reference's outputs:
  D_hist [N][K][W(,F)]   the reference's D after iterations 1 .. N, each from train(maxIterations=i) under the seed
                         (the reference is deterministic), with tolerance = 0;
  spec   [calls][4]      for every svd / eigh the update made in the N-iteration run: iteration, number of patches,
                         the top two singular values (svd) or covariance eigenvalues (eigh), recorded by wrapping
                         scipy.linalg.svd / eigh while the reference runs;
  gap                    the smallest relative gap (top1 - top2) / top1 over those calls (1 when no call had two);
  tolerance, iterations  the learner's stop tolerance and the iteration count it must stop at.  A case with
                         tolerance > 0 has it half way between two consecutive SIGN-ALIGNED alphas (include/hscksvd.h's
                         sign rule applied to the reference's history, hsc_amd.ksvd's stop quantity).
"""
import logging
import os
import sys

import numpy as np
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'ksvd.npz')


def planted(T, K, W, F, nb, seed, noise=0.01):
    """A float64 signal of `nb` random atoms (K shapes of width W) at random positions, plus white noise."""
    rs = np.random.RandomState(seed)
    atoms = rs.randn(K, W, F)
    atoms /= np.sqrt(np.sum(np.square(atoms), axis=(1, 2), keepdims=True))
    x = noise * rs.randn(T, F)
    for t, k, a in zip(rs.randint(0, T - W, nb), rs.randint(0, K, nb), rs.randn(nb)):
        x[t:t + W] += (2.0 + abs(a)) * np.sign(a) * atoms[k]
    return x[:, 0] if F == 1 else x


# name, signal (T, K_planted, W, F, nb, seed), learner (K, W), train arguments, N iterations, seed of the draws
CASES = [
    ('script_locomp', (4000, 16, 32, 1, 60, 1), (64, 32), dict(method='locomp', nbNonzeroCoefs=100, toleranceSnr=20.0), 3, 13),
    ('script_cmp', (4000, 16, 32, 1, 60, 1), (64, 32), dict(method='cmp', nbNonzeroCoefs=100, toleranceSnr=20.0), 3, 13),
    ('odd_w', (2000, 6, 15, 1, 50, 2), (8, 15), dict(method='cmp', nbNonzeroCoefs=60, toleranceSnr=40.0), 4, 12),
    ('odd_w_locomp', (2000, 6, 15, 1, 50, 2), (8, 15), dict(method='locomp', nbNonzeroCoefs=60, toleranceSnr=40.0), 3, 12),
    ('features2', (1500, 4, 16, 2, 40, 3), (6, 16), dict(method='cmp', nbNonzeroCoefs=50, toleranceSnr=40.0), 3, 13),
    ('snr_stop', (2000, 4, 16, 1, 30, 4), (8, 16), dict(method='cmp', nbNonzeroCoefs=None, toleranceSnr=10.0), 3, 14),
    ('never_occurs', (2000, 4, 16, 1, 12, 5), (16, 16), dict(method='cmp', nbNonzeroCoefs=8, toleranceSnr=40.0), 3, 15),
    ('dense', (600, 6, 32, 1, 80, 6), (8, 32), dict(method='cmp', nbNonzeroCoefs=300, toleranceSnr=60.0), 3, 16),
    ('pca', (3000, 4, 16, 1, 10, 7), (8, 16), dict(method='cmp', nbNonzeroCoefs=14, toleranceSnr=40.0, usePCA=True), 3, 17),
    ('tolerance_stop', (1500, 4, 16, 1, 40, 8), (6, 16), dict(method='cmp', nbNonzeroCoefs=40, toleranceSnr=40.0), 6, 18),
]


def align(D_new, D_prev):
    """include/hscksvd.h's sign rule applied per atom to a reference dictionary: orient D_new[k] so that
    D_new[k] . D_prev[k] >= 0, and when that is exactly 0 so that its first non-zero entry is positive.
    (The zero rules' e_0 / e_{n-1} and PCA's P / |P| are the reference's own vectors and are kept as they are.)"""
    out = np.array(D_new, dtype=np.float64)
    K = out.shape[0]
    a, b = out.reshape(K, -1), np.asarray(D_prev, np.float64).reshape(K, -1)
    for k in range(K):
        nz = np.flatnonzero(a[k])
        if np.array_equal(a[k], b[k]) or (len(nz) == 1 and a[k][nz[0]] == 1.0):
            continue                                   # unchanged, or the zero rules' e_0 / e_{n-1}
        d = float(np.dot(a[k], b[k]))
        if d < 0.0 or (d == 0.0 and len(nz) and a[k][nz[0]] < 0.0):
            a[k] = -a[k]
    return out


def aligned_history(D0, hist):
    out, prev = [], np.asarray(D0, np.float64)
    for D in hist:
        prev = align(D, prev)
        out.append(prev)
    return out


def run(ns, x, seed, K, W, kw, maxIterations, record=None):
    np.random.seed(seed)
    cdl = ns.modeling.ConvolutionalDictionaryLearner(K, W, algorithm='ksvd')
    return cdl.train(x, maxIterations=maxIterations, tolerance=0.0, **kw)


class _Iterations(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self, logging.DEBUG)
        self.n = 0

    def emit(self, record):
        if record.getMessage().startswith('K-SVD iteration'):
            self.n += 1


def run_recorded(ns, x, seed, K, W, kw, N):
    calls = []
    h = _Iterations()
    log = logging.getLogger(ns.modeling.__name__)
    log.addHandler(h)
    log.setLevel(logging.DEBUG)
    svd, eigh = scipy.linalg.svd, scipy.linalg.eigh

    def svd_rec(a, *args, **kwargs):
        U, s, Vh = svd(a, *args, **kwargs)
        calls.append((h.n, a.shape[1], s[0], s[1] if len(s) > 1 else 0.0))
        return U, s, Vh

    def eigh_rec(a, *args, **kwargs):
        w, v = eigh(a, *args, **kwargs)
        top = np.sort(w)[::-1]
        calls.append((h.n, -1, top[0], top[1] if len(top) > 1 else 0.0))
        return w, v

    scipy.linalg.svd, scipy.linalg.eigh = svd_rec, eigh_rec
    try:
        D = run(ns, x, seed, K, W, kw, N)
    finally:
        scipy.linalg.svd, scipy.linalg.eigh = svd, eigh
        log.removeHandler(h)
    return D, np.array(calls, dtype=np.float64).reshape(-1, 4), h.n


def init_D(x, K, W, seed):
    sys.path.insert(0, ROOT)
    from hsc_amd.learning import ConvolutionalDictionaryLearner
    np.random.seed(seed)
    return ConvolutionalDictionaryLearner(K, W, algorithm='ksvd')._init_D(x, initMethod='noise')


def main():
    ns = ref_loader.load_reference()
    if ns is None:
        raise SystemExit('the reference is not available')
    out = {'names': np.array([c[0] for c in CASES])}
    for name, sig, (K, W), kw, N, seed in CASES:
        x = planted(*sig)
        hist = [np.asarray(run(ns, x, seed, K, W, kw, i), np.float64) for i in range(1, N)]
        D_last, calls, ran = run_recorded(ns, x, seed, K, W, kw, N)
        hist.append(np.asarray(D_last, np.float64))
        assert ran == N, (name, ran)
        gaps = [(c[2] - c[3]) / c[2] for c in calls if c[2] > 0.0 and c[3] > 0.0]
        gap = min(gaps) if gaps else 1.0
        tolerance, iterations = 0.0, N
        if name == 'tolerance_stop':
            ah = aligned_history(init_D(x, K, W, seed), hist)
            prev = init_D(x, K, W, seed)
            alphas = []
            for D in ah:
                alphas.append(float(np.sqrt(np.sum(np.square(D - prev)))))
                prev = D
            # stop after iteration j + 1: the first alpha below every earlier one, placed half way
            for j in range(1, len(alphas) - 1):
                if alphas[j] < min(alphas[:j]):
                    tolerance, iterations = 0.5 * (alphas[j] + min(alphas[:j])), j + 1
                    break
            assert tolerance > 0.0, alphas
            print('  %s: sign-aligned alphas %s, tolerance %.6g, stops after %d' % (name, alphas, tolerance, iterations))
        p = name + '/'
        out[p + 'x'] = x
        out[p + 'seed'] = np.int64(seed)
        out[p + 'K'] = np.int64(K)
        out[p + 'W'] = np.int64(W)
        out[p + 'method'] = np.array(kw['method'])
        out[p + 'nbNonzeroCoefs'] = np.float64(np.nan if kw['nbNonzeroCoefs'] is None else kw['nbNonzeroCoefs'])
        out[p + 'toleranceSnr'] = np.float64(kw['toleranceSnr'])
        out[p + 'usePCA'] = np.int64(bool(kw.get('usePCA', False)))
        out[p + 'maxIterations'] = np.int64(N)
        out[p + 'tolerance'] = np.float64(tolerance)
        out[p + 'iterations'] = np.int64(iterations)
        out[p + 'D_hist'] = np.stack(hist)
        out[p + 'spec'] = calls
        out[p + 'gap'] = np.float64(gap)
        print('%-16s T=%d K=%d W=%d calls=%d gap=%.3g' % (name, x.shape[0], K, W, len(calls), gap), flush=True)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
