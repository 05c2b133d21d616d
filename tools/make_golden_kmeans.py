"""Golden vectors of the reference's convolutional k-means learner (ConvolutionalDictionaryLearner(algorithm='kmean'),
hsc/modeling.py:420-524) -> tests/golden/kmeans.npz.

Needs the reference next to the repository (loaded read-only through oracle/ref_loader.py); run from the
repository root:  python tools/make_golden_kmeans.py

Every case stores its signal x (float32 or float64), the numpy seed under which the reference draws its windows,
D and resets, the arguments of train(), and the reference's outputs, recorded while it runs:
  D              the learned dictionary (dtype included);
  assign_t/_k    [iterations][N] the assignment of every iteration (the arg-max over convolve1d_batch's output);
  nbResets       [iterations] from the reference's own log line;
  iterations     the number of iterations run.
The assignments are also checked against the pinned fma chain of the oracle, so that the cases
are ones on which the reference's BLAS order and the chain agree.  Cases:
  sparse_level      [T,8] level-style coefficients, W*F = 256, many all-zero windows;
  f32_noise         float32 data, initMethod='noise' and resetMethod='noise' (float64 D from the start);
  f32_noise_reset   float32 data, random_samples init, a 'noise' reset promotes D to float64 mid-run;
  average           resetMethod='random_samples_average';
  window0_only      a seed (searched, recorded) under which some centroid's only member is window 0;
  tolerance_stop    tolerance > 0, half way between two logged alphas: the run stops early.
"""
import logging
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'kmeans.npz')


def level_signal(T, F, nb, seed, dtype=np.float64):
    """A sparse [T, F] coefficient stream: `nb` bursts of a few non-zero coefficients, most windows all zero."""
    rs = np.random.RandomState(seed)
    x = np.zeros((T, F))
    for c in rs.randint(0, T - 8, nb):
        for _ in range(rs.randint(1, 4)):
            x[c + rs.randint(0, 8), rs.randint(F)] = rs.uniform(0.5, 2.0) * rs.choice([-1.0, 1.0])
    return x.astype(dtype)


def planted_1d(T, nb, seed, dtype=np.float32):
    rs = np.random.RandomState(seed)
    x = np.zeros(T)
    atoms = rs.standard_normal((4, 16))
    for _ in range(nb):
        t = rs.randint(0, T - 16)
        x[t:t + 16] += atoms[rs.randint(4)] * rs.uniform(0.5, 2.0)
    return x.astype(dtype)


class _Log(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self, logging.DEBUG)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def run_reference(ref, x, K, W, seed, kw):
    """The reference's train() under numpy seed `seed`, with its assignments and log lines recorded."""
    rec = []
    orig = ref.modeling.convolve1d_batch

    def spy(sequences, filters, padding='valid'):
        c = orig(sequences, filters, padding)
        flat = np.argmax(np.abs(c.reshape(c.shape[0], -1)), axis=1)
        rec.append((flat // c.shape[2], flat % c.shape[2], np.array(sequences), np.array(filters)))
        return c

    h = _Log()
    root = logging.getLogger()
    old = root.level
    root.addHandler(h)
    root.setLevel(logging.DEBUG)
    ref.modeling.convolve1d_batch = spy
    try:
        np.random.seed(seed)
        D = ref.modeling.ConvolutionalDictionaryLearner(K, W, algorithm='kmean').train(x, **kw)
    finally:
        ref.modeling.convolve1d_batch = orig
        root.removeHandler(h)
        root.setLevel(old)
    logs = [m for m in h.lines if m.startswith('K-mean iteration')]
    resets = [int(re.search(r'nb resets = (\d+)', m).group(1)) for m in logs]
    alphas = [float(re.search(r'tolerance = ([0-9.e+-]+|nan|inf)', m).group(1)) for m in logs]
    return D, rec, resets, alphas


def oracle_agrees(rec):
    from oracle import hsc_oracle as orc
    for t, k, windows, D in rec:
        w3 = windows.reshape((windows.shape[0], windows.shape[1], -1))
        D3 = D.reshape((D.shape[0], D.shape[1], -1))
        dt = np.result_type(w3.dtype, D3.dtype)
        for n in range(len(w3)):
            ip = orc.convolve1d(np.ascontiguousarray(w3[n], dtype=dt), np.ascontiguousarray(D3, dtype=dt), padding='valid')
            o = int(np.argmax(np.abs(ip).reshape(-1)))
            if (o // ip.shape[1], o % ip.shape[1]) != (t[n], k[n]):
                return False
    return True


def window0_only(rec):
    return any(np.array_equal(np.flatnonzero(k == c), [0]) for _, k, _, _ in rec for c in range(int(k.max()) + 1))


def main():
    ref = ref_loader.load_reference()
    assert ref is not None, 'the reference is not available in this environment'
    cases = [
        ('sparse_level', level_signal(6000, 8, 150, 1), 16, 32, 21,
         dict(nbRandomWindows=400, maxIterations=5, tolerance=0.0, resetMethod='random_samples')),
        ('f32_noise', planted_1d(3000, 80, 2), 6, 16, 22,
         dict(nbRandomWindows=300, maxIterations=5, tolerance=0.0, initMethod='noise', resetMethod='noise')),
        ('f32_noise_reset', level_signal(4000, 1, 40, 3, np.float32)[:, 0], 8, 16, 23,
         dict(nbRandomWindows=300, maxIterations=5, tolerance=0.0, initMethod='random_samples', resetMethod='noise')),
        ('average', planted_1d(3000, 80, 4, np.float64), 7, 15, 24,
         dict(nbRandomWindows=250, maxIterations=5, tolerance=0.0, resetMethod='random_samples_average', nbAveragedPatches=5)),
        ('tolerance_stop', planted_1d(3000, 100, 5), 5, 16, 25,
         dict(nbRandomWindows=300, maxIterations=12, resetMethod='random_samples')),
    ]
    out = {}
    names = []
    for name, x, K, W, seed, kw in cases:
        if name == 'tolerance_stop':
            kw = dict(kw, tolerance=0.0)
            _, _, _, alphas = run_reference(ref, x, K, W, seed, kw)
            i = next(i for i in range(2, len(alphas)) if alphas[i] < 0.5 * min(alphas[:i]))
            kw['tolerance'] = 0.5 * (alphas[i] + min(alphas[:i]))
        D, rec, resets, _ = run_reference(ref, x, K, W, seed, kw)
        assert oracle_agrees(rec), name
        print('%-16s D %s %s, %d iterations, resets %s' % (name, D.shape, D.dtype, len(rec), resets))
        names.append(name)
        out[name + '/x'] = x
        out[name + '/D'] = D
        out[name + '/assign_t'] = np.stack([r[0] for r in rec]).astype(np.int32)
        out[name + '/assign_k'] = np.stack([r[1] for r in rec]).astype(np.int32)
        out[name + '/nbResets'] = np.array(resets, dtype=np.int32)
        out[name + '/iterations'] = len(rec)
        out[name + '/K'], out[name + '/W'], out[name + '/seed'] = K, W, seed
        for a, v in kw.items():
            out[name + '/' + a] = v
    # a seed under which some centroid's only member is window 0 (the reference's np.any() quirk)
    x = level_signal(2000, 2, 30, 6)
    kw = dict(nbRandomWindows=60, maxIterations=3, tolerance=0.0, resetMethod='random_samples')
    for seed in range(1000):
        D, rec, resets, _ = run_reference(ref, x, 6, 8, seed, kw)
        if window0_only(rec) and oracle_agrees(rec):
            break
    else:
        raise AssertionError('no seed with a window-0-only centroid')
    print('%-16s seed %d, resets %s' % ('window0_only', seed, resets))
    names.append('window0_only')
    out['window0_only/x'] = x
    out['window0_only/D'] = D
    out['window0_only/assign_t'] = np.stack([r[0] for r in rec]).astype(np.int32)
    out['window0_only/assign_k'] = np.stack([r[1] for r in rec]).astype(np.int32)
    out['window0_only/nbResets'] = np.array(resets, dtype=np.int32)
    out['window0_only/iterations'] = len(rec)
    out['window0_only/K'], out['window0_only/W'], out['window0_only/seed'] = 6, 8, seed
    for a, v in kw.items():
        out['window0_only/' + a] = v
    out['names'] = np.array(names)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
