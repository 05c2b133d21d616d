"""Golden vectors of the reference's convolutional k-means learner over a corpus of signals -> tests/golden/kmeans_corpus.npz.

Needs the reference next to the repository (loaded read-only through oracle/ref_loader.py); run from the
repository root:  python tools/make_golden_kmeans_corpus.py

The reference's learner (ConvolutionalDictionaryLearner(algorithm='kmean'), hsc/modeling.py:420-526) runs unchanged
except for one function replaced in memory: the loaded module's extractRandomWindows(data, nb, width) draws over the
admissible starts of ALL signals of the case (tests/kmeans_corpus_restatement.py::corpus_windows)
and cuts every window from its own signal.  The learner is handed the stacked signals as `data`, which it reads only
for the low / high of a 'noise' initialisation and for their dimensions.  Nothing of the reference's text is stored.

Every case stores its signals (x: the stack, lengths), the numpy seed, the arguments, and what the reference computed:
D (dtype included), every iteration's assignment (assign_t / assign_k [iterations][N]), nbResets [iterations], the
number of iterations, and the drawn windows (win_signal / win_start [N]).  The assignments are checked against the
pinned fma chain of the oracle, as in tools/make_golden_kmeans.py.  Cases:
  uniform_b4        four float64 signals of one length ([B,T] form);
  ragged_short      a ragged list whose shortest signal has exactly 2W + 1 samples (one admissible start, drawn);
  odd_w             odd W on a ragged list;
  sparse_level_f3   [T_b,3] level-style coefficients, most windows all zero;
  f32_noise         float32 data, initMethod='noise';
  f32_noise_reset   float32 data, random_samples init, a 'noise' reset promotes D to float64 mid-run;
  end_samples       resetMethod='random_samples' on signals of 2W + 1 .. 2W + 4 samples: every patch is cut next to its
  end_average       signal's end; the same with 'random_samples_average';
  tolerance_stop    tolerance > 0, half way between two logged alphas: the run stops early;
  window0_only      a seed (searched over 0 .. 199, recorded) under which some centroid's only member is window 0.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import make_golden_kmeans as mk  # noqa: E402
from oracle import ref_loader  # noqa: E402
from tests.kmeans_corpus_restatement import corpus_windows  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'kmeans_corpus.npz')


class _Corpus(object):
    """Stands in for the reference module's extractRandomWindows while one case runs."""

    def __init__(self, signals):
        self.signals = signals
        self.draws = []

    def __call__(self, sequence, nbWindows, width):
        sig, start = corpus_windows(self.signals, nbWindows, width, np.random)
        self.draws.append((sig, start))
        windows = np.stack([self.signals[b][s:s + width] for b, s in zip(sig, start)])
        if windows.ndim < sequence.ndim + 1:               # _init_D hands a [T,1] view of 1-D data
            windows = windows[:, :, np.newaxis]
        return windows


def run_case(ref, signals, K, W, seed, kw):
    corpus = _Corpus(signals)
    orig = ref.modeling.extractRandomWindows
    ref.modeling.extractRandomWindows = corpus
    try:
        D, rec, resets, alphas = mk.run_reference(ref, np.concatenate(signals), K, W, seed, kw)
    finally:
        ref.modeling.extractRandomWindows = orig
    return D, rec, resets, alphas, corpus.draws[0]


def short_signals(nb, W, seed, dtype=np.float64):
    """Signals of 2W + 1 .. 2W + 4 samples with a few non-zero bursts: every window ends at or next to its signal's end."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(nb):
        x = np.zeros(2 * W + 1 + rs.randint(0, 4))
        if rs.rand() < 0.6:
            c = rs.randint(0, len(x) - 4)
            x[c:c + 4] = rs.standard_normal(4)
        out.append(x.astype(dtype))
    return out


def main():
    ref = ref_loader.load_reference()
    assert ref is not None, 'the reference is not available in this environment'
    P, L = mk.planted_1d, mk.level_signal
    cases = [
        ('uniform_b4', 'array', [P(800, 25, 10 + b, np.float64) for b in range(4)], 6, 16, 31,
         dict(nbRandomWindows=300, maxIterations=5, tolerance=0.0, resetMethod='random_samples')),
        ('ragged_short', 'list', [P(160, 6, 20, np.float64), P(33, 1, 21, np.float64), P(240, 9, 22, np.float64),
                                  P(70, 2, 23, np.float64)], 6, 16, 33,
         dict(nbRandomWindows=300, maxIterations=5, tolerance=0.0, resetMethod='noise')),
        ('odd_w', 'list', [P(500, 18, 30, np.float64), P(1200, 40, 31, np.float64), P(90, 3, 32, np.float64)], 7, 15, 32,
         dict(nbRandomWindows=250, maxIterations=5, tolerance=0.0, resetMethod='random_samples')),
        ('sparse_level_f3', 'list', [L(700, 3, 14, 40), L(300, 3, 6, 41), L(1000, 3, 20, 42)], 8, 12, 34,
         dict(nbRandomWindows=400, maxIterations=5, tolerance=0.0, resetMethod='random_samples')),
        ('f32_noise', 'list', [P(900, 30, 50), P(400, 12, 51), P(700, 22, 52)], 6, 16, 35,
         dict(nbRandomWindows=300, maxIterations=5, tolerance=0.0, initMethod='noise', resetMethod='noise')),
        ('f32_noise_reset', 'list', [L(1200, 1, 12, 60, np.float32)[:, 0], L(800, 1, 8, 61, np.float32)[:, 0],
                                     L(1000, 1, 10, 62, np.float32)[:, 0]], 8, 16, 36,
         dict(nbRandomWindows=300, maxIterations=5, tolerance=0.0, initMethod='random_samples', resetMethod='noise')),
        ('end_samples', 'list', short_signals(40, 8, 70), 6, 8, 37,
         dict(nbRandomWindows=200, maxIterations=6, tolerance=0.0, resetMethod='random_samples')),
        ('end_average', 'list', short_signals(40, 9, 71), 6, 9, 38,
         dict(nbRandomWindows=200, maxIterations=6, tolerance=0.0, resetMethod='random_samples_average', nbAveragedPatches=5)),
        ('tolerance_stop', 'list', [P(1000, 35, 80), P(600, 20, 81), P(1100, 36, 82)], 5, 16, 39,
         dict(nbRandomWindows=300, maxIterations=12, resetMethod='random_samples')),
    ]
    out = {}
    names = []

    def store(name, form, signals, K, W, seed, kw, D, rec, resets, draw):
        names.append(name)
        out[name + '/x'] = np.concatenate(signals)
        out[name + '/lengths'] = np.array([len(q) for q in signals], dtype=np.int64)
        out[name + '/form'] = form
        out[name + '/D'] = D
        out[name + '/assign_t'] = np.stack([r[0] for r in rec]).astype(np.int32)
        out[name + '/assign_k'] = np.stack([r[1] for r in rec]).astype(np.int32)
        out[name + '/nbResets'] = np.array(resets, dtype=np.int32)
        out[name + '/iterations'] = len(rec)
        out[name + '/win_signal'], out[name + '/win_start'] = draw[0].astype(np.int32), draw[1].astype(np.int32)
        out[name + '/K'], out[name + '/W'], out[name + '/seed'] = K, W, seed
        for a, v in kw.items():
            out[name + '/' + a] = v

    for name, form, signals, K, W, seed, kw in cases:
        if name == 'tolerance_stop':
            kw = dict(kw, tolerance=0.0)
            alphas = run_case(ref, signals, K, W, seed, kw)[3]
            i = next(i for i in range(2, len(alphas)) if alphas[i] < 0.5 * min(alphas[:i]))
            kw['tolerance'] = 0.5 * (alphas[i] + min(alphas[:i]))
        D, rec, resets, _, draw = run_case(ref, signals, K, W, seed, kw)
        assert mk.oracle_agrees(rec), name
        if name == 'ragged_short':
            assert np.any(draw[0] == 1), name                # the one admissible start of the shortest signal is drawn
        assert len(rec) <= 6 or name == 'tolerance_stop', name
        if name.startswith('end_') or name == 'f32_noise_reset':
            assert sum(resets) > 0, name
        if name == 'f32_noise_reset':
            assert D.dtype == np.float64 and rec[0][3].dtype == np.float32, name      # promoted mid-run
        print('%-16s D %s %s, %d iterations, resets %s' % (name, D.shape, D.dtype, len(rec), resets))
        store(name, form, signals, K, W, seed, kw, D, rec, resets, draw)
    # a seed under which some centroid's only member is window 0 (the reference's np.any() quirk)
    signals = [L(700, 2, 3, 90), L(400, 2, 2, 91), L(900, 2, 4, 92)]
    kw = dict(nbRandomWindows=200, maxIterations=3, tolerance=0.0, resetMethod='random_samples')
    for seed in range(200):
        D, rec, resets, _, draw = run_case(ref, signals, 8, 8, seed, kw)
        if mk.window0_only(rec) and mk.oracle_agrees(rec):
            print('%-16s seed %d, resets %s' % ('window0_only', seed, resets))
            store('window0_only', 'list', signals, 8, 8, seed, kw, D, rec, resets, draw)
            break
    else:
        print('window0_only: no seed in 0 .. 199 leaves a centroid with window 0 as its only member; case not stored')
    out['names'] = np.array(names)
    np.savez_compressed(OUT, **out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
