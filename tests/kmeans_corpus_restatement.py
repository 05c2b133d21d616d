"""CPU restatement of the corpus form of libhsckmeans.so (hsckmeans_set_corpus, include/hsckmeans.h): the numpy twin of
tests/kmeans_restatement.py with the stacked-signal upload, and the corpus window draw of DESIGN.md section 17 written
out in plain numpy, one window at a time."""
import numpy as np

from tests.kmeans_restatement import FakeContext


class FakeCorpusContext(FakeContext):
    """The numpy twin of hsc_amd.kmeans._Context with set_corpus: one learner on the stack [rows, F], after the checks
    hsckmeans_set_corpus makes on the host."""

    def set_corpus(self, x, row_offsets, starts, W):
        assert row_offsets[0] == 0 and x.shape[0] == row_offsets[-1]
        lens = np.diff(row_offsets)
        assert np.all(lens > 2 * W), 'every signal is longer than 2W'
        for n, s in enumerate(starts):
            b = int(np.searchsorted(row_offsets, s, side='right')) - 1
            assert row_offsets[b] <= s and s + 2 * W <= row_offsets[b + 1], 'window %d crosses a seam' % n
        self.row_offsets = row_offsets
        self.set_data(x[np.newaxis], np.asarray(starts)[np.newaxis], W)

    def set_plan(self, plan):
        assert plan in (0, 1, 2)


def corpus_windows(signals, nb, width, rng):
    """`nb` windows of `width` samples over the admissible starts of all signals: signal b offers the starts
    0 .. T_b - width - 1 (A_b = T_b - width of them); one randint over their total, then signal by signal.
    Returns (signal [nb], start [nb])."""
    A = [len(q) - width for q in signals]
    g = rng.randint(low=0, high=sum(A), size=(nb,))
    sig = np.zeros(nb, dtype=np.int64)
    start = np.zeros(nb, dtype=np.int64)
    for n in range(nb):
        r = int(g[n])
        b = 0
        while r >= A[b]:
            r -= A[b]
            b += 1
        sig[n], start[n] = b, r
    return sig, start
