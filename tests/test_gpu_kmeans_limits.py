"""libhsckmeans's step at the edges of its launch plan, bit for bit against the numpy restatement
(tests/kmeans_restatement.FakeContext): windows per workgroup WPB = min(64, 256 / (W + 1)) from 64 (W = 1, 2) down to 1
(W >= 128) and the window limit W = 255 with W = 256 past it, window features staged FC at a time in 48 KB with
FC < F, and K across several groups of 16 atoms, a partial last group among them."""
import numpy as np
import pytest

from hsc_amd import _native
from hsc_amd import kmeans
from hsc_amd.kmeans import ConvolutionalKMeansLearner
from tests import kmeans_restatement as rst
from tests.test_kmeans import _DeviceTouched, no_device  # noqa: F401 (a fixture)

# the launch plan of hsckmeans_step, restated
MAX_W = 255                 # kMaxW: the W + 1 positions of a window fit the 256 columns of a workgroup
MAX_WPB = 64                # kMaxWPB
COLUMNS = 256               # 4 waves x kTilesPerWave (4) x 16 columns
STAGE_BYTES = 48 * 1024     # kStageBytes: the window features staged per workgroup


def windows_per_block(W):
    return max(1, min(MAX_WPB, COLUMNS // (W + 1)))


def staged_features(W, itemsize):
    """FC before it is clamped to F: as many features of WPB windows of 2W samples as fit the stage."""
    return max(1, STAGE_BYTES // (windows_per_block(W) * 2 * W * itemsize))


# (W, K, dtype); F = FC + 1, so the features come in two chunks, the second of one feature
STEPS = [
    (127, 16, np.float32),     # WPB = 2; K = 16: one full group
    (127, 64, np.float64),     # WPB = 2; K = 64: four full groups
    (128, 17, np.float32),     # WPB = 1 (W + 1 = 128 columns, half the workgroup's); K = 17: a group of one atom
    (128, 33, np.float64),     # WPB = 1; K = 33: two full groups and one of one atom
    (200, 33, np.float32),     # WPB = 1
    (200, 17, np.float64),     # WPB = 1
    (255, 64, np.float32),     # WPB = 1, W = kMaxW: all 256 columns
    (255, 16, np.float64),     # WPB = 1, W = kMaxW
    (1, 64, np.float32),       # WPB = 64 (capped): windows of 2 samples, 2 positions each
    (1, 17, np.float64),       # WPB = 64 (capped)
    (2, 33, np.float32),       # WPB = 64 (capped): 3 positions per window
    (2, 16, np.float64),       # WPB = 64 (capped)
]
N = 67                      # windows: a last workgroup of 1 (WPB = 2) or 3 (WPB = 64) windows


@pytest.mark.gpu
@pytest.mark.parametrize('W,K,dtype', STEPS, ids=['W%d-K%d-%s' % (w, k, np.dtype(d).name) for w, k, d in STEPS])
def test_step_matches_restatement(W, K, dtype):
    F = staged_features(W, np.dtype(dtype).itemsize) + 1
    T = 6 * W + 300
    rs = np.random.RandomState(W * 100 + K)
    x = rs.randn(T, F).astype(dtype)
    x[:2 * W] = 0.0                                                       # an all-zero window: (t, k) = (0, 0)
    starts = rs.randint(2 * W, T - 2 * W + 1, N).astype(np.int64)
    starts[:3] = 0, 2 * W, 4 * W                                         # windows 1 and 2 disjoint
    D = rs.randn(K, W, F)
    # the last atom (of the last group), and the first atom past the first group, planted as the patches at one
    # position of windows 1 and 2: the only atoms those windows can match, at that position
    tp = min(3, W)
    planted = {K - 1: 1}
    if K > 17:
        planted[16] = 2
    for a, n in planted.items():
        D[a] = x[starts[n] + tp:starts[n] + tp + W]
    D = D / np.sqrt(np.sum(D ** 2, axis=(1, 2), keepdims=True))
    mode = np.array([1 if dtype == np.float32 else 2], dtype=np.int32)
    ctx = kmeans._context(0)
    ctx.set_data(np.ascontiguousarray(x[None]), starts[None], W)
    t, k, count, nonzero, sums, _ = ctx.step(D[None], mode)
    fake = rst.FakeContext()
    fake.set_data(np.ascontiguousarray(x[None]), starts[None], W)
    t2, k2, count2, nonzero2, sums2, _ = fake.step(D[None], mode)
    assert (t2[0, 0], k2[0, 0]) == (0, 0)
    assert all((t2[0, n], k2[0, n]) == (tp, a) for a, n in planted.items())
    assert np.array_equal(t, t2) and np.array_equal(k, k2)
    assert np.array_equal(count, count2) and np.array_equal(nonzero, nonzero2)
    assert sums.dtype == sums2.dtype == dtype and np.array_equal(sums, sums2)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_window_past_the_limit_is_unsupported(dtype):
    W = MAX_W + 1
    x = np.random.RandomState(0).randn(1, 4 * W, 2).astype(dtype)
    with pytest.raises(_native.HscmpError) as ei:
        kmeans._context(0).set_data(x, np.zeros((1, 8), dtype=np.int64), W)
    assert ei.value.code == _native.ERR_UNSUPPORTED


def test_learner_window_past_the_limit_raises_before_any_device_call(no_device):
    x = np.random.RandomState(0).randn(2000)
    with pytest.raises(NotImplementedError, match=str(MAX_W)):
        ConvolutionalKMeansLearner(4, MAX_W + 1).train(x, 50)
    with pytest.raises(_DeviceTouched):
        ConvolutionalKMeansLearner(4, MAX_W).train(x, 50)
