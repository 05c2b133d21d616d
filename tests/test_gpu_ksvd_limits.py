"""libhscksvd's dictionary update at the atom sizes its one-workgroup Jacobi solver was sized for: W*F from 33 to the
limit of 64 (at 64 every lane of a wave owns a sample and a Jacobi round rotates 32 pairs), the PCA branch there, and
one atom with thousands of occurrences, some within W of both signal ends.  Against the float64 restatement
(tests/ksvd_restatement.py), as test_ksvd.test_update_matches_restatement compares; the Jacobi loop must also converge
before its cap of 40 sweeps."""
import numpy as np
import pytest
import scipy.sparse

from hsc_amd import ksvd
from tests import ksvd_restatement as rst
from tests.test_ksvd import _DeviceTouched, _err_up_to_sign, _random_input, no_device  # noqa: F401 (a fixture)

MAX_SWEEPS = 40             # kMaxSweeps of hscksvd.hip


def _heavy_input(T, K, W, F, m, seed):
    """Atom 0 at m positions (among them the first and last W samples of the signal, where its patches run off the
    ends), the other atoms at 4 m / K random positions each."""
    rs = np.random.RandomState(seed)
    D = rs.randn(K, W, F)
    D /= np.sqrt(np.sum(np.square(D), axis=(1, 2), keepdims=True))
    ends = np.concatenate([np.arange(W), np.arange(T - W, T)])
    t0 = np.unique(np.concatenate([ends, rs.choice(np.arange(W, T - W), m - len(ends), replace=False)]))
    t = np.concatenate([t0, rs.randint(0, T, 4 * m)])
    k = np.concatenate([np.zeros(len(t0), np.int64), rs.randint(1, K, 4 * m)])
    key = np.unique(t.astype(np.int64) * K + k)
    t, k = key // K, key % K
    A = scipy.sparse.csc_matrix((rs.randn(len(key)), (t, k)), shape=(T, K))
    return (D[:, :, 0] if F == 1 else D), A


def compare_with_restatement(out, D, A, pca):
    """`out` = (D, coefficients, stats, ...) of a device sweep of (D, A) against the restatement's: n_k exactly, D within
    1e-10 (with the restatement's signs), the coefficients within 1e-12 max|A|, the top eigenvalues, and the Jacobi loop
    converged under its cap.  A problem without a stored entry has nothing but D and the zero stats to compare."""
    D_ref, A_ref, st_ref = rst.sweep(D, A, pca)
    D_gpu, A_gpu, st_gpu = out[:3]
    assert np.array_equal(st_gpu[:, 0], st_ref[:, 0])
    assert _err_up_to_sign(D_gpu, D_ref) <= 1e-10
    assert np.array_equal(A_gpu.indices, A_ref.indices) and np.array_equal(A_gpu.indptr, A_ref.indptr)
    if A_ref.nnz:
        scale = np.max(np.abs(A_ref.data))
        assert np.max(np.abs(A_gpu.data - A_ref.data)) <= 1e-12 * scale
    assert np.max(np.abs(D_gpu - D_ref)) <= 1e-10
    occ = st_ref[:, 3] == 1
    assert np.allclose(st_gpu[occ, 1], st_ref[occ, 1], rtol=1e-10, atol=1e-12 * np.max(st_ref[:, 1]))
    # every atom that went through the eigensolver converged: a sweep that rotated nothing ended the loop, under the cap
    assert np.all(st_gpu[occ, 3] >= 1) and np.all(st_gpu[st_ref[:, 0] > 0, 3] < MAX_SWEEPS), st_gpu[:, 3]
    return st_ref


def _check(D, A, pca):
    st_ref = compare_with_restatement(ksvd.update(D, A, usePCA=pca), D, A, pca)
    assert np.any(st_ref[:, 3] == 1)
    return st_ref


# (W, F): the atom sizes 33 .. 64 of the solver's one-workgroup plan
LARGE_ATOMS = [
    (33, 1),    # n = 33: one past 32, a padded order n2 = 34 and 17 rotations a round
    (63, 1),    # n = 63: odd, padded to 64
    (64, 1),    # n = 64: the limit, 32 rotations a round, no padding
    (32, 2),    # n = 64 with two features
    (21, 3),    # n = 63 with three features
    (16, 4),    # n = 64 with four features
]


@pytest.mark.gpu
@pytest.mark.parametrize('W,F', LARGE_ATOMS, ids=['W%d_F%d' % a for a in LARGE_ATOMS])
def test_update_large_atoms_match_restatement(W, F):
    D, A = _random_input(3000, 8, W, F, 200, W * 10 + F, 1)
    _check(D, A, False)


@pytest.mark.gpu
@pytest.mark.parametrize('W', [64, 33])
def test_update_large_atoms_pca_match_restatement(W):
    D, A = _random_input(3000, 8, W, 1, 120, W, 1)
    _check(D, A, True)


@pytest.mark.gpu
@pytest.mark.parametrize('pca', [False, True], ids=['svd', 'pca'])
def test_update_atom_with_thousands_of_occurrences(pca):
    D, A = _heavy_input(20000, 6, 64, 1, 4000, 5)
    st = _check(D, A, pca)
    assert st[0, 0] == 4000 and st[0, 3] == 1


def test_atom_size_past_the_limit_raises_before_any_device_call(no_device):
    """W*F = 65 is refused by check_update_shapes; W*F = 64 gets through to the device."""
    A = scipy.sparse.csc_matrix(np.eye(500, 4))
    with pytest.raises(NotImplementedError, match='64'):
        ksvd.update(np.ones((4, 65)), A)
    with pytest.raises(NotImplementedError, match='64'):
        ksvd.update(np.ones((4, 13, 5)), A)
    with pytest.raises(_DeviceTouched):
        ksvd.update(np.ones((4, 64)), A)
