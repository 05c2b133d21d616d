"""The empirical information-rate functions of hsc_amd.analysis against what the reference returned on the same data
(tests/golden/analysis.npz, written by tools/make_golden_analysis.py from the real reference): same operations, same dtype,
so the figures are compared exactly."""
import os

import numpy as np
import pytest
import scipy.sparse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'analysis.npz')


class _Dictionary(object):
    """What the functions read of a MultilevelDictionary: counts, scales, decompositions, getNbLevels."""

    def __init__(self, g):
        self.counts = g['counts']
        self.scales = g['scales']
        self.decompositions = []
        for l in range(1, len(self.counts)):
            ptr = g['dec%d_ptr' % l]
            lev, fi, ti = g['dec%d_levels' % l], g['dec%d_findices' % l], g['dec%d_tindices' % l]
            self.decompositions.append([[lev[a:b], fi[a:b], ti[a:b], None] for a, b in zip(ptr[:-1], ptr[1:])])

    def getNbLevels(self):
        return len(self.counts)


@pytest.fixture(scope='module')
def golden():
    g = np.load(GOLDEN)
    matrices = [scipy.sparse.csc_matrix((g['m%d_data' % l], g['m%d_indices' % l], g['m%d_indptr' % l]), shape=tuple(g['m%d_shape' % l]))
                for l in range(len(g['counts']))]
    return g, _Dictionary(g), matrices


def test_fixture_is_what_the_issue_asks_for(golden):
    g, mld, matrices = golden
    assert mld.getNbLevels() == 3 and int(g['T']) == 2048 > int(mld.scales.max())
    assert all(m.shape == (2048, k) and m.nnz > 0 for m, k in zip(matrices, mld.counts))
    assert os.path.getsize(GOLDEN) < 64 * 1024


def test_multilevel_rates_equal_the_reference(golden):
    from hsc_amd.analysis import calculateEmpiricalMultilevelInformationRates
    g, mld, matrices = golden
    before = [m.copy() for m in matrices]
    got = calculateEmpiricalMultilevelInformationRates(matrices, mld)
    assert got.dtype == g['multilevel_rates'].dtype and got.shape == (3,)
    assert np.array_equal(got, g['multilevel_rates'])
    assert got[0] > got[1] > got[2]                       # handing events down multiplies them
    for a, b in zip(matrices, before):                    # the caller's matrices are not edited
        assert (a != b).nnz == 0


def test_information_rate_equals_the_reference_sparse_and_dense(golden):
    from hsc_amd.analysis import calculateEmpiricalInformationRates
    g, mld, matrices = golden
    got = calculateEmpiricalInformationRates(matrices, mld)
    assert isinstance(got, float) and got == float(g['rate'])
    assert got == float(g['multilevel_rates'][-1])       # nothing handed down yet
    dense = [g['ev%d' % l] for l in range(3)]
    assert all(d.shape == (m.nnz, 3) for d, m in zip(dense, matrices))
    got = calculateEmpiricalInformationRates(dense, mld)
    assert isinstance(got, float) and got == float(g['rate_dense'])


def test_distribution_ratios_equal_the_reference(golden):
    from hsc_amd.analysis import calculateDistributionRatios
    g, mld, matrices = golden
    got = calculateDistributionRatios(matrices)
    assert got.dtype == np.float64 and np.array_equal(got, g['ratios'])
    assert got.sum() == pytest.approx(1.0, abs=1e-15)
    nnz = np.array([m.nnz for m in matrices], dtype=np.float64)
    assert np.array_equal(got, nnz / nnz.sum())
