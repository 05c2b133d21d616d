"""What the tests of the per-signal SNR table of the hierarchical coder share: the table and the census
of it with the CPU oracle.  The cases are those of tests/test_gpu_ragged_hierarchy.py."""
import numpy as np

from tests.test_gpu_ragged_hierarchy import _OracleLevelCoder

# rows = signals, columns = levels, in dB.  tests/test_rules_hierarchy_census.py is the condition this table has to meet.
S = [[6, 20, 12], [9, 16, 18], [12, 12, 8], [15, 8, 14], [18, 24, 10]]
SINGLETON_WEIGHT = 0.95

_COUNTS = {}


def oracle_hcmp():
    """The hierarchical host logic with the CPU oracle as its level coder (no GPU)."""
    from hsc_amd.modeling import HierarchicalConvolutionalMatchingPursuit
    ref = HierarchicalConvolutionalMatchingPursuit(method='cmp')
    ref._level_coder = lambda D: _OracleLevelCoder(D)
    return ref


def level_counts(name, x, b, mld, row, nbBlocks):
    """Stored non-zeros per level of signal b of case `name` under `row` (one target per level): computed once per key."""
    key = (name, b, tuple(float(v) for v in row), str(nbBlocks))
    if key not in _COUNTS:
        levels = oracle_hcmp()._forwardPhase(x, mld, list(row), nbBlocks, SINGLETON_WEIGHT)
        _COUNTS[key] = [int(np.count_nonzero(c.toarray())) for c in levels]
    return _COUNTS[key]
