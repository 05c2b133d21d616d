"""The table of tests/test_gpu_rules_hierarchy.py can tell a signal's own SNR targets from its neighbours' (DESIGN.md section 26).

No GPU: the hierarchical host logic (_forwardPhase) runs with the CPU oracle as its level coder, on the generated case of
tests/test_gpu_ragged_hierarchy.py, with nbBlocks 4 and 1.  Two conditions on the stored non-zeros per level:

  rows     every signal longer than 3 Wmax - 3 samples, at every level, has another count under its own row than under at least
           3 of the other 4 rows -- an encode that handed signal b somebody else's row would show;
  columns  replacing one entry of a signal's row by the next signal's value of that column changes that level's count for at
           least three of the four signals longer than Wmax -- an encode that read a column from the wrong signal would show.

The signal of exactly Wmax samples has one position per atom and cannot tell; it is exempt from both."""
import numpy as np
import pytest

from tests.rules_hierarchy_util import S, level_counts
from tests.test_gpu_ragged_hierarchy import GENERATED_SCALES, _lengths, cases  # noqa: F401 (fixture)

B, LEVELS = 5, 3


@pytest.fixture(scope='module')
def generated(cases):  # noqa: F811
    name, xs, mld, _, _, _ = cases('generated')
    lengths = _lengths(GENERATED_SCALES)
    assert [len(x) for x in xs] == lengths and np.shape(S) == (B, LEVELS)
    return name, xs, mld, lengths


@pytest.mark.parametrize('nbBlocks', [4, 1])
def test_a_row_tells_its_signal(generated, nbBlocks):
    name, xs, mld, lengths = generated
    wmax = lengths[1]
    long_ones = [b for b in range(B) if lengths[b] > 3 * wmax - 3]
    assert len(long_ones) == 3
    worst = B
    for b in long_ones:
        own = level_counts(name, xs[b], b, mld, S[b], nbBlocks)
        assert all(n > 0 for n in own), (b, own)
        for l in range(LEVELS):
            differ = sum(level_counts(name, xs[b], b, mld, S[r], nbBlocks)[l] != own[l] for r in range(B) if r != b)
            print('nbBlocks %s signal %d level %d: differs under %d of 4 rows' % (nbBlocks, b, l, differ))
            worst = min(worst, differ)
            assert differ >= 3, (nbBlocks, b, l, differ)
    assert worst >= 3


@pytest.mark.parametrize('nbBlocks', [4, 1])
def test_a_column_tells_its_signal(generated, nbBlocks):
    name, xs, mld, lengths = generated
    wmax = lengths[1]
    four = [b for b in range(B) if lengths[b] > wmax]
    assert len(four) == 4
    for l in range(LEVELS):
        changed = []
        for b in four:
            row = list(S[b])
            row[l] = S[(b + 1) % B][l]
            assert row[l] != S[b][l]
            changed.append(level_counts(name, xs[b], b, mld, row, nbBlocks)[l] != level_counts(name, xs[b], b, mld, S[b], nbBlocks)[l])
        print('nbBlocks %s level %d: the count changes for signals %s' % (nbBlocks, l, [b for b, c in zip(four, changed) if c]))
        assert sum(changed) >= 3, (nbBlocks, l, changed)
