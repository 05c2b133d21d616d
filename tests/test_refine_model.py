"""tools/refine_model.py, the numpy restatement of the bound loop's selection rule, at a small shape (T = 4096, K = 64): every
bound it forms is at least the exact score, and every selection refines at least once (after the bound pass and behind the
bound loop every row holds a bound, so a winner has to be refined before it is exact -- if not by this selection, by an
earlier one, which then refined in its place)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


@pytest.mark.parametrize('kind', ['planted', 'noise'])
@pytest.mark.parametrize('products', [(1, 1), (1, 3)])
def test_bounds_hold_and_every_selection_refines(kind, products):
    import hsc_amd.synth as synth
    import refine_model
    T, K, W, L0 = 4096, 64, 64, 48
    D = synth.make_dictionary(K, W, seed=2)
    x = np.asarray(synth.make_signal(D, T, 0, kind=kind, nb_atoms=L0, seed=2), dtype=np.float32).reshape(-1)
    m = refine_model.Model(D)
    per_sel, from_memory, rate = m.run(x, L0, *products)
    print('%s init %d / loop %d: refines per selection %.3f, from memory %.3f, hit rates %s' % ((kind,) + products + (per_sel, from_memory, rate)))
    assert m.min_margin >= 0.0
    assert per_sel >= 1.0
    assert 0.0 <= from_memory <= 1.0 and all(0.0 <= v <= 1.0 for v in rate.values())
