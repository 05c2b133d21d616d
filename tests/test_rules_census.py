"""The rows of tests/rules_util.py can tell a per-signal stop rule from a batch one (no GPU: the CPU oracle encodes every signal
with its own scalars).  A row that fails here has the wrong inputs, not the wrong kernel: the GPU tests of tests/test_gpu_rules.py
compare bit for bit, but a row in which every signal would stop at the same place under any of the row's values would pass them
with one rule for the whole batch."""
import numpy as np
import pytest

from tests import rules_util as ru

RULE_STOPS = {'nbNonzeroCoefs': 'nnz', 'toleranceSnr': 'snr', 'toleranceResidualScale': 'residual_scale'}


def _encode(name, b, **override):
    from oracle import hsc_oracle as orc
    xs, D, w = ru.row_inputs(name)
    kw = ru.signal_kw(name, b)
    kw.update(override)
    return orc.cmp_encode(xs[b], D, weights=w, **kw)[2]


def _same_events(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ('t', 'k', 'c'))


def _is_prefix(a, b):
    n = min(len(a['t']), len(b['t']))
    return all(np.array_equal(a[key][:n], b[key][:n]) for key in ('t', 'k', 'c'))


@pytest.fixture(scope='module')
def own():
    """name -> the oracle's trace of every signal under its own scalars, computed once."""
    return {name: [_encode(name, b) for b in range(len(ru.ROWS[name][1]))] for name in ru.ROWS}


@pytest.mark.parametrize('name', sorted(ru.ROWS))
def test_signals_of_a_row_stop_differently(name, own):
    infos = own[name]
    stops = set(i['stop'] for i in infos)
    counts = [len(i['t']) for i in infos]
    assert len(stops) >= 2 or len(set(counts)) >= 2, (stops, counts)
    assert len(set(counts)) >= 4, counts             # (six signals: most of them apart, not one odd one out)


@pytest.mark.parametrize('name', sorted(ru.ROWS))
def test_no_signal_stops_for_a_trivial_reason(name, own):
    """Every signal stops on one of the rules the row gives per signal, not on an empty selection or a vanished residual, and not at
    its first atom unless its own nbNonzeroCoefs says 1; and under its neighbour's values it would stop somewhere else."""
    per_signal = ru.ROWS[name][4]
    B = len(ru.ROWS[name][1])
    for b, info in enumerate(own[name]):
        assert info['stop'] in [RULE_STOPS[key] for key in per_signal], (b, info['stop'])
        first_atom_asked = per_signal.get('nbNonzeroCoefs', [None] * B)[b] == 1
        assert len(info['t']) >= 2 or first_atom_asked, b
        if 'nbNonzeroCoefs' in per_signal and info['stop'] == 'nnz':
            assert info['nnz'] == per_signal['nbNonzeroCoefs'][b]
        nb = (b + 1) % B
        theirs = {key: vals[nb] for key, vals in per_signal.items()}
        if theirs == {key: vals[b] for key, vals in per_signal.items()}:
            continue
        other = _encode(name, b, **theirs)
        assert other['stop'] != info['stop'] or not _same_events(other, info), (b, nb)


@pytest.mark.parametrize('name', sorted(n for n in ru.ROWS if ru.is_blocked(n) and 'toleranceSnr' in ru.ROWS[n][4]))
def test_blocked_snr_rows_reach_the_weak_atom_filter(name, own):
    """Blocked rounds drop the atoms of a round whose window energy lies below a threshold that follows toleranceSnr
    (modeling.py:1090-1099): with its neighbour's toleranceSnr a signal then takes ANOTHER path, not a shorter or longer stretch
    of the same one.  At least one signal of the row must show that, or the row would pass with the batch's threshold in the filter."""
    per_signal = ru.ROWS[name][4]
    B = len(ru.ROWS[name][1])
    forked = []
    for b, info in enumerate(own[name]):
        other = _encode(name, b, toleranceSnr=per_signal['toleranceSnr'][(b + 1) % B])
        if not _is_prefix(other, info):
            forked.append(b)
    assert forked, 'no signal of the row leaves its path under its neighbour\'s toleranceSnr'


def test_quad_row_has_four_rules_in_one_workgroup():
    """The four-signal loop on six signals: one full workgroup whose four signals stop on four different nbNonzeroCoefs, and one
    partly filled (the shape tests/test_gpu_rules.py relies on for its row f32_quad_forced_l0)."""
    _, lengths, env, _, per_signal, expected, _ = ru.ROWS['f32_quad_forced_l0']
    assert expected.endswith('_x4') and env['HSCMP_MFMA_QUAD'] == '1'
    assert len(lengths) == 6 and len(set(per_signal['nbNonzeroCoefs'][:4])) == 4
