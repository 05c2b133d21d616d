"""hscmp_encode_batch_from_level_rules: the level hand-off on the device with stop rules per signal.

Two contexts.  Level 0 (6 atoms of 8 taps, float64) encodes five planted signals of 64 to 300 samples with an nbNonzeroCoefs each
(hscmp_encode_batch_rules); level 1 (their 6 singletons and 5 composite atoms, tests/test_gpu_ragged_levels.py's dictionary
builder) takes signals 1 .. 3 of it with a table of its own.  Per signal and bit for bit -- all eight stats with the stop reason,
slots, events, residual, both energies -- the result must equal the chain of two single-signal encodes with the signal's values in
the scalar fields, and the CPU oracle on the level-0 result.

This module holds the checks and no test of its own: ROWS (at the end) lists them, and the one GPU test of
tests/test_gpu_rules_hierarchy.py runs every row and names each that fails -- a row takes milliseconds, and the suite's item
count stays what it was but for that one test (as tests/test_gpu_rules.py groups its rows)."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_ragged_levels import F64, _all_results, _check_against_oracle, _level_dictionary, _same

LENGTHS = [300, 64, 200, 150, 120]
L0_LEVEL0 = [24, 5, 16, 12, 10]
FIRST, COUNT = 1, 3
EPS = float(np.finfo(F64).eps)
CAP = 2048
# name: (the shared arguments, the arguments per signal of the sub-range).  The oracle's stop reasons, signals 1, 2, 3: 'l0' nnz at 3, 9
# and 6 atoms; 'blocked_snr' snr at 3, 14, 9; 'scale' residual_scale at 4, 16, 12; 'all' nnz (4), snr (10), nnz (7)
KINDS = {
    'l0': ({}, dict(nbNonzeroCoefs=[3, 9, 6])),
    'blocked_snr': (dict(nbBlocks=4), dict(toleranceSnr=[6.0, 14.0, 10.0])),
    'scale': ({}, dict(toleranceResidualScale=[0.8, 0.3, 0.5])),
    'all': (dict(nbBlocks=4), dict(nbNonzeroCoefs=[4, 30, 7], toleranceSnr=[20.0, 9.0, 20.0], toleranceResidualScale=[0.05, 0.05, 0.6])),
}
_PROBLEM = []


def _problem():
    if not _PROBLEM:
        import hsc_amd.synth as synth
        D0 = synth.make_dictionary(6, 8, seed=2, dtype=F64)
        xs = [synth.make_signal(D0, n, i, kind='planted', nb_atoms=n // 10, noise=0.05, seed=2, dtype=F64) for i, n in enumerate(LENGTHS)]
        _PROBLEM.append((xs, D0[:, :, np.newaxis], _level_dictionary(1, 6, 5, 8, F64)))
    return _PROBLEM[0]


def _signal_kw(kind, i):
    shared, per_signal = KINDS[kind]
    kw = dict(shared)
    kw.update((key, vals[i]) for key, vals in per_signal.items())
    return kw


def _rules_params(kind, **kw):
    from hsc_amd import _native
    shared, per_signal = KINDS[kind]
    return _native.make_rules(COUNT, **per_signal), _native.make_params(eps=EPS, maxEvents=kw.pop('maxEvents', CAP), **dict(shared, **kw))


def _padded_signals(xs):
    x = np.zeros((len(xs), max(len(s) for s in xs), 1), dtype=F64)
    for b, s in enumerate(xs):
        x[b, :len(s), 0] = s
    return x, np.array([len(s) for s in xs], dtype=np.int32)


class _Chain(object):
    """Level 0 encoded (five signals, an nbNonzeroCoefs each) and a level-1 engine with its dictionary."""

    def __init__(self, uniform=False):
        from hsc_amd import _native
        xs, D0, D1 = _problem()
        # (uniform: every signal cut, or padded with zeros, to 120 samples)
        self.xs = [np.pad(s[:120], (0, 120 - len(s[:120]))) for s in xs] if uniform else xs
        self.lens = np.array([len(s) for s in self.xs], dtype=np.int32)
        self.prev, self.lvl = _native.Engine(0), _native.Engine(0)
        try:
            self.prev.set_dictionary(D0)
            self.lvl.set_dictionary(D1, dtype=F64)
            x, lens = _padded_signals(self.xs)
            if uniform:                         # (a plain batch with the largest nbNonzeroCoefs: a uniform previous level)
                self.prev.encode_batch(x, _native.make_params(eps=EPS, maxEvents=CAP, nbNonzeroCoefs=10))
                assert not self.prev.last_variant().endswith(('_ragged', '_rules'))
            else:
                self.prev.encode_batch_rules(x, lens, _native.make_rules(len(xs), nbNonzeroCoefs=L0_LEVEL0), _native.make_params(eps=EPS, maxEvents=CAP))
        except Exception:
            self.close()
            raise

    def sub_lens(self):
        return self.lens[FIRST:FIRST + COUNT]

    def results(self):
        return _all_results(self.lvl, self.sub_lens())[0]

    def close(self):
        self.prev.close(); self.lvl.close()


def _run_out(eng, rounds):
    from hsc_amd import _native
    for _ in range(10000):
        if not (eng.fetch_stats()[:, _native.STAT_STOP] == _native.STOP_RUNNING).any():
            return
        eng.continue_rounds(rounds)
    raise AssertionError('the batch does not stop')


def _single_chains(kind, xs, level0_l0):
    """Signals FIRST .. FIRST + COUNT - 1, each alone through two fresh contexts with its own scalars; also the dense level-1 inputs."""
    from hsc_amd import _native
    from hsc_amd.modeling import _slots_to_csc
    _, D0, D1 = _problem()
    out, inputs = [], []
    e0, e1 = _native.Engine(0), _native.Engine(0)
    try:
        e0.set_dictionary(D0)
        e1.set_dictionary(D1, dtype=F64)
        for i in range(COUNT):
            s = xs[FIRST + i]
            e0.encode_batch(s.reshape((1, -1, 1)), _native.make_params(eps=EPS, maxEvents=CAP, nbNonzeroCoefs=level0_l0[FIRST + i]))
            st, sk, sa = e0.fetch_slots()
            ns = int(e0.fetch_stats()[0, _native.STAT_SLOTS])
            inputs.append(_slots_to_csc(st[0], sk[0], sa[0], ns, (len(s), D0.shape[0]), 1e-16).toarray())
            e1.encode_batch_from_level(e0, 0, 1, 1e-16, _native.make_params(eps=EPS, maxEvents=CAP, **_signal_kw(kind, i)))
            assert not e1.last_variant().endswith(('_ragged', '_rules'))
            out.append(_all_results(e1, [len(s)])[0][0])
    finally:
        e0.close(); e1.close()
    return out, inputs


def _sub_range_equals_single_signal_chains(kind):
    from oracle import hsc_oracle as orc
    from hsc_amd import _native
    D1 = _problem()[2]
    chain = _Chain()
    try:
        chain.lvl.encode_batch_from_level(chain.prev, FIRST, COUNT, 1e-16, _native.make_params(eps=EPS, maxEvents=CAP, **_signal_kw(kind, 0)))
        ragged_variant = chain.lvl.last_variant()
        assert ragged_variant.endswith('_ragged')
        rules, params = _rules_params(kind)
        chain.lvl.encode_batch_from_level_rules(chain.prev, FIRST, COUNT, 1e-16, rules, params)
        assert chain.lvl.last_variant() == ragged_variant + '_rules'
        got = chain.results()
        assert len(set(len(g['t']) for g in got)) == COUNT, 'the three signals stop at the same place'
        single, inputs = _single_chains(kind, chain.xs, L0_LEVEL0)
        for i in range(COUNT):
            _same(got[i], single[i])
            _check_against_oracle(got[i], orc.cmp_encode(inputs[i], D1, **_signal_kw(kind, i)), int(chain.sub_lens()[i]), D1.shape[0])
    finally:
        chain.close()


def _uniform_previous_level_gets_count_lengths_of_T():
    from hsc_amd import _native
    chain = _Chain(uniform=True)
    try:
        for kind in ('l0', 'blocked_snr'):
            rules, params = _rules_params(kind)
            chain.lvl.encode_batch_from_level_rules(chain.prev, FIRST, COUNT, 1e-16, rules, params)
            assert chain.lvl.last_variant().endswith('_ragged_rules')
            got = chain.results()
            single, _ = _single_chains(kind, chain.xs, [10] * 5)
            for i in range(COUNT):
                _same(got[i], single[i])
    finally:
        chain.close()


def _regrowth_stepping_and_stop_signal_keep_every_signals_rules():
    from hsc_amd import _native
    chain = _Chain()
    lvl, prev = chain.lvl, chain.prev
    try:
        for kind in ('l0', 'scale', 'all'):
            rules, params = _rules_params(kind)
            lvl.encode_batch_from_level_rules(prev, FIRST, COUNT, 1e-16, rules, params)
            one = chain.results()
            # a start capacity of 8 events: grow and resume until no signal stops on capacity
            rules, params = _rules_params(kind, maxEvents=8)
            lvl.encode_batch_from_level_rules(prev, FIRST, COUNT, 1e-16, rules, params)
            del rules                                     # (the context keeps its own copy of the table)
            stops = lvl.fetch_stats()[:, _native.STAT_STOP]
            assert (stops == _native.STOP_CAPACITY).any() and (stops != _native.STOP_CAPACITY).any(), (kind, stops)
            cap = 8
            while (lvl.fetch_stats()[:, _native.STAT_STOP] == _native.STOP_CAPACITY).any():
                cap *= 4
                assert cap <= CAP
                lvl.grow_events(cap)
                lvl.continue_rounds(0)
            for a, b in zip(chain.results(), one):
                _same(a, b)
            # one round per launch
            rules, params = _rules_params(kind, maxRounds=1)
            lvl.encode_batch_from_level_rules(prev, FIRST, COUNT, 1e-16, rules, params)
            _run_out(lvl, 1)
            for a, b in zip(chain.results(), one):
                _same(a, b)
        # hscmp_stop_signal: the others go on to their own rules
        rules, params = _rules_params('scale')
        lvl.encode_batch_from_level_rules(prev, FIRST, COUNT, 1e-16, rules, params)
        one = chain.results()
        rules, params = _rules_params('scale', maxRounds=2)
        lvl.encode_batch_from_level_rules(prev, FIRST, COUNT, 1e-16, rules, params)
        lvl.stop_signal(1)                                # (16 rounds alone: two rounds in, far from its rule)
        _run_out(lvl, 2)
        two = chain.results()
        for i in (0, 2):
            _same(two[i], one[i])
        assert _native.STOP_NAMES[int(two[1]['stats'][_native.STAT_STOP])] == 'callback'
        n = len(two[1]['t'])
        assert n == 2 and all(np.array_equal(two[1][key], one[1][key][:n]) for key in ('t', 'k', 'c'))
    finally:
        chain.close()


def _the_table_does_not_leak_into_the_next_chained_batch():
    from hsc_amd import _native
    scalar_params = _native.make_params(eps=EPS, maxEvents=CAP, nbNonzeroCoefs=11, toleranceSnr=12.0, nbBlocks=4)
    fresh = _Chain()
    try:
        fresh.lvl.encode_batch_from_level(fresh.prev, FIRST, COUNT, 1e-16, scalar_params)
        variant = fresh.lvl.last_variant()
        want = fresh.results()
    finally:
        fresh.close()
    chain = _Chain()
    try:
        rules, params = _rules_params('all')
        chain.lvl.encode_batch_from_level_rules(chain.prev, FIRST, COUNT, 1e-16, rules, params)
        assert chain.lvl.last_variant().endswith('_rules')
        chain.lvl.encode_batch_from_level(chain.prev, FIRST, COUNT, 1e-16, scalar_params)
        assert chain.lvl.last_variant() == variant and not variant.endswith('_rules')
        for a, b in zip(chain.results(), want):
            _same(a, b)
    finally:
        chain.close()


def _raw_rules(l0=None, snr=None, scale=None):
    """A hscmp_signal_rules past make_rules' checks (the library's own are under test)."""
    from hsc_amd import _native
    r = _native.HscmpSignalRules()
    r.arrays = {}
    for field, vals, dt in (('nb_nonzero_coefs', l0, np.int32), ('tolerance_snr', snr, np.float64), ('tolerance_residual_scale', scale, np.float64)):
        if vals is not None:
            r.arrays[field] = np.ascontiguousarray(vals, dtype=dt)
            assert r.arrays[field].shape == (COUNT,)
            setattr(r, field, r.arrays[field].ctypes.data)
    return r


def _refusals_leave_the_held_batch_and_its_table():
    from hsc_amd import _native
    chain = _Chain()
    lvl, prev = chain.lvl, chain.prev
    empty = _native.Engine(0)
    try:
        rules, params = _rules_params('all')
        lvl.encode_batch_from_level_rules(prev, FIRST, COUNT, 1e-16, rules, params)
        whole = chain.results()
        rules2, params2 = _rules_params('all', maxRounds=1)
        lvl.encode_batch_from_level_rules(prev, FIRST, COUNT, 1e-16, rules2, params2)
        before = chain.results()
        who = 'hscmp_encode_batch_from_level_rules'

        def refused(code, *words, rules=rules, first=FIRST, count=COUNT, method=None, previous=prev):
            if method is not None:
                lvl.set_method(method)
            try:
                with pytest.raises(_native.HscmpError) as e:
                    lvl.encode_batch_from_level_rules(previous, first, count, 1e-16, rules, params)
            finally:
                lvl.set_method(_native.METHOD_CMP)
            assert e.value.code == code, str(e.value)
            for word in (who,) + words:
                assert word in str(e.value), str(e.value)
            for a, b in zip(chain.results(), before):
                _same(a, b)

        refused(_native.ERR_INVALID, 'no rule has an array: use hscmp_encode_batch_from_level', rules=None)
        refused(_native.ERR_INVALID, 'no rule has an array: use hscmp_encode_batch_from_level', rules=_native.HscmpSignalRules())
        refused(_native.ERR_INVALID, 'signal 2', 'nb_nonzero_coefs is -1', rules=_raw_rules(l0=[1, 2, -1]))
        refused(_native.ERR_INVALID, 'signal 1', 'tolerance_snr is nan', rules=_raw_rules(snr=[1.0, float('nan'), 3.0]))
        refused(_native.ERR_INVALID, 'signal 0', 'tolerance_snr is -1', rules=_raw_rules(l0=[1, 1, 1], snr=[-1.0, 2.0, 3.0]))
        refused(_native.ERR_INVALID, 'signal 2', 'tolerance_residual_scale is nan', rules=_raw_rules(scale=[0.1, 0.1, float('nan')]))
        refused(_native.ERR_INVALID, 'signal 1', 'tolerance_residual_scale is -0.1', rules=_raw_rules(scale=[0.1, -0.1, 0.1]))
        refused(_native.ERR_UNSUPPORTED, 'the LoCOMP loop has no per-signal stop rules', method=_native.METHOD_LOCOMP)
        # what hscmp_encode_batch_from_level refuses
        refused(_native.ERR_INVALID, 'bad signal range', first=3, count=3)
        refused(_native.ERR_INVALID, 'bad signal range', count=0)
        empty.set_dictionary(_problem()[1])
        refused(_native.ERR_STATE, 'the previous level has no results', previous=empty)
        # (a NULL previous level, past the Python wrapper)
        rc = lvl._lib.hscmp_encode_batch_from_level_rules(lvl._h, None, FIRST, COUNT, ctypes.c_double(1e-16), ctypes.byref(rules), ctypes.byref(params))
        assert rc == _native.ERR_INVALID and b'NULL context' in lvl._lib.hscmp_last_error(lvl._h)
        for a, b in zip(chain.results(), before):
            _same(a, b)
        # the held rules batch resumes with its own table
        _run_out(lvl, 1)
        for a, b in zip(chain.results(), whole):
            _same(a, b)
    finally:
        chain.close(); empty.close()


# (name, check) of every row above
ROWS = [('sub_range_equals_single_signal_chains[%s]' % kind, lambda kind=kind: _sub_range_equals_single_signal_chains(kind)) for kind in sorted(KINDS)] + [
    ('uniform_previous_level_gets_count_lengths_of_T', _uniform_previous_level_gets_count_lengths_of_T),
    ('regrowth_stepping_and_stop_signal_keep_every_signals_rules', _regrowth_stepping_and_stop_signal_keep_every_signals_rules),
    ('the_table_does_not_leak_into_the_next_chained_batch', _the_table_does_not_leak_into_the_next_chained_batch),
    ('refusals_leave_the_held_batch_and_its_table', _refusals_leave_the_held_batch_and_its_table),
]
