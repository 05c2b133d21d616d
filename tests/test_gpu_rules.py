"""Stop rules per signal (hscmp_encode_batch_rules): nbNonzeroCoefs, toleranceSnr and
toleranceResidualScale as one value per signal of a batch.

Every row of tests/rules_util.py (the matrix of tests/test_gpu_ragged.py; tests/test_rules_census.py shows on the CPU that its
signals do stop at different places) runs as a rules batch.  Each signal must give, bit for bit, what the same engine gives it alone
with its own scalars, what the CPU oracle gives it, and -- where its values equal the scalars -- what the batch gives it when it is
encoded with one scalar per rule: events, coefficient slots, stats, residual and energies."""
import ctypes

import numpy as np
import pytest

from tests import rules_util as ru
from tests.test_gpu_ragged import F32, _all_results, _check_against_oracle, _padded, _same, _signal_results

pytestmark = pytest.mark.gpu

CAP = 2048


def _row(name, monkeypatch):
    dtype, lengths, env, shared, per_signal, expected, _ = ru.ROWS[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    xs, D, w = ru.row_inputs(name)
    x, lens = _padded(xs)
    uniform = len(set(lengths)) == 1
    return xs, D, w, x, lens, uniform, shared, per_signal, expected, float(np.finfo(dtype).eps)


def _rules_params(per_signal, shared, B, eps, **kw):
    from hsc_amd import _native
    return _native.make_rules(B, **per_signal), _native.make_params(eps=eps, maxEvents=kw.pop('maxEvents', CAP), **dict(shared, **kw))


def _each(names, body, monkeypatch):
    """body(name, monkeypatch) for every row, each under its own environment; every failing row is named at the end.  (One test
    per group of rows, not one per row: a row takes milliseconds, and the suite's item count stays what a reader can scan.)"""
    failed = []
    for name in names:
        with monkeypatch.context() as m:
            try:
                body(name, m)
            except AssertionError as e:
                failed.append('%s: %s' % (name, (str(e).splitlines() or [repr(e)])[0]))
    assert not failed, '%d of %d rows failed:\n%s' % (len(failed), len(names), '\n'.join(failed))


def _run_out(eng, rounds):
    from hsc_amd import _native
    for _ in range(10000):
        if not (eng.fetch_stats()[:, _native.STAT_STOP] == _native.STOP_RUNNING).any():
            return
        eng.continue_rounds(rounds)
    raise AssertionError('the batch does not stop')


def test_rules_rows(monkeypatch):
    """Every row of tests/rules_util.py."""
    _each(sorted(ru.ROWS), _rules_row, monkeypatch)


def _rules_row(name, monkeypatch):
    from hsc_amd import _native
    xs, D, w, x, lens, uniform, shared, per_signal, expected, eps = _row(name, monkeypatch)
    B, K = len(xs), D.shape[0]
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        # the batch with ONE scalar per rule (signal 1's): its plan is the rules batch's, and the signals with these values must agree
        one = 1
        scalar_params = _native.make_params(eps=eps, maxEvents=CAP, **ru.signal_kw(name, one))
        if uniform:
            eng.encode_batch(x, scalar_params)
            ragged_variant = eng.last_variant() + '_ragged'
        else:
            eng.encode_batch_ragged(x, lens, scalar_params)
            ragged_variant = eng.last_variant()
        if expected is not None:
            assert ragged_variant == expected + '_ragged'
        scalar, _ = _all_results(eng, lens)

        rules, params = _rules_params(per_signal, shared, B, eps)
        eng.encode_batch_rules(x, None if uniform else lens, rules, params)
        assert eng.last_variant() == ragged_variant + '_rules'
        got, raw = _all_results(eng, lens)
        for b, Tb in enumerate(lens):
            assert not raw[b, Tb:].any(), 'the residual above the signal length is not zero'
        shared_values = [b for b in range(B) if ru.signal_kw(name, b) == ru.signal_kw(name, one)]
        assert one in shared_values
        for b in shared_values:
            _same(got[b], scalar[b])
        for b, s in enumerate(xs):
            kw = ru.signal_kw(name, b)
            eng.encode_batch(s.reshape((1, -1, 1)), _native.make_params(eps=eps, maxEvents=CAP, **kw))
            _same(got[b], _signal_results(eng, 0, len(s)))
            _check_against_oracle(got[b], s, D, w, kw, K)
    finally:
        eng.close()


def test_device_entry_and_nan_padding(monkeypatch):
    """The device-pointer entry equals the host one, and rows above a signal's length are never read."""
    _each(['f32_default_l0', 'f32_blocked_rp_snr', 'f32_force_generic_blocked_snr', 'f64_default_l0', 'f32_uniform_blocked_l0_and_snr'],
          _device_entry_and_nan_padding, monkeypatch)


def _device_entry_and_nan_padding(name, monkeypatch):
    import torch
    from hsc_amd import _native
    xs, D, w, x, lens, uniform, shared, per_signal, _, eps = _row(name, monkeypatch)
    xn, _ = _padded(xs, fill=np.nan)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        rules, params = _rules_params(per_signal, shared, len(xs), eps)
        eng.encode_batch_rules(x, None if uniform else lens, rules, params)
        variant = eng.last_variant()
        ref, raw0 = _all_results(eng, lens)
        xd = torch.from_numpy(xn).to('cuda:0')
        torch.cuda.synchronize()
        eng.encode_batch_rules_device(xd.data_ptr(), xd.shape[0], xd.shape[1], None if uniform else lens, rules, params)
        eng.synchronize()
        assert eng.last_variant() == variant and variant.endswith('_ragged_rules')
        dev, raw = _all_results(eng, lens)
        assert np.array_equal(raw, raw0)
        for a, b in zip(dev, ref):
            _same(a, b)
    finally:
        eng.close()


def test_resuming_keeps_every_signals_rules(monkeypatch):
    """hscmp_continue, hscmp_grow_events and hscmp_stop_signal on a rules batch: the table outlives the encode."""
    _each(['f32_default_l0', 'f32_quad_forced_l0', 'f32_blocked_rp_snr', 'f32_blocked_no_rp_snr', 'f32_force_generic_l0', 'f32_blocked_scale',
           'f32_blocked_l0_and_snr'], _resume_matches_one_launch, monkeypatch)
    _each(['f32_default_l0', 'f32_quad_forced_l0', 'f32_blocked_l0_and_snr'], _capacity_regrowth_reproduces_the_uninterrupted_run, monkeypatch)
    _each(['f32_default_l0'], _stop_signal_leaves_the_other_signals_rules, monkeypatch)


def _resume_matches_one_launch(name, monkeypatch):
    """max_rounds = 2 and hscmp_continue until every signal stopped: one launch's results."""
    from hsc_amd import _native
    xs, D, w, x, lens, uniform, shared, per_signal, _, eps = _row(name, monkeypatch)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        rules, params = _rules_params(per_signal, shared, len(xs), eps)
        eng.encode_batch_rules(x, lens, rules, params)
        variant = eng.last_variant()
        one, raw1 = _all_results(eng, lens)
        rules, params = _rules_params(per_signal, shared, len(xs), eps, maxRounds=2)
        eng.encode_batch_rules(x, lens, rules, params)
        del rules                                         # (the context keeps its own copy of the table)
        _run_out(eng, 2)
        assert eng.last_variant() == variant
        two, raw2 = _all_results(eng, lens)
        assert np.array_equal(raw1, raw2)
        for a, b in zip(two, one):
            _same(a, b)
    finally:
        eng.close()


def _capacity_regrowth_reproduces_the_uninterrupted_run(name, monkeypatch):
    """maxEvents = 16 under an nbNonzeroCoefs array that reaches 60: signals stop on the capacity of their event lists, and
    hscmp_grow_events + hscmp_continue take each of them on to its own nbNonzeroCoefs."""
    from hsc_amd import _native
    xs, D, w, x, lens, uniform, shared, per_signal, _, eps = _row(name, monkeypatch)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        rules, params = _rules_params(per_signal, shared, len(xs), eps)
        eng.encode_batch_rules(x, lens, rules, params)
        one, _ = _all_results(eng, lens)
        rules, params = _rules_params(per_signal, shared, len(xs), eps, maxEvents=16)
        eng.encode_batch_rules(x, lens, rules, params)
        stops = eng.fetch_stats()[:, _native.STAT_STOP]
        assert (stops == _native.STOP_CAPACITY).any() and (stops != _native.STOP_CAPACITY).any()
        eng.grow_events(CAP)
        eng.continue_rounds(0)
        two, _ = _all_results(eng, lens)
        for a, b in zip(two, one):
            _same(a, b)
    finally:
        eng.close()


def _stop_signal_leaves_the_other_signals_rules(name, monkeypatch):
    from hsc_amd import _native
    xs, D, w, x, lens, uniform, shared, per_signal, _, eps = _row(name, monkeypatch)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        rules, params = _rules_params(per_signal, shared, len(xs), eps)
        eng.encode_batch_rules(x, lens, rules, params)
        one, _ = _all_results(eng, lens)
        rules, params = _rules_params(per_signal, shared, len(xs), eps, maxRounds=3)
        eng.encode_batch_rules(x, lens, rules, params)
        eng.stop_signal(1)                                # (nbNonzeroCoefs 60: three rounds in, far from its rule)
        _run_out(eng, 3)
        two, _ = _all_results(eng, lens)
        for b in range(len(xs)):
            if b != 1:
                _same(two[b], one[b])
        assert _native.STOP_NAMES[int(two[1]['stats'][_native.STAT_STOP])] == 'callback'
        n = len(two[1]['t'])
        assert n == 3 and all(np.array_equal(two[1][key], one[1][key][:n]) for key in ('t', 'k', 'c'))
    finally:
        eng.close()


def test_table_lifetime_and_refusals(monkeypatch):
    """The table belongs to its batch: it does not leak into the next one, and no refusal touches the batch the context holds."""
    for body in (_table_does_not_leak_into_the_next_batch, _refusals_leave_the_previous_batch):
        with monkeypatch.context() as m:
            body(m)
    _a_set_of_dictionaries_refuses_rules()


def _table_does_not_leak_into_the_next_batch(monkeypatch):
    """A plain and a ragged encode behind a rules batch give what they give on a fresh engine: every signal stops on the scalars."""
    from hsc_amd import _native
    name = 'f32_blocked_l0_and_snr'
    xs, D, w, x, lens, uniform, shared, per_signal, _, eps = _row(name, monkeypatch)
    scalar_params = _native.make_params(eps=eps, maxEvents=CAP, nbNonzeroCoefs=40, toleranceSnr=18.0, **shared)
    full = np.full(len(xs), x.shape[1], dtype=np.int32)
    fresh = _native.Engine(0)
    try:
        fresh.set_dictionary(D, w)
        fresh.encode_batch(x, scalar_params)
        plain_variant = fresh.last_variant()
        plain, _ = _all_results(fresh, full)
        fresh.encode_batch_ragged(x, lens, scalar_params)
        ragged_variant = fresh.last_variant()
        ragged, _ = _all_results(fresh, lens)
    finally:
        fresh.close()
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        rules, params = _rules_params(per_signal, shared, len(xs), eps)
        for check_ragged in (False, True):
            eng.encode_batch_rules(x, lens, rules, params)
            assert eng.last_variant().endswith('_rules')
            if check_ragged:
                eng.encode_batch_ragged(x, lens, scalar_params)
                assert eng.last_variant() == ragged_variant
                got, _ = _all_results(eng, lens)
            else:
                eng.encode_batch(x, scalar_params)
                assert eng.last_variant() == plain_variant
                got, _ = _all_results(eng, full)
            for a, b in zip(got, ragged if check_ragged else plain):
                _same(a, b)
    finally:
        eng.close()


def _raw_rules(B, l0=None, snr=None, scale=None):
    """A hscmp_signal_rules past make_rules' checks (the library's own are under test)."""
    from hsc_amd import _native
    r = _native.HscmpSignalRules()
    r.arrays = {}
    for field, vals, dt in (('nb_nonzero_coefs', l0, np.int32), ('tolerance_snr', snr, np.float64), ('tolerance_residual_scale', scale, np.float64)):
        if vals is not None:
            r.arrays[field] = np.ascontiguousarray(vals, dtype=dt)
            assert r.arrays[field].shape == (B,)
            setattr(r, field, r.arrays[field].ctypes.data)
    return r


def _refusals_leave_the_previous_batch(monkeypatch):
    """Every refusal of hscmp_encode_batch_rules answers its documented code before anything is queued: the batch the context holds
    stays fetchable, and a rules batch stays resumable with ITS table."""
    from hsc_amd import _native
    name = 'f32_default_l0'
    xs, D, w, x, lens, uniform, shared, per_signal, _, eps = _row(name, monkeypatch)
    B = len(xs)
    eng = _native.Engine(0)
    try:
        eng.set_dictionary(D, w)
        rules, params = _rules_params(per_signal, shared, B, eps)
        eng.encode_batch_rules(x, lens, rules, params)
        whole, _ = _all_results(eng, lens)
        rules2, params2 = _rules_params(per_signal, shared, B, eps, maxRounds=2)
        eng.encode_batch_rules(x, lens, rules2, params2)
        before, _ = _all_results(eng, lens)

        def refused(code, *words, rules=rules, lengths=lens, method=None):
            if method is not None:
                eng.set_method(method)
            try:
                with pytest.raises(_native.HscmpError) as e:
                    eng.encode_batch_rules(x, lengths, rules, params)
            finally:
                eng.set_method(_native.METHOD_CMP)
            assert e.value.code == code, str(e.value)
            for word in words:
                assert word in str(e.value), str(e.value)
            after, _ = _all_results(eng, lens)
            for a, b in zip(after, before):
                _same(a, b)

        refused(_native.ERR_INVALID, 'use hscmp_encode_batch_ragged', rules=None)
        refused(_native.ERR_INVALID, 'use hscmp_encode_batch_ragged', rules=_native.HscmpSignalRules())
        refused(_native.ERR_INVALID, 'signal 2', 'nb_nonzero_coefs', rules=_raw_rules(B, l0=[1, 2, -1, 4, 5, 6]))
        refused(_native.ERR_INVALID, 'signal 5', 'tolerance_snr', rules=_raw_rules(B, snr=[1.0, 2.0, 3.0, 4.0, 5.0, float('nan')]))
        refused(_native.ERR_INVALID, 'signal 0', 'tolerance_snr', rules=_raw_rules(B, l0=[1] * B, snr=[-1.0, 2.0, 3.0, 4.0, 5.0, 6.0]))
        refused(_native.ERR_INVALID, 'signal 3', 'tolerance_residual_scale', rules=_raw_rules(B, scale=[0.1, 0.1, 0.1, float('nan'), 0.1, 0.1]))
        refused(_native.ERR_INVALID, 'signal 4', 'tolerance_residual_scale', rules=_raw_rules(B, scale=[0.1, 0.1, 0.1, 0.1, -0.1, 0.1]))
        refused(_native.ERR_UNSUPPORTED, 'LoCOMP', method=_native.METHOD_LOCOMP)
        bad = lens.copy()
        bad[1] = x.shape[1] + 1                           # (encode_common's check, still in front of the batch)
        refused(_native.ERR_INVALID, 'signal 1', lengths=bad)
        # the held rules batch resumes with its own table
        _run_out(eng, 2)
        done, _ = _all_results(eng, lens)
        for a, b in zip(done, whole):
            _same(a, b)
    finally:
        eng.close()


def _a_set_of_dictionaries_refuses_rules():
    from hsc_amd import _native
    xs, D, _ = ru.row_inputs('f32_default_l0')
    x = np.stack([s[:700] for s in xs if len(s) >= 700])[:, :, None]
    B = x.shape[0]
    eps = float(np.finfo(F32).eps)
    eng = _native.Engine(0)
    try:
        eng.set_dictionaries(np.stack([D, D[::-1].copy()]))
        params = _native.make_params(eps=eps, maxEvents=256, nbNonzeroCoefs=10)
        eng.encode_batch_multi(x, np.arange(B, dtype=np.int32) % 2, params)
        before, _ = _all_results(eng, [700] * B)
        with pytest.raises(_native.HscmpError) as e:
            eng.encode_batch_rules(x, None, _native.make_rules(B, nbNonzeroCoefs=list(range(1, B + 1))), params)
        assert e.value.code == _native.ERR_STATE and 'set of 2 dictionaries' in str(e.value)
        after, _ = _all_results(eng, [700] * B)
        for a, b in zip(after, before):
            _same(a, b)
    finally:
        eng.close()


def _reference_signal(single, s, D, **kw):
    coef, residual = single.computeCoefficients(s, D, **kw)
    return coef, residual, single.lastResult


def test_modeling_accepts_a_sequence_per_rule():
    for form in ('uniform', 'list', 'lengths'):
        _modeling_accepts_a_sequence_per_rule(form)
    _modeling_stop_condition_runs_round_by_round()


def _modeling_accepts_a_sequence_per_rule(form):
    """computeCoefficientsBatch / encodeBatch with sequences: per signal what computeCoefficients gives it alone with its scalars, in
    the shapes of the input's form; the default maxEvents (2 * max(nbNonzeroCoefs) + 64) and a small one that has to grow."""
    from hsc_amd.modeling import ConvolutionalMatchingPursuit, ConvolutionalSparseCoder
    name = 'f32_uniform_blocked_l0_and_snr' if form == 'uniform' else 'f32_blocked_l0_and_snr'
    xs, D, _ = ru.row_inputs(name)
    shared, per_signal = ru.ROWS[name][3], ru.ROWS[name][4]
    if form == 'uniform':
        seqs, extra = np.stack(xs), {}
    elif form == 'list':
        seqs, extra = xs, {}
    else:
        x, lens = _padded(xs, fill=np.nan)
        seqs, extra = x[:, :, 0], dict(lengths=lens)
    cmp = ConvolutionalMatchingPursuit()
    res = ConvolutionalSparseCoder(D, cmp).encodeBatch(seqs, nbNonzeroCoefs=np.array(per_signal['nbNonzeroCoefs']),
                                                       toleranceSnr=tuple(per_signal['toleranceSnr']), **dict(shared, **extra))
    small = cmp.computeCoefficientsBatch(seqs, D, nbNonzeroCoefs=per_signal['nbNonzeroCoefs'], toleranceSnr=per_signal['toleranceSnr'],
                                         maxEvents=16, **dict(shared, **extra))
    assert res.variant.endswith('_ragged_rules') and small.variant == res.variant
    if form == 'uniform':
        assert res.lengths is None and isinstance(res.residuals, np.ndarray) and res.residuals.shape == (len(xs), len(xs[0]))
    else:
        assert list(res.lengths) == [len(s) for s in xs] and isinstance(res.residuals, list)
    single = ConvolutionalMatchingPursuit()
    for b, s in enumerate(xs):
        coef, residual, one = _reference_signal(single, s, D, **ru.signal_kw(name, b))
        for r in (res, small):
            assert r.coefficients[b].shape == (len(s), D.shape[0]) and (r.coefficients[b] != coef).nnz == 0
            assert r.residuals[b].shape == residual.shape and np.array_equal(r.residuals[b], residual)
            assert all(np.array_equal(u, v) for u, v in zip(r.events[b], one.events[0]))
            assert np.array_equal(r.stats[b], one.stats[0]) and np.array_equal(r.energies[b], one.energies[0])


def _modeling_stop_condition_runs_round_by_round():
    """A stopCondition: one round per launch, every signal under its own nbNonzeroCoefs across the hscmp_continue calls, and the
    callback's own stops beside them."""
    from hsc_amd.modeling import ConvolutionalMatchingPursuit
    name = 'f32_default_l0'
    xs, D, _ = ru.row_inputs(name)
    l0 = ru.ROWS[name][4]['nbNonzeroCoefs']

    def stop(seq, residual, coefficients):
        return seq.shape[0] % 2 == 1 and coefficients.nnz >= 20          # (the odd lengths, once they hold 20 coefficients)

    res = ConvolutionalMatchingPursuit().computeCoefficientsBatch(xs, D, nbNonzeroCoefs=l0, stopCondition=stop)
    assert res.variant.endswith('_ragged_rules')
    single = ConvolutionalMatchingPursuit()
    for b, s in enumerate(xs):
        coef, residual, one = _reference_signal(single, s, D, nbNonzeroCoefs=l0[b], stopCondition=stop)
        assert (res.coefficients[b] != coef).nnz == 0 and np.array_equal(res.residuals[b], residual)
        assert all(np.array_equal(u, v) for u, v in zip(res.events[b], one.events[0]))
        assert np.array_equal(res.stats[b], one.stats[0])
    stops = res.stop_reasons()
    assert 'callback' in stops and 'nnz' in stops
