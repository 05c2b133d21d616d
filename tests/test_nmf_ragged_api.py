"""ConvolutionalNMF.computeCoefficientsRaggedBatch (hscnmf_compute_ragged) on the CPU: the headers and
EXPORTS / PLAN_EXPORTS, the chunk arithmetic through nmf.ragged_plan (hscnmf_ragged_plan needs no device), and what the Python layer
prepares for the library call (the call itself replaced by a fake).  The GPU tests are in tests/test_gpu_nmf_ragged.py."""
import os
import re

import numpy as np
import pytest

from hsc_amd import _native, nmf
from hsc_amd.nmf import ConvolutionalNMF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 40


# ------------------------------------------------------------------------------------------------ header and exports
def test_header_declares_what_exports_loads():
    """include/hscnmf.h declares the entry points that take a context (EXPORTS) and includes include/hscnmf_plan.h, which
    declares the context-free hscnmf_ragged_plan (PLAN_EXPORTS); the library exports both."""
    text = open(os.path.join(ROOT, 'include', 'hscnmf.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    plan = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'hscnmf_plan.h')).read(), flags=re.S)
    assert re.search(r'\bint hscnmf_compute_ragged\(hscnmf_ctx\* ctx, int dtype, const void\* x, const int64_t\* lengths, int B, int F,', code)
    assert re.search(r'\bint hscnmf_ragged_plan\(int dtype, const int64_t\* lengths, int B, int F, int K, int W, uint64_t budget_bytes,', plan)
    assert '#include "hscnmf_plan.h"' in code
    assert sorted(set(re.findall(r'\b(hscnmf_[a-z0-9_]+)\s*\(', code))) == sorted(nmf.EXPORTS)
    assert sorted(set(re.findall(r'\b(hscnmf_[a-z0-9_]+)\s*\(', plan))) == sorted(nmf.PLAN_EXPORTS)
    assert 'hscnmf_compute_ragged' in nmf.EXPORTS and nmf.PLAN_EXPORTS == ['hscnmf_ragged_plan']
    lib = nmf.load_library()
    for name in nmf.EXPORTS + nmf.PLAN_EXPORTS:
        assert hasattr(lib, name), name
    assert len(lib.hscnmf_compute_ragged.argtypes) == 19 and len(lib.hscnmf_ragged_plan.argtypes) == 10
    note = re.search(r'int hscnmf_version\(void\);\s*/\*(.*?)\*/', text, flags=re.S).group(1)
    assert lib.hscnmf_version() == 2 and 'hscnmf_compute_ragged' in note and 'hscnmf_ragged_plan' in note


# ------------------------------------------------------------------------------------------------ the plan
def test_plan_one_chunk_under_a_large_budget():
    first, most = nmf.ragged_plan(np.float32, [300, 17, 4000, 129], 3, 8, 6, BIG)
    assert first.tolist() == [0, 4] and first.dtype == np.int32 and 0 < most < BIG


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_plan_budget_for_two_of_three_equal_signals(dtype):
    lengths, F, K, W = [5000, 5000, 5000], 2, 8, 6
    _, one = nmf.ragged_plan(dtype, lengths[:1], F, K, W, BIG)
    first2, two = nmf.ragged_plan(dtype, lengths[:2], F, K, W, BIG)
    _, three = nmf.ragged_plan(dtype, lengths, F, K, W, BIG)
    assert first2.tolist() == [0, 2] and one < two < three
    first, most = nmf.ragged_plan(dtype, lengths, F, K, W, two)
    assert first.tolist() == [0, 2, 3] and most == two
    first, most = nmf.ragged_plan(dtype, lengths, F, K, W, two - 1)           # one byte less: one signal per chunk
    assert first.tolist() == [0, 1, 2, 3] and most == one
    # the bytes are the A pair, x, the residual, the partials and the small tables: at least the four large arrays
    item = np.dtype(dtype).itemsize
    assert one >= 2 * (5000 - W + 1) * K * item + 2 * 5000 * F * item


def test_plan_a_signal_beyond_the_budget_gets_its_own_chunk():
    lengths = [300, 300, 50000, 300, 300]
    _, small = nmf.ragged_plan(np.float32, [300, 300], 1, 8, 6, BIG)
    _, big = nmf.ragged_plan(np.float32, [50000], 1, 8, 6, BIG)
    assert small < big
    first, most = nmf.ragged_plan(np.float32, lengths, 1, 8, 6, small)
    assert first.tolist() == [0, 2, 3, 5] and most == big
    first, most = nmf.ragged_plan(np.float32, lengths, 1, 8, 6, 1)            # every signal is beyond a budget of one byte
    assert first.tolist() == [0, 1, 2, 3, 4, 5] and most == big


def test_plan_bytes_are_monotone_in_k_and_f():
    lengths = [300, 17, 4000, 129]
    by_k = [nmf.ragged_plan(np.float32, lengths, 2, K, 6, BIG)[1] for K in (1, 2, 7, 8, 9, 33, 64)]
    by_f = [nmf.ragged_plan(np.float32, lengths, F, 8, 6, BIG)[1] for F in (1, 2, 3, 7, 16)]
    assert by_k == sorted(by_k) and len(set(by_k)) == len(by_k)
    assert by_f == sorted(by_f) and len(set(by_f)) == len(by_f)
    assert nmf.ragged_plan(np.float64, lengths, 2, 8, 6, BIG)[1] > nmf.ragged_plan(np.float32, lengths, 2, 8, 6, BIG)[1]


def test_plan_is_a_partition_into_runs_within_the_budget():
    rs = np.random.RandomState(4)
    lengths = rs.randint(6, 3000, size=40).tolist()
    _, whole = nmf.ragged_plan(np.float64, lengths, 2, 5, 6, BIG)
    for budget in (whole // 3, whole // 7, whole // 20):
        first, most = nmf.ragged_plan(np.float64, lengths, 2, 5, 6, budget)
        assert first[0] == 0 and first[-1] == len(lengths) and np.all(np.diff(first) >= 1)
        sizes = [nmf.ragged_plan(np.float64, lengths[a:b], 2, 5, 6, BIG)[1] for a, b in zip(first[:-1], first[1:])]
        assert most == max(sizes)
        for (a, b), s in zip(zip(first[:-1], first[1:]), sizes):
            assert s <= budget or b - a == 1
            if b < len(lengths):                          # greedy: the next signal would not have fitted
                assert nmf.ragged_plan(np.float64, lengths[a:b + 1], 2, 5, 6, BIG)[1] > budget


PLAN_BAD = [
    ('dtype', dict(dtype=7), 'unknown dtype'),
    ('no_signal', dict(lengths=[]), 'B = 0'),
    ('k', dict(K=0), 'K = 0'),
    ('f', dict(F=0), 'F = 0'),
    ('w', dict(W=1), 'filter width 1'),
    ('short', dict(lengths=[300, 5, 300]), 'signal 1'),
    ('budget', dict(budget=0), 'budget_bytes'),
]


@pytest.mark.parametrize('name,kw,needle', PLAN_BAD, ids=[b[0] for b in PLAN_BAD])
def test_plan_refuses_bad_arguments(monkeypatch, name, kw, needle):
    args = dict(dtype=np.float32, lengths=[300, 300], F=1, K=8, W=6, budget=BIG)
    args.update(kw)
    if name == 'dtype':
        monkeypatch.setattr(_native, 'dtype_code', lambda dt: 7)
    with pytest.raises(_native.HscmpError) as ei:
        nmf.ragged_plan(**args)
    assert ei.value.code == _native.ERR_INVALID, str(ei.value)
    assert 'hscnmf_ragged_plan' in str(ei.value) and needle in str(ei.value), str(ei.value)


def test_plan_refuses_null_pointers_and_unsupported_shapes():
    lib = nmf.load_library()
    lens = np.array([300], dtype=np.int64)
    n, most = np.zeros(1, np.int32), np.zeros(1, np.uint64)
    p = _native._ptr
    assert lib.hscnmf_ragged_plan(0, None, 1, 1, 8, 6, 100, None, p(n), p(most)) == _native.ERR_INVALID
    assert lib.hscnmf_ragged_plan(0, p(lens), 1, 1, 8, 6, 100, None, None, p(most)) == _native.ERR_INVALID
    assert lib.hscnmf_ragged_plan(0, p(lens), 1, 1, 8, 6, 100, None, p(n), None) == _native.ERR_INVALID
    assert lib.hscnmf_ragged_plan(0, p(lens), 1, 1, 8, 6, 100, None, p(n), p(most)) == 0 and n[0] == 1     # chunk_first may be NULL
    # a shape whose workgroup does not fit the LDS, and a signal beyond the per-signal limit L * K <= 2^28
    with pytest.raises(_native.HscmpError) as ei:
        nmf.ragged_plan(np.float64, [70000], 64, 8, 40000, BIG)
    assert ei.value.code == _native.ERR_UNSUPPORTED and 'LDS' in str(ei.value)
    with pytest.raises(_native.HscmpError) as ei:
        nmf.ragged_plan(np.float32, [300, (1 << 28) // 8 + 6], 1, 8, 6, BIG)
    assert ei.value.code == _native.ERR_UNSUPPORTED and 'signal 1' in str(ei.value)
    assert nmf.ragged_plan(np.float32, [300, (1 << 28) // 8 + 5], 1, 8, 6, BIG)[0].tolist() == [0, 2]


# ------------------------------------------------------------------------------------------------ the Python layer
def _capture(monkeypatch):
    captured = {}

    def fake(device, dt, x, lengths, D3, a0, energy, params):
        captured.update(dt=dt, x=x, lengths=lengths, D3=D3, a0=a0, energy=energy, max_iterations=params.max_iterations,
                        has_snr=params.has_snr, tolerance_snr=params.tolerance_snr, memory_budget=params.memory_budget,
                        calls=captured.get('calls', 0) + 1)
        B = len(lengths)
        st = nmf.NMFStats(np.ones(B, np.int32), np.ones(B, np.int32), np.zeros(B), np.zeros(B), np.zeros(5))
        coef = np.arange(x.shape[0] * D3.shape[0], dtype=dt).reshape((x.shape[0], D3.shape[0]))
        return coef, -x, st
    monkeypatch.setattr(nmf, '_call_compute_ragged', fake)
    return captured


def _split(stack, lengths):
    ends = np.cumsum(lengths)
    return [stack[e - n:e] for e, n in zip(ends, lengths)]


def _ragged(dtype, F, lengths=(40, 9, 23)):
    rs = np.random.RandomState(1)
    return [rs.random_sample((T,) if F == 1 else (T, F)).astype(dtype) for T in lengths]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('F', [1, 3])
def test_stacking_draw_order_and_results(monkeypatch, dtype, F):
    """The call hands over the stack, the rows 0 .. L_b-1 of each signal's coefficients (drawn per signal in corpus
    order, as a loop of computeCoefficients draws them) and the energies, and cuts the results back per signal."""
    captured = _capture(monkeypatch)
    K, W = 5, 4
    sigs = _ragged(dtype, F)
    lengths = [q.shape[0] for q in sigs]
    D = np.random.RandomState(2).random_sample((K, W) if F == 1 else (K, W, F)).astype(dtype)
    cnmf = ConvolutionalNMF(memoryBudget=12345)
    np.random.seed(17)
    coef, resid, st = cnmf.computeCoefficientsRaggedBatch(sigs, D, nbMaxIterations=3, toleranceSnr=2.5)
    np.random.seed(17)
    a0 = [nmf.draw_initial_coefficients(T, K, dtype) for T in lengths]           # what per-signal calls draw, in order
    stack = np.concatenate(sigs).reshape((-1, F))
    assert captured['dt'] == dtype and captured['calls'] == 1
    assert (captured['max_iterations'], captured['has_snr'], captured['tolerance_snr'], captured['memory_budget']) == (3, 1, 2.5, 12345)
    assert captured['lengths'].dtype == np.int64 and captured['lengths'].tolist() == lengths
    assert captured['x'].dtype == dtype and captured['x'].shape == (sum(lengths), F) and np.array_equal(captured['x'], stack)
    assert captured['x'].flags['C_CONTIGUOUS'] and captured['a0'].flags['C_CONTIGUOUS'] and captured['D3'].flags['C_CONTIGUOUS']
    assert captured['D3'].shape == (K, W, F) and np.array_equal(captured['D3'], D.reshape((K, W, F)))
    assert captured['a0'].dtype == dtype and captured['a0'].shape == (sum(T - W + 1 for T in lengths), K)
    assert np.array_equal(captured['a0'], np.concatenate([a[:T - W + 1] for a, T in zip(a0, lengths)]))
    assert captured['energy'].dtype == np.float64
    assert np.array_equal(captured['energy'], [np.sum(np.square(q)) for q in _split(captured['x'], lengths)])
    # results: lists per signal, the residual squeezed for 1-D signals
    assert isinstance(coef, list) and isinstance(resid, list) and len(coef) == len(resid) == len(sigs)
    whole = np.arange(sum(lengths) * K, dtype=dtype).reshape((-1, K))
    for c, r, q, cw in zip(coef, resid, sigs, _split(whole, lengths)):
        assert c.shape == (q.shape[0], K) and c.dtype == dtype and np.array_equal(c, cw)
        assert r.shape == q.shape and r.dtype == dtype and np.array_equal(r, -q)
    assert st is cnmf.lastStats and st.iterations.shape == (len(sigs),)
    # explicit initial coefficients: no draw at all, the same rows handed over
    first = captured['a0'].copy()
    state = np.random.get_state()[1].copy()
    cnmf.computeCoefficientsRaggedBatch(sigs, D, initialCoefficients=a0)
    assert np.array_equal(np.random.get_state()[1], state) and np.array_equal(captured['a0'], first)
    assert captured['max_iterations'] == 1 and captured['has_snr'] == 0


def test_draws_equal_per_signal_calls(monkeypatch):
    """Under one seed the ragged call hands over, signal by signal, what computeCoefficients hands to hscnmf_compute."""
    captured = _capture(monkeypatch)
    K, W = 5, 4
    sigs = _ragged(np.float32, 2)
    D = np.random.RandomState(2).random_sample((K, W, 2)).astype(np.float32)
    np.random.seed(5)
    ConvolutionalNMF().computeCoefficientsRaggedBatch(sigs, D, nbMaxIterations=2)
    seen = []

    class FakeContext(object):
        def call(self, name, dtype, x, B, T, F, D3, K_, W_, a0, *rest):
            import ctypes
            n = B * T * K_
            seen.append(np.ctypeslib.as_array(ctypes.cast(a0, ctypes.POINTER(ctypes.c_float)), (n,)).reshape((T, K_)).copy())
    monkeypatch.setattr(nmf, '_context', lambda device: FakeContext())
    np.random.seed(5)
    for q in sigs:
        ConvolutionalNMF().computeCoefficients(q, D, nbMaxIterations=2)
    assert np.array_equal(captured['a0'], np.concatenate([a[:a.shape[0] - W + 1] for a in seen]))


@pytest.mark.parametrize('F', [1, 2])
def test_input_forms_prepare_the_same_arrays(monkeypatch, F):
    """A list, a tuple, and the padded array with `lengths` (NaN padding, never copied) give identical arrays; a [B,T(,F)]
    array is the list of its rows."""
    captured = _capture(monkeypatch)
    K, W = 3, 4
    sigs = _ragged(np.float64, F)
    lengths = [q.shape[0] for q in sigs]
    D = np.random.RandomState(2).random_sample((K, W) if F == 1 else (K, W, F))
    padded = np.full((len(sigs), max(lengths) + 5) + sigs[0].shape[1:], np.nan)
    for b, q in enumerate(sigs):
        padded[b, :q.shape[0]] = q
    got = []
    for kw in (dict(sequences=sigs), dict(sequences=tuple(sigs)), dict(sequences=padded, lengths=lengths),
               dict(sequences=padded, lengths=np.array(lengths, dtype=np.int32))):
        np.random.seed(3)
        coef, resid, _ = ConvolutionalNMF().computeCoefficientsRaggedBatch(D=D, nbMaxIterations=2, **kw)
        got.append({k: captured[k].copy() for k in ('x', 'lengths', 'D3', 'a0', 'energy')})
        assert np.all(np.isfinite(captured['x'])) and np.all(np.isfinite(captured['energy']))
        assert [r.shape for r in resid] == [q.shape for q in sigs] and all(np.all(np.isfinite(r)) for r in resid)
    for g in got[1:]:
        for k in g:
            assert np.array_equal(g[k], got[0][k]), k
    same = np.stack([q[:lengths[1]] for q in sigs])            # [B,T(,F)]: every row a signal
    np.random.seed(3)
    ConvolutionalNMF().computeCoefficientsRaggedBatch(same, D, nbMaxIterations=2)
    a = {k: captured[k].copy() for k in ('x', 'lengths', 'a0', 'energy')}
    np.random.seed(3)
    ConvolutionalNMF().computeCoefficientsRaggedBatch(list(same), D, nbMaxIterations=2)
    for k in a:
        assert np.array_equal(a[k], captured[k]), k


def test_float32_signals_with_a_float64_dictionary_run_in_float64_and_come_back_in_float32(monkeypatch):
    """The dtype rules of computeCoefficientsBatch: the draw in the data's dtype, the run in the common dtype, the results
    cast back to the data's."""
    captured = _capture(monkeypatch)
    sigs = _ragged(np.float32, 1)
    D = np.random.RandomState(2).random_sample((5, 4))
    np.random.seed(9)
    coef, resid, _ = ConvolutionalNMF().computeCoefficientsRaggedBatch(sigs, D)
    np.random.seed(9)
    a0 = [nmf.draw_initial_coefficients(q.shape[0], 5, np.float32) for q in sigs]
    assert captured['dt'] == np.float64 and captured['a0'].dtype == np.float64
    assert np.array_equal(captured['a0'], np.concatenate([a[:a.shape[0] - 3] for a in a0]).astype(np.float64))
    assert all(c.dtype == np.float32 for c in coef) and all(r.dtype == np.float32 and r.ndim == 1 for r in resid)


def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(nmf, '_context', no_device)
    monkeypatch.setattr(nmf, 'load_library', no_device)
    monkeypatch.setattr(nmf, '_call_compute_ragged', no_device)


def _sig(*lengths, **kw):
    return [np.random.RandomState(T).random_sample((T,) + kw.get('tail', ())).astype(kw.get('dtype', np.float64)) for T in lengths]


BAD = [
    ('w_below_2', 1, dict(sequences=_sig(30, 40)), 'signal 0'),
    ('shorter_than_w', 8, dict(sequences=_sig(30, 7, 40)), 'signal 1'),
    ('mixed_dtypes', 4, dict(sequences=_sig(30) + _sig(31, dtype=np.float32)), 'one dtype'),
    ('mixed_f', 4, dict(sequences=_sig(30, tail=(2,)) + _sig(31, tail=(3,))), 'same F'),
    ('empty_list', 4, dict(sequences=[]), 'at least one signal'),
    ('lengths_with_list', 4, dict(sequences=_sig(30, 40), lengths=[30, 40]), 'lengths='),
    ('lengths_too_long', 4, dict(sequences=np.zeros((2, 30)), lengths=[30, 31]), 'padded length'),
    ('lengths_count', 4, dict(sequences=np.zeros((2, 30)), lengths=[30]), 'entries'),
    ('one_dimension', 4, dict(sequences=np.zeros((30,))), 'dimensions'),
    ('dictionary_features', 4, dict(sequences=_sig(30, tail=(2,))), 'dictionary'),
    ('coefficients_count', 4, dict(sequences=_sig(30, 40), initialCoefficients=[np.ones((30, 4))]), 'initial coefficient arrays'),
    ('coefficients_shape', 4, dict(sequences=_sig(30, 40), initialCoefficients=[np.ones((30, 4)), np.ones((39, 4))]),
     'initial coefficients of signal 1'),
]


@pytest.mark.parametrize('name,W,kw,needle', BAD, ids=[b[0] for b in BAD])
def test_argument_errors_raise_before_any_device_call(monkeypatch, name, W, kw, needle):
    _no_device(monkeypatch)
    with pytest.raises(Exception) as ei:
        ConvolutionalNMF().computeCoefficientsRaggedBatch(D=np.ones((4, W)), nbMaxIterations=2, **kw)
    assert not isinstance(ei.value, AssertionError), ei.value
    assert needle in str(ei.value), str(ei.value)
    assert 'k-means' not in str(ei.value)


def test_the_uniform_calls_do_not_go_through_the_ragged_path(monkeypatch):
    """computeCoefficientsBatch and computeCoefficients are unchanged: they still call hscnmf_compute."""
    monkeypatch.setattr(nmf, '_call_compute_ragged', lambda *a, **k: pytest.fail('the ragged call was used'))
    names = []

    class FakeContext(object):
        def call(self, name, *args):
            names.append(name)
    monkeypatch.setattr(nmf, '_context', lambda device: FakeContext())
    ConvolutionalNMF().computeCoefficients(np.random.random(30), np.random.random((4, 5)), nbMaxIterations=2)
    ConvolutionalNMF().computeCoefficientsBatch(np.random.random((2, 30)), np.random.random((4, 5)), nbMaxIterations=2)
    assert names == ['compute', 'compute']
