"""The wide loop on the host side (no GPU): its shape rule through hscmp_wide_plan -- the arithmetic plan_encode goes by --
the argument checks, and the C ABI of the two new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def _plan(K, W, B, T, nbBlocks='auto', F=1, dtype=F32, weights=False, **kw):
    from hsc_amd import _native
    kw.setdefault('toleranceSnr', 20.0)
    params = _native.make_params(nbBlocks=nbBlocks, eps=1e-7, **kw)
    return _native.wide_plan(K, W, F, dtype, weights, B, T, params)


def test_the_reference_workflow_goes_wide_by_default():
    """One long signal, nbBlocks='auto' (blocks of 4W): more candidates per round than the round-parallel workgroup holds."""
    for K, W, T in ((32, 16, 65536), (64, 64, 262144), (128, 32, 1048576), (256, 64, 1048576)):
        p = _plan(K, W, 1, T)
        assert p['candidates'] == T // (4 * W) + 1
        assert p['can_run'] and p['by_default'], (K, W, T, p)
        assert 0 < p['control_lds'] <= 158 * 1024


def test_below_the_round_parallel_cap_only_when_forced():
    p = _plan(32, 16, 3, 16384)                      # 257 candidates: the round-parallel loop runs it
    assert p == dict(can_run=True, by_default=False, candidates=257, control_lds=p['control_lds'])
    p = _plan(128, 32, 1, 1048576, nbBlocks=10)      # 11 long blocks
    assert p['can_run'] and not p['by_default'] and p['candidates'] == 11


def test_large_batches_keep_todays_loops():
    assert _plan(32, 16, 16, 65536)['by_default']
    p = _plan(32, 16, 17, 65536)
    assert p['can_run'] and not p['by_default']


def test_one_round_per_call_keeps_todays_loop_unless_forced():
    p = _plan(32, 16, 1, 65536, maxRounds=1)         # a stopCondition callback: one round per call
    assert p['can_run'] and not p['by_default']


@pytest.mark.parametrize('what, kw', [
    ('three chunks of taps', dict(W=20)),
    ('five chunks', dict(W=40)),
    ('one chunk', dict(W=8)),
    ('several features', dict(F=3)),
    ('float64', dict(dtype=F64)),
    ('single arg-max', dict(nbBlocks=1)),
    ('toleranceResidualScale', dict(toleranceResidualScale=0.5)),
    ('signal shorter than 3W-2', dict(T=40)),
    ('more candidates than the sort holds', dict(T=16384 * 64 + 64)),
])
def test_shapes_without_a_wide_form(what, kw):
    args = dict(K=32, W=16, B=1, T=65536)
    args.update(kw)
    p = _plan(**args)
    assert not p['can_run'] and not p['by_default'], (what, p)


def test_the_cap_on_candidates_and_the_lds_budget():
    """16 384 candidates are sorted in LDS (8 bytes each, padded to a power of two); the dictionary image of the control
    workgroup's own atoms shares the budget, so a large dictionary lowers the cap."""
    assert _plan(32, 16, 1, 16383 * 64)['can_run']                       # 16 384 candidates, 128 KiB of keys, a 2 KiB image
    assert not _plan(32, 16, 1, 16384 * 64)['can_run']                   # 16 385
    big = _plan(256, 64, 1, 8192 * 256 + 256)                            # 8 193 candidates -> 16 384 keys beside a 64 KiB image
    assert not big['can_run'] and big['control_lds'] > 158 * 1024
    assert _plan(256, 64, 1, 8191 * 256)['can_run']                      # 8 192 keys


def test_weights_take_their_lds():
    a, b = _plan(64, 32, 1, 65536), _plan(64, 32, 1, 65536, weights=True)
    assert b['control_lds'] == a['control_lds'] + 4 * 64


def test_bad_arguments_are_refused():
    from hsc_amd import _native
    params = _native.make_params(nbBlocks='auto', toleranceSnr=20.0, eps=1e-7)
    for bad in (dict(K=0), dict(W=0), dict(B=0), dict(T=0), dict(F=0)):
        args = dict(K=32, W=16, F=1, B=1, T=4096)
        args.update(bad)
        with pytest.raises(_native.HscmpError) as ex:
            _native.wide_plan(args['K'], args['W'], args['F'], F32, False, args['B'], args['T'], params)
        assert ex.value.code == _native.ERR_INVALID
    lib = _native.load_library()
    out = np.zeros(4, dtype=np.int32)
    assert lib.hscmp_wide_plan(32, 16, 1, 0, 0, 1, 4096, None, out.ctypes.data_as(ctypes.c_void_p)) == _native.ERR_INVALID
    assert lib.hscmp_wide_plan(32, 16, 1, 0, 0, 1, 4096, ctypes.byref(params), None) == _native.ERR_INVALID
    assert lib.hscmp_wide_counters(None, out.ctypes.data_as(ctypes.c_void_p)) == _native.ERR_INVALID


def test_the_header_declares_what_the_binding_loads():
    from hsc_amd import _native
    text = open(os.path.join(ROOT, 'include', 'hscmp.h')).read()
    for name in ('hscmp_wide_plan', 'hscmp_wide_counters'):
        assert re.search(r'\bint %s\(' % name, text) and name in _native.EXPORTS
    assert '"_wide"' in text                        # hscmp_encode_batch_device says when it is synchronous


def test_the_knob_is_read_in_one_place():
    """read_knobs of hscmp_api.hip, and nowhere else in the package"""
    pkg = os.path.join(ROOT, 'hierarchical-sparse-coding_amd')
    readers = []
    for base, _, names in os.walk(pkg):
        for name in names:
            if name.endswith(('.hip', '.h', '.py')):
                text = open(os.path.join(base, name)).read()
                readers += [name] * (text.count('getenv("HSCMP_WIDE")') + text.count("environ.get('HSCMP_WIDE'") + text.count("environ['HSCMP_WIDE'"))
    assert readers == ['hscmp_api.hip']
