"""What the stop-rules-per-signal test files share (tests/test_rules_census.py on the CPU, tests/test_gpu_rules.py on the GPU): the
rows of the matrix -- the inputs of tests/test_gpu_ragged.py with a value per signal for one or two of the three stop rules -- and
the scalars a signal gets when it is encoded alone."""
import numpy as np

from tests.test_gpu_ragged import F32, F64, GEN_LENGTHS, MF_LENGTHS

UNIFORM_LENGTHS = [2048] * 6

# a value per signal (six signals in every row): L0 with the smallest (1) and the largest next to each other inside the first
# workgroup of the four-signal loop, SNR targets from 5 to 30 dB, residual scales around the planted coefficients' size
L0 = [5, 60, 17, 33, 60, 1]
L0_GEN = [3, 7, 5, 30, 12, 1]                 # (the generic lengths start at W: few atoms fit)
SNR = [30.0, 5.0, 12.0, 20.0, 25.0, 8.0]
SNR_GEN = [30.0, 25.0, 28.0, 5.0, 12.0, 20.0]
SCALE = [0.05, 0.8, 0.4, 0.1, 0.2, 0.6]

# name: (dtype, lengths, env, the arguments every signal shares, the arguments given per signal, variant without the suffixes
#        (None: what the uniform entry picks for the padded batch), weights)
ROWS = {
    # 1-3: the matrix-core loops of single arg-max encodes
    'f32_default_l0': (F32, MF_LENGTHS, {}, {}, dict(nbNonzeroCoefs=L0), 'mfma_init+mfma_loop_f32_bound', False),
    'f32_exact_init_l0': (F32, MF_LENGTHS, {'HSCMP_EXACT_INIT': '1'}, {}, dict(nbNonzeroCoefs=L0), 'mfma_init+mfma_loop_f32', False),
    'f32_quad_forced_l0': (F32, MF_LENGTHS, {'HSCMP_MFMA_QUAD': '1', 'HSCMP_EXACT_INIT': '1'}, {}, dict(nbNonzeroCoefs=L0),
                           'mfma_init+mfma_loop_f32_x4', False),
    # 4-5: blocked rounds, round-parallel and not: the weak-atom filter reads the signal's own toleranceSnr
    'f32_blocked_rp_snr': (F32, MF_LENGTHS, {'HSCMP_RP': '1'}, dict(nbBlocks=6), dict(toleranceSnr=SNR), 'mfma_init+mfma_loop_f32_rp', False),
    'f32_blocked_rp_auto_snr': (F32, MF_LENGTHS, {'HSCMP_RP': '1'}, dict(nbBlocks='auto'), dict(toleranceSnr=SNR),
                                'mfma_init+mfma_loop_f32_rp', False),
    'f32_blocked_no_rp_snr': (F32, MF_LENGTHS, {'HSCMP_RP': '0'}, dict(nbBlocks=6), dict(toleranceSnr=SNR), 'mfma_init+mfma_loop_f32', False),
    'f32_blocked_no_rp_auto_snr': (F32, MF_LENGTHS, {'HSCMP_RP': '0'}, dict(nbBlocks='auto'), dict(toleranceSnr=SNR),
                                   'mfma_init+mfma_loop_f32', False),
    # 6: the generic pair, lengths from W and 3W-3 on
    'f32_force_generic_l0': (F32, GEN_LENGTHS, {'HSCMP_FORCE_GENERIC': '1'}, {}, dict(nbNonzeroCoefs=L0_GEN), 'generic_init+generic_loop_f32', False),
    'f32_force_generic_blocked_snr': (F32, GEN_LENGTHS, {'HSCMP_FORCE_GENERIC': '1'}, dict(nbBlocks=3), dict(toleranceSnr=SNR_GEN),
                                      'generic_init+generic_loop_f32', False),
    # 7: float64
    'f64_default_l0': (F64, MF_LENGTHS, {}, {}, dict(nbNonzeroCoefs=L0), 'mfma_init+mfma_loop_f64', False),
    'f64_blocked_snr': (F64, MF_LENGTHS, {}, dict(nbBlocks=6), dict(toleranceSnr=SNR), None, False),
    'f64_generic_l0': (F64, GEN_LENGTHS, {}, {}, dict(nbNonzeroCoefs=L0_GEN), 'generic_init+generic_loop_f64', False),
    'f64_generic_blocked_snr': (F64, GEN_LENGTHS, {}, dict(nbBlocks=3), dict(toleranceSnr=SNR_GEN), 'generic_init+generic_loop_f64', False),
    # 8: weights
    'f32_weights_l0': (F32, MF_LENGTHS, {'HSCMP_EXACT_INIT': '1'}, {}, dict(nbNonzeroCoefs=L0), None, True),
    'f32_weights_blocked_snr': (F32, MF_LENGTHS, {}, dict(nbBlocks=6), dict(toleranceSnr=SNR), None, True),
    'f64_weights_l0': (F64, MF_LENGTHS, {}, {}, dict(nbNonzeroCoefs=L0), None, True),
    # 9: the residual scale (the plan is the one a scalar toleranceResidualScale picks: expected None)
    'f32_scale': (F32, MF_LENGTHS, {}, {}, dict(toleranceResidualScale=SCALE), None, False),
    'f32_blocked_scale': (F32, MF_LENGTHS, {}, dict(nbBlocks=6), dict(toleranceResidualScale=SCALE), None, False),
    # 10: two rules per signal at once
    'f32_l0_and_snr': (F32, MF_LENGTHS, {}, {}, dict(nbNonzeroCoefs=L0, toleranceSnr=SNR), None, False),
    'f32_blocked_l0_and_snr': (F32, MF_LENGTHS, {'HSCMP_RP': '1'}, dict(nbBlocks=6), dict(nbNonzeroCoefs=L0, toleranceSnr=SNR),
                               'mfma_init+mfma_loop_f32_rp', False),
    # 11: the same arrays on uniform lengths (the ragged rows above are the other form)
    'f32_uniform_l0': (F32, UNIFORM_LENGTHS, {}, {}, dict(nbNonzeroCoefs=L0), 'mfma_init+mfma_loop_f32_bound', False),
    'f32_uniform_blocked_snr': (F32, UNIFORM_LENGTHS, {'HSCMP_RP': '1'}, dict(nbBlocks=6), dict(toleranceSnr=SNR), 'mfma_init+mfma_loop_f32_rp', False),
    'f32_uniform_blocked_l0_and_snr': (F32, UNIFORM_LENGTHS, {'HSCMP_RP': '0'}, dict(nbBlocks='auto'), dict(nbNonzeroCoefs=L0, toleranceSnr=SNR),
                                       'mfma_init+mfma_loop_f32', False),
}


def _signals(dtype, lengths, K=32, W=32, seed=5, weights=False):
    """tests/test_gpu_ragged.py's signals with at least four planted atoms and five times its noise: the shortest signals (W,
    3W-3, 3W-2 samples) then need several atoms for every rule here, so none of them stops at its first atom whatever its rule says."""
    import hsc_amd.synth as synth
    D = synth.make_dictionary(K, W, seed=seed, dtype=dtype)
    xs = [synth.make_signal(D, int(n), i, kind='planted', nb_atoms=max(4, min(40, n // 48)), noise=0.05, seed=seed, dtype=dtype)
          for i, n in enumerate(lengths)]
    w = None
    if weights:
        w = np.ones(K, dtype=dtype)
        w[::3] = dtype(0.5)              # (the singleton weights of a level dictionary: some atoms count less)
    return xs, D, w


_INPUTS = {}


def row_inputs(name):
    """(signals, D, weights or None) of a row; built once per (dtype, lengths, weights) and shared: treat them as read-only."""
    dtype, lengths, _, _, _, _, weighted = ROWS[name]
    key = (dtype, tuple(lengths), weighted)
    if key not in _INPUTS:
        _INPUTS[key] = _signals(dtype, lengths, weights=weighted)
    return _INPUTS[key]


def signal_kw(name, b):
    """The keyword arguments signal b of a row gets when it is encoded alone: the shared ones and its own scalars."""
    _, _, _, shared, per_signal, _, _ = ROWS[name]
    kw = dict(shared)
    kw.update((key, vals[b]) for key, vals in per_signal.items())
    return kw


def is_blocked(name):
    return ROWS[name][3].get('nbBlocks', 1) != 1
