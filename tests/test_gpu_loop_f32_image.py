"""The bound loop on a float32 image (MfmaRecorr with BOUND): whole
encodes, bit for bit, against HSCMP_EXACT_INIT=1 (both passes exact) and HSCMP_EXACT_RECORR=1 (exact loop behind the
bound pass) -- events, slots, stats, energies, residual.  HSCMP_MFMA_QUAD=1 forces the four-signal loop, the only one with
the bound form.  No case carries a tolerance, and the tests assert identity only.

The workgroup keeps [bf16 image][float32 image][weights] in LDS: the bound tile reads the first, the exact chains (refine,
resolve_group, the residual update) and the fallback tile the second.

(a) the image's offsets: every chunk count the bound loop is built for (W = 57: 8 chunks, W = 32: 4, W = 13: 2), K not a
    multiple of 32 (padded atoms; K = 33: one atom in the second group), odd W (padded taps), with and without weights,
    planted and noise; and a dictionary whose entries carry full 24-bit significands with magnitudes from 2^-30 to 2^30,
    the values three bf16 terms were once needed for;
(b) the fallback tile (a window with a sample outside the model of the bound tile) at each width, with weights: the sample
    inside the support of the first atom (the update touches it), and beside the support in a row the atom re-correlates;
(c) the refine's loads -- hint, window, the stored scores of the winner's segment (whatever order they are issued in;
    DESIGN.md section 11 has the measurement of issuing them together): winners in the first and the last segment and on
    either side of a segment boundary, for one, two, four and eight stored scores per lane; both signal ends (even W:
    the stale row T - 1); noise with T = 6000, where single selections refine more positions than the list holds, so
    that the full list's commit falls between the hint's load and the segment's; a resumed encode, maxRounds = 3, the
    caller's buffer overwritten between the rounds."""
import numpy as np
import pytest

from test_gpu_loop_bounds import _encode, _engine, _family, _identity, _same, _weights

pytestmark = pytest.mark.gpu

SHAPES = [(5, 2500, 50, 57), (6, 3000, 40, 32), (4, 1500, 33, 13)]


def _params(L0=60, **kw):
    from hsc_amd import _native
    return _native.make_params(nbNonzeroCoefs=L0, eps=1e-30, maxEvents=4096, **kw)


def _plant(x, b, D, k, p, amp):
    import hsc_amd.synth as synth
    s, e, es, ee = synth.centered_span(x.shape[1], D.shape[1], p)
    x[b, s:e] += amp * D[k].astype(np.float64)[es:ee]


def _wide_dictionary(K, W, seed):
    """Every entry (1 + m 2^-23) 2^e with a random 23-bit m, e uniform in -30 .. 29, random sign: inside the model of the
    bound pass (|d| in [2^-30, 2^30]), and nowhere near a sum of two bf16 values."""
    rs = np.random.RandomState(seed)
    bits = (rs.randint(0, 1 << 23, size=(K, W)).astype(np.uint32) | (rs.randint(127 - 30, 127 + 30, size=(K, W)).astype(np.uint32) << 23) |
            (rs.randint(0, 2, size=(K, W)).astype(np.uint32) << 31))
    D = bits.view(np.float32)
    assert np.all(np.abs(D) >= 2.0 ** -30) and np.all(np.abs(D) < 2.0 ** 30)
    return np.ascontiguousarray(D)


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['planted', 'noise'])
@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_image_offsets(kind, shape, weights):
    B, T, K, W = SHAPES[shape]
    x, D = _family(kind, B, T, K, W, 130 + shape)
    _identity(x, D, _weights(K, weights, shape), _params(60))


@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_full_significands_wide_magnitudes(shape, weights):
    """The atoms are far from unit norm, so the pursuit leaves the model (and float32) within a few atoms: the first
    selections run the bound tile and the chains on these entries, the later ones the fallback tile."""
    B, T, K, W = SHAPES[shape]
    D = _wide_dictionary(K, W, 140 + shape)
    x = np.random.RandomState(140 + shape).standard_normal((B, T)).astype(np.float32)
    _identity(x, D, _weights(K, weights, shape), _params(8))


# ---- (b) ----------------------------------------------------------------------------------------------------------------
OUTSIDE = [np.inf, np.nan, 2.0 ** 70, 2.0 ** -70]


@pytest.mark.parametrize('shape', range(len(SHAPES)))
def test_fallback_tile(shape):
    import hsc_amd.synth as synth
    _, T, K, W = SHAPES[shape]
    B = 2 * len(OUTSIDE)
    D = synth.make_dictionary(K, W, seed=150 + shape)
    x = np.stack([synth.make_signal(D, T, b, kind='planted', nb_atoms=12, noise=0.01, seed=150 + shape, return_events=False) for b in range(B)])
    w = _weights(K, True, shape)
    for b in range(B):
        p = 300 + 100 * b
        _plant(x, b, D, (3 + 5 * b) % K, p, 9.0 / float(w[(3 + 5 * b) % K]))       # the first atom of the signal
        s, e, _, _ = synth.centered_span(T, W, p)
        if b % 2 == 0:
            x[b, s + (W // 3) + b % 3] = OUTSIDE[b // 2]      # inside the atom's support
        else:
            x[b, e + 1 + b % 3] = OUTSIDE[b // 2]             # beside it: read by the rows p + 2 .. p + W - 1, not changed
    x = np.ascontiguousarray(x, dtype=np.float32)
    _identity(x, D, w, _params(30))


# ---- (c) ----------------------------------------------------------------------------------------------------------------
def _segment_winners(B, T, K, W, seg, seed, w=None):
    """Descending winners in the first segment, the last one, and at the last position of one segment and the first of the
    next (which of the two leads alternates from signal to signal); smaller atoms 1 % apart in between keep every
    selection refining."""
    import hsc_amd.synth as synth
    D = synth.make_dictionary(K, W, seed=seed)
    rs = np.random.RandomState(seed)
    x = 1e-4 * rs.standard_normal((B, T))
    nseg = (T + seg - 1) // seg
    last0 = (nseg - 1) * seg
    m = nseg // 2
    for b in range(B):
        pos = [seg // 2 + b, last0 + (T - 1 - last0) // 2, m * seg - 1, m * seg, (m + 5) * seg, (m + 5) * seg - 1]
        if b % 2:
            pos[2], pos[3] = pos[3], pos[2]
        for j, p in enumerate(pos):
            k = (7 * j + b) % K
            _plant(x, b, D, k, p, (8.0 - 0.5 * j) / (1.0 if w is None else float(w[k])))
        small = np.arange(3 * W, T - 3 * W, max(5 * W, T // 24))
        for j, p in enumerate(small):
            k = (3 * j + b) % K
            _plant(x, b, D, k, p, 2.0 * 1.01 ** ((j * 7 + b) % len(small)) / (1.0 if w is None else float(w[k])))
    return np.ascontiguousarray(x, dtype=np.float32), D


@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_winners_at_segment_boundaries(shape, weights):
    B, T, K, W = SHAPES[shape]
    w = _weights(K, weights, shape)
    x, D = _segment_winners(B, T, K, W, 64, 160 + shape, w)
    _identity(x, D, w, _params(40))


@pytest.mark.parametrize('T, seg', [(33000, 128), (66000, 256), (132000, 512)])
def test_winners_at_boundaries_of_longer_segments(T, seg):
    """512 segments at the most: 2, 4 and 8 stored scores per lane."""
    assert (T + seg - 1) // seg <= 512 < (T + seg // 2 - 1) // (seg // 2)
    w = _weights(33, True, 3)
    x, D = _segment_winners(4, T, 33, 13, seg, 170, w)
    _identity(x, D, w, _params(40))


@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_both_signal_ends(shape, weights):
    B, T, K, W = SHAPES[shape]
    x, D = _family('ends', B, T, K, W, 180 + shape)
    _identity(x, D, _weights(K, weights, shape), _params(60))


def test_both_signal_ends_even_width():
    x, D = _family('ends', 5, 2500, 50, 58, 185)                # (8 chunks, even W: the stale row T - 1)
    _identity(x, D, _weights(50, True, 5), _params(60))


@pytest.mark.parametrize('shape', range(len(SHAPES)))
@pytest.mark.parametrize('weights', [False, True])
def test_full_list_commit_inside_a_selection(shape, weights):
    B, _, K, W = SHAPES[shape]
    x, D = _family('noise', B, 6000, K, W, 190 + shape)
    _identity(x, D, _weights(K, weights, shape), _params(120))


@pytest.mark.parametrize('shape', range(len(SHAPES)))
def test_resumed_encode(shape):
    B, T, K, W = SHAPES[shape]
    w = _weights(K, True, shape)
    x, D = _segment_winners(B, T, K, W, 64, 200 + shape, w)
    eng = _engine(D, w)
    a = _encode(eng, x, _params(40, maxRounds=3), 'bound', rounds=3, scramble=np.float32(123.0))
    b = _encode(eng, x, _params(40, maxRounds=3), 'exact', rounds=3)
    c = _encode(eng, x, _params(40, maxRounds=3), 'exact_recorr', rounds=3, scramble=np.float32(-7.0))
    full = _encode(eng, x, _params(40), 'bound')
    assert full['variant'] == 'mfma_init+mfma_loop_f32_bound_x4', full['variant']
    _same(a, b)
    _same(a, c)
    _same(a, full)
