"""The three bf16 planes of the bound loop (csrc/hscmp_bound.h), on the CPU.

The four-signal loop keeps the dictionary only as bf16 planes hi = rn(v), lo = rn(v - hi), rem = (v - hi) - lo, and its
exact chains rebuild every float32 tap as (hi + lo) + rem.  hscmp_set_dictionary checks the rebuild element by element;
this test runs the same arithmetic (bf16_split, bf16_rem) over every float32 of the dictionary model, |v| in
[2^-30, 2^30], both signs: the rem plane is a bf16 and the rebuild is bitwise v for all of them."""
import numpy as np

LO_BITS = 0x30800000        # 2^-30
HI_BITS = 0x4E800000        # 2^30
CHUNK = 1 << 24


def _rn_bits(b):
    """bf16_rn_bits: round to nearest even, as float32 bit patterns (uint32)."""
    return (b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)


def _check(bits):
    v = bits.view(np.float32)
    hb = _rn_bits(bits)
    r = v - hb.view(np.float32)                               # exact
    lb = _rn_bits(r.view(np.uint32))
    rf = r - lb.view(np.float32)
    rb = rf.view(np.uint32)
    qb = rb & np.uint32(0xffff0000)
    back = (hb.view(np.float32) + lb.view(np.float32)) + qb.view(np.float32)
    ok = ((rb & np.uint32(0xffff)) == 0) & (back.view(np.uint32) == bits)
    return int(np.count_nonzero(~ok))


def test_rebuild_is_exact_over_the_model_range():
    bad = 0
    n = 0
    with np.errstate(all='raise'):
        for start in range(LO_BITS, HI_BITS + 1, CHUNK):
            bits = np.arange(start, min(start + CHUNK, HI_BITS + 1), dtype=np.uint32)
            bad += _check(bits)
            bad += _check(bits | np.uint32(0x80000000))
            n += 2 * bits.size
    assert n == 2 * (HI_BITS - LO_BITS + 1)
    assert bad == 0


def test_rebuild_fails_where_it_should_not_be_trusted():
    """The check is not vacuous: dropping the rem plane, or a rem that is not a bf16, is caught."""
    v = np.array([1.0 + 2.0 ** -20, -3.0000002, 1234.5677], dtype=np.float32)
    bits = v.view(np.uint32)
    hb = _rn_bits(bits)
    r = v - hb.view(np.float32)
    lb = _rn_bits(r.view(np.uint32))
    assert np.any((hb.view(np.float32) + lb.view(np.float32)).view(np.uint32) != bits)
    assert _check(bits) == 0
