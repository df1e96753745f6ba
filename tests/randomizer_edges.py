"""Edge words for the 64-bit batch randomizer k, applied as r = lo32(k) + hi32(k) x^2 (mod the group
order) by jac_mul_glv (bls_curve.h: signed radix-16 digits d_j in [-7, 8] and a top carry per half,
c_8 for the low half and c_8' for the high one), tg1_mul_glv (bgv_tg1.h) and tc_mul_glv
(bgv_tcurve.h: unsigned 2-bit windows, an `inf` flag that picks the accumulator's source bank), and
the seed that puts a chosen word into a chosen slot.  Test infrastructure only; no test in here.

Slot i's randomizer is the i-th nonzero splitmix64 word of the seed, mix(seed + (i + 1) GAMMA), in the
debug hooks (bgv_calls.cpp debug_slots) and in the product path under bgv_set_rng_seed
(bgv_sched.cpp fill_scalars).  mix is a bijection on 64 bits, so seed = unmix(k) - (i + 1) GAMMA.
"""
from oracle import bls12381 as o

MASK64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
M1, M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB

# The halves.  Radix-16 view (jac_mul_glv) / 2-bit view (tg1_mul_glv, tc_mul_glv):
HALVES = [
    1, 2, 3,           # one addition, in the last window only; the three 2-bit table entries
    7, 8, 9,           # digit 7 (no carry), digit 8 (kept as +8, no carry), 9 = -7 + carry into d_1
    0x40000000, 0x80000000, 0xC0000000,  # a single top digit: 2-bit 1, 2, 3; radix-16 4, 8 and 0xC = -4 with c_8
    0x55555555, 0xAAAAAAAA,  # every 2-bit digit 1 / 2; radix-16 5s with no carry / 0xA = -6, -5, ... with every carry
    0x77777777, 0x88888888,  # the largest digits that do not carry: all 7, all 8 (c_8 clear)
    0x88888889,        # the low 9 carries and every 8 + 1 after it carries: the whole chain up to c_8
    0x99999999,        # -7, -6, -6, ...: a carry out of every digit, c_8 set
    0xFFFFFFFF,        # all-ones: every 2-bit digit 3; radix-16 -1, 0, 0, ... and c_8
]


def _edge_words():
    ws = []
    # The high half zero: every b-digit is 0 and c_8' is clear, the b-additions are computed and
    # dropped (jac_glv_step's select, the 2-bit schedules' bank 4 -> 4) in every window.
    ws += [h for h in HALVES]
    # The low half zero: the accumulator stays at infinity through the whole a-digit stream, the `inf`
    # flag is still set when the first b-digit arrives and the first finite value comes from the
    # endomorphism table (banks 6-8, E(T[m - 1])); with c_8' set it is infinity + E(P) before the loop.
    ws += [h << 32 for h in HALVES]
    # The same digit in both halves of every window: entry and E(entry) of one table index added back
    # to back; c_8 and c_8' both set for the last three, the last-window-only addition twice for 1.
    ws += [(h << 32) | h for h in (1, 3, 8, 0x88888889, 0xAAAAAAAA, 0xFFFFFFFF)]
    # Crosses: c_8 without c_8' beside a last-window-only b-addition, and the reverse (c_8' entering
    # an accumulator still at infinity); c_8' with an all-7 low half (no carry) and c_8 with an all-7
    # high half; the full carry chain in the high half over a lone digit 7 in the low one.
    ws += [(1 << 32) | 0xFFFFFFFF, (0xFFFFFFFF << 32) | 1, (0x99999999 << 32) | 0x77777777,
           (0x77777777 << 32) | 0x99999999, (0x88888889 << 32) | 7]
    out = []
    for w in ws:
        if w and w not in out:
            out.append(w)
    return out


EDGE_WORDS = _edge_words()


def _mix(z):
    z = ((z ^ (z >> 30)) * M1) & MASK64
    z = ((z ^ (z >> 27)) * M2) & MASK64
    return z ^ (z >> 31)


def _unxorshift(z, s):
    """The y with y ^ (y >> s) == z."""
    y, k = z, s
    while k < 64:
        y = z ^ (y >> s)
        k += s
    return y


def _unmix(w):
    z = _unxorshift(w, 31)
    z = (z * pow(M2, -1, 1 << 64)) & MASK64
    z = _unxorshift(z, 27)
    z = (z * pow(M1, -1, 1 << 64)) & MASK64
    return _unxorshift(z, 30)


def seed_for(word, slot):
    """The seed whose slot-th (0-based) nonzero splitmix64 word is `word`."""
    from tools.gen_golden_r04 import randomizers
    assert 0 < word <= MASK64 and slot >= 0
    seed = (_unmix(word) - (slot + 1) * GAMMA) & MASK64
    assert _mix((seed + (slot + 1) * GAMMA) & MASK64) == word
    assert seed != 0, "seed 0 asks bgv_set_rng_seed for getrandom words"
    # a zero word earlier in the stream would shift the index
    assert randomizers(seed, slot + 1)[slot][0] == word, (hex(word), slot)
    return seed


def glv_scalar(word):
    """The randomizer a word stands for: lo32 + hi32 x^2 mod the group order."""
    return ((word & 0xFFFFFFFF) + (word >> 32) * o.X * o.X) % o.R
