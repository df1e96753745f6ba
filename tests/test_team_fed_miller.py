"""The fed team Miller loop on the host (tests/native/fedsim.cpp): line records walked by
miller_lines_walk, scaled by the pair's P and laid out pair-major as k_lines_team writes them,
read back lane by lane as a k_miller_team_fed team does, the accumulator through the tm_emu team
operations.  After a final exponentiation the fed value equals miller_loop1's for a signature
pair (P = -G1) and for a pubkey-sum pair (Jacobian P, Z != 1), both over a Jacobian Q with
Z != 1; a pair that takes no part gives 1 and writes nothing; writer and reader agree on the
record offsets for pair 0 and pair cap - 1 of a capacity that is no multiple of 64.  Run as a
stand-alone program, at -O2 and under AddressSanitizer + UBSan."""
import pytest

from tests import fedsim

WANT = (
    "sig: final_exp(fed) == final_exp(miller_loop1)",
    "pk: final_exp(fed) == final_exp(miller_loop1)",
    "dead: the team's value is 1",
    "dead: the buffer is untouched",
    "offsets: records are whole, 16-byte aligned, contiguous per pair, inside the buffer",
    "offsets: exactly two pairs' words were written",
)


@pytest.mark.parametrize("kind", ["O2", "san"])
def test_fed_loop_on_the_host(kind):
    code, lines, err = fedsim.run(kind)
    print("\n".join(lines))
    assert code == 0, (lines, err[-2000:])
    assert lines and all(ln.startswith("ok ") for ln in lines), lines
    names = {ln[3:] for ln in lines}
    for w in WANT:
        assert w in names, w
