"""CPU: the stack walk's ring of 8 slots (tone_chase_ring, k_tone.h) against a plain walk on an unbounded stack.

tests/c/chase_ring_cases.cpp, a program of its own built with -fsanitize=address,undefined against the one-lane
vocabulary (tests/emul).  Rings of 8 and of 16 slots, windows of eight lines: every sequence of 14 lines over three
values (4 782 969 of them); seeded rows of 777 and 585 lines -- random values with and without ties, descending and
ascending staircases, plateaus of 1 to 40 equal values, stretches of VAMD_NEGINF, and rows that drive the stack up and
take it down six deep on a line, line after line; the kernel's [slot][lane] layout at stride 64 for lanes 0 and 63, the
other lanes' slots untouched; windows shorter than eight lines on eight slots, longer ones on sixteen, and the choice
tone_chase_thread makes from linesper.  Rows, rings and survivor lists are heap blocks of exactly the sizes the walk may
touch, so a step outside is the sanitizer's to report.

The guard of the read-back (a slot reused by the index a ring-length above) is compiled in with a counter, in this
program only.  It decides no step anywhere above -- the program fails if it does -- which is what k_tone.h's comment
argues: with linesper <= ring the guard is unreachable, and the library is built WITHOUT it.  That the counter works is
shown on windows of 16 lines over 8 slots, a pair the library never runs, where it must move.
"""
import pytest

from tests import hostbuild


@pytest.mark.parametrize("prefetch", [0, 1])
def test_ring_of_8_and_16_against_the_plain_walk(prefetch):
    """prefetch: VAMD_CHASE_PREFETCH, how the walk fetches its row (0 as shipped: everything; 1, the earlier form: the seeded rows)."""
    exe = hostbuild.program("chase_ring_cases.cpp", ["-DVAMD_CHASE_PREFETCH=%d" % prefetch] + (["-DCHASE_CASES_SEEDED_ONLY"] if prefetch else []))
    stdout = hostbuild.run_ok(exe)
    print(stdout)
    assert "guard: decided 0 steps" in stdout
