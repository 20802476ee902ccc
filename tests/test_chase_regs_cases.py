"""CPU: the stack walk with its window in registers (tone_chase_regs<8>, k_tone.h) against a plain walk on an unbounded
stack and against the ring walk it replaces in the lane-per-block kernel (tone_chase_ring<8>).

tests/c/chase_regs_cases.cpp, a program of its own built with -fsanitize=address,undefined against the one-lane
vocabulary (tests/emul).  Every sequence of 14 lines over three values (4 782 969 of them); seeded random rows of 777
and 585 lines and of every length from 1 to 40 (the end of a row inside a trip of 32 lines, rows shorter than the
window); all lines equal (VAMD_NEGINF: the silent block); strictly rising and strictly falling rows; sawteeth of period
7, 8 and 9, both ways up (pops that reach exactly to the window's edge, and one short of it).  Compared: the survivor
list, the count, that the list is byte for byte the ring walk's, and that nothing is written beyond the count.  Rows and
lists are heap blocks of exactly the padded sizes, so a step outside is the sanitizer's to report.
"""
from tests import hostbuild


def test_register_walk_against_the_plain_walk_and_the_ring_walk():
    exe = hostbuild.program("chase_regs_cases.cpp")
    stdout = hostbuild.run_ok(exe)
    print(stdout)
    assert "exhaustive: 4782969 sequences" in stdout and " 0 mismatches: ok" in stdout
