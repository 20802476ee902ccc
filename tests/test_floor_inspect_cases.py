"""CPU: inspect_error_wave (k_floor.inc) on crafted ranges against a serial restatement of inspect_error.

tests/c/floor_inspect_cases.cpp, a program of its own built with -fsanitize=address,undefined against the one-lane
vocabulary (tests/emul): ranges of 1, 2, 63, 64, 65, 128 and 1024 points; ascending, flat and descending lines; the only
failing point at the first, the last and an interior place of every chunk of 64; candidate points that must not count
(class bit clear; a zero past the first point) and the zero first point that must; no failing point with the squared
error one below, at and one above (floor(maxerr) + 1) * cnt; the count thresholds against a large error; the integer and
the float form of the point tests.  Each range is a heap block of exactly the points visited, so a read past either end
is the sanitizer's to report.

This pins the logic of the walk that ends at the first failing chunk (VAMD_FL_INSPECT_STOP) and of the walk it
replaces; a chunk is one point in this build.  The 64-lane and the half-wave forms are tests/test_floor_split_gpu.py's.
"""
import pytest

from tests import hostbuild


@pytest.mark.parametrize("stop", [1, 0])
def test_inspect_error_wave_against_the_serial_walk(stop):
    hostbuild.run_ok(hostbuild.program("floor_inspect_cases.cpp", ["-DVAMD_FL_INSPECT_STOP=%d" % stop]))
