"""CPU: the feed's host arithmetic (vorbis_amd/csrc/vamd_feed_host.h) on crafted cases.

tests/c/feed_host_cases.cpp, a program of its own built with -fsanitize=address,undefined against the shipped header:
plan_slices over five streams of 0, 1, 11, 3 and 0 blocks with the size classes interleaved, at 1, 2, 5, 7, nb - 1, nb and
nb + 1 blocks per slice, every field of every slice against a brute-force restatement, and a plan out of stream order
refused; the comment table's image (own and shared comments, a vector shorter than the group, offsets, lengths, longest
and sum); the two record layouts' fields disjoint and aligned for (ns, nb) = (1, 0), (1, 1), (3, 5); the live mirror's two
steps at block sizes 256 / 2048 and 777 frames per write (an absent stream, a 1-frame piece, an early close, the buffer
bound, the rebase's bounds, a stream reopened).  Every array is a heap block of exactly the size visited, so a read or
write past either end is the sanitizer's to report.
"""
import os
import subprocess

from tests import checker

ROOT = checker.ROOT


def test_feed_host_arithmetic_on_crafted_cases(tmp_path):
    exe = str(tmp_path / "feed_host_cases")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vorbis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "feed_host_cases.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith(": ok"), r.stdout[-4000:] + r.stderr[-4000:]
