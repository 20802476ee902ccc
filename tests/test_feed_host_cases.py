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
from tests import hostbuild


def test_feed_host_arithmetic_on_crafted_cases():
    hostbuild.run_ok(hostbuild.program("feed_host_cases.cpp", ["-Wall"]))
