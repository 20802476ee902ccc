"""CPU: the decoder's plan image (vorbis_amd/csrc/vamd_decode_layout.h), the layout the kernels read.

tests/c/decode_layout_host.cpp, a program of its own built with -fsanitize=address,undefined against the shipped header.
decode_layout over pages absent / present x live x byte carry (live and pages) x windows x segments, with every count a
call of that kind has in {0, 1, 3} (nb, nlap, ns, both src lists, npg, nin, nout, nbin, nbout, nseg): every part on a
16-byte boundary, the non-empty parts pairwise disjoint and inside [0, plan_bytes), the statuses at or behind plan_bytes,
o.unpack == o.order exactly when the call is not live.  decode_image_fill for a hand-made plan of three packets, plain and
live, with and without begin[], with and without the window lists, planar and interleaved: the lists in the image as
given, the bits rows 8 * (at - byte0) and 8 * (at + len - byte0), a frameless stream's offset_out as 0, the segment rows'
out scaled by the channels under interleaving alone; the image lies between guard bytes, and every list handed in is a
heap block of exactly its count.
"""
from tests import hostbuild


def test_decode_layout_and_image_on_the_host():
    hostbuild.run_ok(hostbuild.program("decode_layout_host.cpp", ["-Wall"]))
