"""CPU suite: vamd_create() refuses a setup blob whose point-stereo amplitudes (vorbis_info_psy_global's
coupling_prepointamp / coupling_postpointamp) lie outside the nine stereo thresholds they index -- the host reads that
table through them when it binds the parameter block, so a value that is not 0 .. 8 must never get that far."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests.checker import ROOT
from tests.feed_cases import ABI, LIB


def _offsets():
    src = r'''#include <stdio.h>
#include <stddef.h>
#include "vamd_setup.h"
int main(void) {
  printf("%zu %zu %d\n", offsetof(vamd_setup_header, psy_g.coupling_prepointamp), offsetof(vamd_setup_header, psy_g.coupling_postpointamp),
         VAMD_PACKETBLOBS);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        return [int(v) for v in subprocess.check_output([os.path.join(d, "p")], text=True).split()]


@pytest.mark.parametrize("value", [-1, 9, 1 << 20, -(1 << 31)])
def test_point_amplitudes_outside_the_threshold_table_are_refused(value):
    L = C.CDLL(LIB)
    L.vamd_create_abi.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    good = np.fromfile(os.path.join(ROOT, "vorbis_amd", "data", "setup_44k_stereo_q4.bin"), dtype=np.uint8)
    pre, post, blobs = _offsets()
    for base in (pre, post):
        for k in (0, blobs // 2, blobs - 1):
            at = base + 4 * k
            assert 0 <= int(good[at:at + 4].view(np.int32)[0]) <= 8   # (the committed blob's own values are inside)
            b = good.copy()
            b[at:at + 4] = np.frombuffer(np.int32(value).tobytes(), np.uint8)
            h = C.c_void_p()
            assert L.vamd_create_abi(C.byref(h), b.ctypes.data_as(C.c_void_p), b.size, -1, ABI) == -131
            assert not h.value
