"""Run on the GPU with a -DVAMD_COUNT_CALLS build of the library (tools/fl_phases_pmc.sh): calls of inspect_error_wave
and of the split loop's fit_line_pair per channel-block of the bench's input (uniform noise, 44k_stereo_q4, long blocks)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import vorbis_amd
nb = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob("44k_stereo_q4"), 0)
pcm = torch.rand((nb, 2, 2048), device="cuda") - 0.5
outs = an.alloc_outputs(1, nb, ("mdct", "logmask", "posts", "post_valid", "iwork", "nonzero", "ampmax_out"))
an.reserve(1, nb)
an.analyze(pcm, outs=outs)
torch.cuda.synchronize()
an.debug_cycles(True)
an.analyze(pcm, outs=outs)
torch.cuda.synchronize()
c = an.debug_cycles(False, read=True)
cb = nb * 2
print("calls per channel-block over %d: inspect_error_wave %.2f  fit_line_pair (split loop) %.2f   posts %d" %
      (cb, float(c[3][0]) / cb, float(c[3][1]) / cb, an.posts[1]))
