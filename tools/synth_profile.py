"""k_synth by phase: the in-kernel stopwatch (vamd_debug_cycles) over a batch of blocks through vamd_analyze_batch_synth, beside
k_transform's own phases over the same blocks in the same launch sequence.  Ticks are summed over a block's waves (one per
channel) and divided by the blocks; a phase's share is what matters, the waves of a CU overlap.

    python tools/synth_profile.py [setup] [blocks]
"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import vorbis_amd

setup = sys.argv[1] if len(sys.argv) > 1 else "44k_stereo_q4"
nb = int(sys.argv[2]) if len(sys.argv) > 2 else 32768
an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(setup), 0)
torch.manual_seed(0)
SYNTH = ("residue walk", "coupling + floor", "mdct: rotate", "mdct: butterfly stages", "mdct: 32-point groups", "mdct: bit-reverse + tail")
for W in (1, 0):
    n = an.blocksizes[W]
    t = torch.arange(n, device="cuda") / 44100.0  # a tone over noise: every residue stage has entries
    pcm = (0.4 * torch.sin(2 * torch.pi * 440.0 * t)[None, None, :] + (torch.rand((nb, an.channels, n), device="cuda") - 0.5) * 0.3).contiguous()
    outs = an.alloc_outputs(W, nb, ("synth",))
    args = dict(W=W, lW=W, nW=W, blocktype=1 if W else 0, outs=outs)
    for _ in range(2):
        an.analyze(pcm, **args)
    torch.cuda.synchronize()
    an.debug_cycles(True)
    an.analyze(pcm, **args)
    torch.cuda.synchronize()
    c = an.debug_cycles(False, read=True)
    row = [float(x) / nb / 1e3 for x in c[0]]
    total = sum(row[8:14])
    print("W=%d, %d blocks of %d samples x %d channels; kcycles per block, summed over its waves" % (W, nb, n, an.channels))
    print("  k_transform (marks 1..7: window+fold, butterfly stages, 32-point groups, bit-reverse, spectra out, FFT, logfft): %s  sum %.2f"
          % (" ".join("%.2f" % x for x in row[1:8]), sum(row[:8])))
    for name, x in zip(SYNTH, row[8:14]):
        print("  k_synth  %-26s %7.2f  %5.1f %%" % (name, x, 100.0 * x / total))
    print("  k_synth  %-26s %7.2f" % ("sum", total))
