"""Run on the GPU with a -DVAMD_COUNT_CALLS build of the library (tools/fl_phases_pmc.sh, tools/build_variant.sh): what
the split loop of floor1_fit did per channel-block (the counters of k_floor.h).

  python tools/fl_calls.py [nb]        the bench's input (uniform noise, 44k_stereo_q4, long blocks), and the q 0.9 setup
                                       on long and on short blocks
  python tools/fl_calls.py --signals   every signal of tests/floor_split_signals.py on its own (64 blocks each): q4 long
                                       blocks, q9 short blocks

All through k_floor: k_floor_pair carries no stopwatch, so the pair path has no census (short blocks are counted in batches
below the size from which channels are paired; a half of a pair walks what a wave of k_floor walks, in chunks of 32).
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vorbis_amd

WANT = ("mdct", "logmask", "posts", "post_valid", "iwork", "nonzero", "ampmax_out")
HEAD = "%-34s %7s %7s %7s %7s %7s %7s %7s %7s %7s" % ("input", "inspect", "ret 1", "chunks", "point", "counts", "mse", "ret 0",
                                                       "memo", "most")


def census(name, W, pcm):
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(name), 0)
    nb = pcm.shape[0]
    flags = torch.full((nb,), W, dtype=torch.int32).cuda()
    kw = dict(W=W, lW=flags, nW=flags, blocktype=W, ampmax_in=-9999.0, want=WANT)
    an.analyze(pcm, **kw)
    torch.cuda.synchronize()
    an.debug_cycles(True)
    an.analyze(pcm, **kw)
    torch.cuda.synchronize()
    c = [float(x) for x in an.debug_cycles(False, read=True)[3][:8]]
    an.close()
    return [x / (nb * 2) for x in c], an.posts[W]


def row(label, c):
    calls, ones, chunks, point, counts, memo, most = c[0], c[1], c[2], c[3], c[4], c[5], c[6]
    print("%-34s %7.2f %7.2f %7.2f %7.2f %7.2f %7.2f %7.2f %7.2f %7.2f" %
          (label, calls, ones, chunks, point, counts, ones - point, calls - ones - counts, memo, most))


if __name__ == "__main__":
    print("per channel-block: inspect_error_wave calls, those returning 1, chunks walked, returns by the point test / the count "
          "thresholds / the mse test with 1 / with 0, split-loop trips ending at the memo test, sum of fit_line_pair's `most`")
    print(HEAD)
    if "--signals" in sys.argv:
        from tests import floor_split_signals as S
        for name, W, label in (("44k_stereo_q4", 1, "q4 long"), ("44k_stereo_q9", 0, "q9 short")):
            for kind in S.NAMES:
                rng = np.random.default_rng(11)
                pcm = np.stack([S.block(kind, 2, 2048 if W else 256, rng) for _ in range(64)]).astype(np.float32)
                c, posts = census(name, W, torch.from_numpy(pcm).cuda())
                row("%s %s" % (label, kind), c)
    else:
        nb = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
        torch.manual_seed(1)
        for name, W, label in (("44k_stereo_q4", 1, "bench: q4 long"), ("44k_stereo_q9", 1, "q9 long"), ("44k_stereo_q9", 0, "q9 short")):
            pcm = torch.rand((nb if W else min(nb, 4096), 2, 2048 if W else 256), device="cuda") - 0.5
            c, posts = census(name, W, pcm)
            row("%s, %d posts" % (label, posts), c)
