"""GPU suite (-m gpu): the stack walk with one lane per channel-block and its window in registers (k_tone_chase_regs: no
ring, no LDS) on small batches, every block bit for bit against the CPU checker and every survivor list against a plain
walk of the seed lines the device itself produced.

The lane-per-block kernel is what large batches run; here it is forced on small ones with the knobs the library reads
(VAMD_TEST_KNOBS=1 VAMD_CHASE_WAVE_MAX=0), in a fresh child process per setting, once with six and once with seven noise
teams a CU beside it (VAMD_NOISE_TEAMS); the child asserts from the library's config string that the register walk is
the one in use.  Shapes: 1 stereo block (two lanes of a wave); 33 stereo blocks (66 channel-blocks: a full wave and a wave
of two lanes); 65 mono blocks (a full wave and one lane); 40 short stereo blocks of a setup whose short blocks have 585
lines (not a multiple of the 32 a trip reads).  Signals: tests/tone_fold_signals.py, in turn.  The checker's taps are
computed once, in the parent, and handed to both children.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import checker, tone_fold_signals

pytestmark = pytest.mark.gpu
# (setup, size class, blocks)
SHAPES = (("44k_stereo_q4", 1, 1), ("44k_stereo_q4", 1, 33), ("44k_mono_q5", 1, 65), ("44k_stereo_q9", 0, 40))
KEYS = ("logmask",)  # (+ posts: compare_block takes them when both sides have them)
_ref_file = {}


def batch(name, n, nb):
    """[nb][ch][n]: the signals in turn, starting with noise so that a single block is not the silent one."""
    sig = tone_fold_signals.blocks(checker.SETUPS[name][0], n)
    return np.ascontiguousarray(sig[[(3 + b) % len(sig) for b in range(nb)]])


def plain_walk(seed, linesper):
    """seed_chase's stack discipline (lib/psy.c:454-487) on a list that simply grows; returns the surviving lines."""
    pos, amp = [], []
    for i, s in enumerate(seed):
        while (len(pos) >= 2 and not s < amp[-1] and i < pos[-1] + linesper and amp[-1] <= amp[-2]
               and i < pos[-2] + linesper):
            pos.pop()
            amp.pop()
        pos.append(i)
        amp.append(s)
    return pos


def references(tmp_path_factory):
    """The file with every shape's input and checker taps (one per distinct signal block), written once."""
    if "path" not in _ref_file:
        import vorbis_amd
        from tests.feed_cases import chk_for
        out = {}
        for name, W, nb in SHAPES:
            if (name, W) in out:
                continue
            an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(name), device=0)
            n, nposts = an.blocksizes[W], an.posts[W]
            an.close()
            pcm = batch(name, n, len(tone_fold_signals.NAMES))
            chk = chk_for(name)
            out[(name, W)] = (n, nposts, [chk.tap_block(pcm[k], W, W, W, W, -9999.0) for k in range(len(pcm))])
        path = str(tmp_path_factory.mktemp("chase_regs") / "refs.pkl")
        with open(path, "wb") as f:
            pickle.dump(out, f)
        _ref_file["path"] = path
    return _ref_file["path"]


def child(path):
    """Runs in the child: every shape under the environment it was started with."""
    import torch
    import vorbis_amd
    refs = pickle.load(open(path, "rb"))
    nsig = len(tone_fold_signals.NAMES)
    bad = []
    for name, W, nb in SHAPES:
        n, nposts, ref = refs[(name, W)]
        ch = checker.SETUPS[name][0]
        an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(name), device=0)
        config = an.config_string().split()
        assert "VAMD_CHASE_WAVE_MAX=0" in config and "VAMD_NOISE_TEAMS=" + os.environ["VAMD_NOISE_TEAMS"] in config, config
        assert "chase_walk=regs,regs" in config, config  # the register walk for both size classes
        flags = torch.full((nb,), W, dtype=torch.int32).cuda()
        outs = an.analyze(torch.from_numpy(batch(name, n, nb)).cuda(), W=W, lW=flags, nW=flags, blocktype=W, ampmax_in=-9999.0,
                          want=KEYS + ("posts",))
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        seed, surv, nsurv, nl = an.debug_survivors(W, nb * ch)
        an.close()
        for b in range(nb):  # every block
            if checker.compare_block(ref[b % nsig], {k: v[b] for k, v in got.items()}, nposts, keys=KEYS, verbose=len(bad) < 3):
                bad.append((name, W, nb, "block", b))
        for cb in range(nb * ch):  # every channel-block's survivor list
            want = plain_walk(seed[cb, :nl].tolist(), 8)
            if nsurv[cb] != len(want) or surv[cb, :len(want)].tolist() != want:
                bad.append((name, W, nb, "survivors", cb, int(nsurv[cb]), len(want)))
    print("CHASE REGS CHILD: %d differences %s" % (len(bad), bad[:8]))
    return 1 if bad else 0


@pytest.mark.parametrize("teams", [6, 7])
def test_register_walk_on_small_batches(teams, tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    path = references(tmp_path_factory)
    env = dict(os.environ, VAMD_TEST_KNOBS="1", VAMD_CHASE_WAVE_MAX="0", VAMD_NOISE_TEAMS=str(teams))
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.test_chase_regs_gpu", path],
                       cwd=checker.ROOT, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "CHASE REGS CHILD: 0 differences" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]


if __name__ == "__main__":
    sys.exit(child(sys.argv[1]))
