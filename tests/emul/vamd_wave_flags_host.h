// tests/emul/vamd_wave_flags_host.h -- TEST BUILD ONLY (see vamd_wave_host.h).
//
// The one-lane forms of the lane-mask members of the wave vocabulary (vamd_wave.h: wave_flags, wave_flags_any): the
// mask of one lane is its own condition.
#pragma once

namespace vamd {

VAMD_DEV unsigned long long wave_flags(bool pred) { return pred ? 1ull : 0ull; }
VAMD_DEV bool wave_flags_any(unsigned long long m) { return m != 0ull; }

}  // namespace vamd
