// vamd_arena.h -- the 16-byte rule every arena of the library is laid out by.  No HIP header: the context (vamd_ctx.h)
// and the host-side layouts a test program compiles (vamd_decode_layout.h) both include it.
#pragma once
#include <stddef.h>

// the layout of a host-pointer call's arena (pinned and device side alike): every part begins on a 16-byte boundary --
// the launch code chooses kernels by pointer alignment, and the mapped pinned arena is read and written in place
struct Arena {
  size_t at = 0;  // the arena's size so far
  size_t take(size_t bytes) {
    const size_t o = at;
    at = (at + bytes + 15) & ~(size_t)15;
    return o;
  }
};
