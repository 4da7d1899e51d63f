// block_pieces.h — how a stage call cuts one cache block into pieces: plain arithmetic, no HIP (tests/cpp/block_pieces_test.cpp runs it
// on the host).  The blocks themselves: ResultBlocks and ChunkBlocks, api_internal.h.
#pragma once
#include <stddef.h>

namespace hipstr {

// Pieces back to back in steps of 256 bytes; a piece of no bytes takes a step too, so no two pieces share an address.  What comes home
// is taken first and end_results() marks where it ends: one copy of [0, res) brings all of it, and only that much pinned memory is needed.
struct BlockPieces {
  size_t tot = 0, res = 0;
  size_t take(size_t bytes){ const size_t off = tot; tot = (tot + (bytes ? bytes : 1) + 255) & ~(size_t)255; return off; }
  void end_results(){ res = tot; }
};

}  // namespace hipstr
