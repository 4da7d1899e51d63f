// block_pieces.h — how a stage call cuts one cache block into pieces: plain arithmetic, no HIP (tests/cpp/block_pieces_test.cpp runs it
// on the host).  The blocks themselves: HostArena, ResultBlocks and ChunkBlocks, api_internal.h.
#pragma once
#include <stddef.h>
#include <string.h>
#include <vector>

namespace hipstr {

// Pieces back to back in steps of 256 bytes; a piece of no bytes takes a step too, so no two pieces share an address.  What comes home
// is taken first and end_results() marks where it ends: one copy of [0, res) brings all of it, and only that much pinned memory is needed.
struct BlockPieces {
  size_t tot = 0, res = 0;
  size_t take(size_t bytes){ const size_t off = tot; tot = (tot + (bytes ? bytes : 1) + 255) & ~(size_t)255; return off; }
  void end_results(){ res = tot; }
};

// Host arrays that travel in one pinned block: the same steps, and where each piece's bytes come from.  add() returns a piece's offset;
// pack() copies every piece that has a source to its place (a piece without one is room the device fills).
struct HostPieces {
  struct Piece { const void* src; size_t bytes, off; };
  std::vector<Piece> pieces; size_t total = 0;
  size_t add(const void* src, size_t bytes){
    const size_t off = total; pieces.push_back(Piece{src, bytes, off}); total = (total + (bytes ? bytes : 1) + 255) & ~(size_t)255; return off;
  }
  void pack(char* block) const { for (const Piece& pc : pieces) if (pc.bytes && pc.src) memcpy(block + pc.off, pc.src, pc.bytes); }
};

}  // namespace hipstr
