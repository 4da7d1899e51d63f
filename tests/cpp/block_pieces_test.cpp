// block_pieces_test.cpp — stand-alone check of the piece arithmetic every stage call cuts its cache blocks with
// (hipstr_amd/csrc/block_pieces.h), meant to be built with -fsanitize=address,undefined (tests/test_block_pieces.py does):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/block_pieces_test.cpp -o block_pieces_test
// The offsets against the formula — a piece of b bytes starts where its predecessor's (b' ? b' : 1) bytes end, rounded up to 256 — for
// sizes of zero, on and around the step and large ones; the results' mark with pieces before it, behind it and on either side alone; and
// pieces written end to end into a buffer of exactly `tot` bytes: none overlaps another or leaves the buffer.  HostPieces, the list with
// sources: the same offsets as take(), and pack() into a block of exactly `total` bytes — every piece with a source lands at its offset,
// a piece without one (and the gaps) stays as it was, also when only the pieces before the first one without a source are given room.
// Prints "ok <pieces>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hipstr_amd/csrc/block_pieces.h"

#define CHECK(c) do { if (!(c)){ fprintf(stderr, "block_pieces_test: %s failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

static size_t up256(size_t n){ return (n + 255)/256*256; }

int main(){
  const size_t sizes[] = { 0, 1, 4, 255, 256, 257, 511, 512, 513, 0, 0, 1000, 65536, 65537, (size_t)3 << 20, 0 };
  const size_t n_sizes = sizeof sizes/sizeof sizes[0];
  long pieces = 0;
  // every split of the list into results | rest
  for (size_t n_res = 0; n_res <= n_sizes; n_res++){
    hipstr::BlockPieces P;
    CHECK(P.tot == 0 && P.res == 0);
    std::vector<size_t> off(n_sizes);
    size_t want = 0;
    for (size_t i = 0; i < n_sizes; i++){
      if (i == n_res){ P.end_results(); CHECK(P.res == want); }
      off[i] = P.take(sizes[i]);
      CHECK(off[i] == want && off[i] % 256 == 0);
      want += up256(sizes[i] ? sizes[i] : 1);
      CHECK(P.tot == want);
      pieces++;
    }
    if (n_res == n_sizes){ P.end_results(); CHECK(P.res == want); }
    CHECK(P.res <= P.tot && P.res % 256 == 0);
    // the results are exactly the pieces taken before the mark: the last of them ends inside [0, res), the first of the rest starts at res
    if (n_res > 0) CHECK(off[n_res - 1] + sizes[n_res - 1] <= P.res);
    if (n_res < n_sizes) CHECK(off[n_res] == P.res);
    // each piece filled with its own byte in a buffer of tot bytes (the sanitizer watches the ends), then read back
    std::vector<unsigned char> buf(P.tot, 0xEE);
    for (size_t i = 0; i < n_sizes; i++) if (sizes[i]) memset(buf.data() + off[i], (int)(i + 1), sizes[i]);
    for (size_t i = 0; i < n_sizes; i++)
      for (size_t k = 0; k < sizes[i]; k += (sizes[i] > 4096 ? 4095 : 1)) CHECK(buf[off[i] + k] == (unsigned char)(i + 1));
    // a block of the results' size holds every results' piece (what the pinned side gets)
    std::vector<unsigned char> home(P.res ? P.res : 1);
    for (size_t i = 0; i < n_res; i++) if (sizes[i]) memcpy(home.data() + off[i], buf.data() + off[i], sizes[i]);
  }
  // one piece alone: zero bytes take a step, so the block is never empty
  { hipstr::BlockPieces P; CHECK(P.take(0) == 0 && P.tot == 256); P.end_results(); CHECK(P.res == 256 && P.take(0) == 256 && P.tot == 512 && P.res == 256); pieces += 2; }
  // sizes near the top of 32 bits: size_t arithmetic, no wrap
  { hipstr::BlockPieces P; const size_t big = ((size_t)1 << 32) - 1; CHECK(P.take(big) == 0 && P.tot == (size_t)1 << 32 && P.take(big) == (size_t)1 << 32 && P.tot == (size_t)1 << 33); pieces += 2; }
  // HostPieces: sources of every size, every third piece without one; then the staged form of a posterior run: room for the leading pieces only
  {
    hipstr::HostPieces H; hipstr::BlockPieces P;
    std::vector<std::vector<unsigned char>> src(n_sizes);
    for (size_t i = 0; i < n_sizes; i++){
      src[i].assign(sizes[i], (unsigned char)(i + 1));
      const bool given = i % 3 != 2;
      CHECK(H.add(given ? src[i].data() : NULL, sizes[i]) == P.take(sizes[i]) && H.total == P.tot && H.pieces.size() == i + 1);
      CHECK(H.pieces[i].bytes == sizes[i] && H.pieces[i].off + sizes[i] <= H.total);
      pieces++;
    }
    std::vector<char> block(H.total, (char)0xEE);
    H.pack(block.data());
    for (size_t i = 0; i < n_sizes; i++)
      for (size_t k = 0; k < sizes[i]; k += (sizes[i] > 4096 ? 4095 : 1)) CHECK((unsigned char)block[H.pieces[i].off + k] == (i % 3 != 2 ? (unsigned char)(i + 1) : 0xEE));
    hipstr::HostPieces S;
    const unsigned char a[300] = {7}, b[5] = {9};
    CHECK(S.add(a, sizeof a) == 0 && S.add(b, sizeof b) == 512);
    const size_t in_total = S.total;
    CHECK(in_total == 768 && S.add(NULL, 1000) == 768 && S.add(NULL, 0) == 1792 && S.total == 2048);
    std::vector<char> staged(in_total, (char)0xEE);          // (the sanitizer watches the end: pack() must not touch the pieces without a source)
    S.pack(staged.data());
    CHECK(staged[0] == 7 && staged[299] == 0 && (unsigned char)staged[300] == 0xEE && staged[512] == 9 && (unsigned char)staged[517] == 0xEE);
    pieces += 4;
  }
  printf("ok %ld\n", pieces);
  return 0;
}
