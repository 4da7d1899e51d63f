// block_pieces_test.cpp — stand-alone check of the piece arithmetic every stage call cuts its cache blocks with
// (hipstr_amd/csrc/block_pieces.h), meant to be built with -fsanitize=address,undefined (tests/test_block_pieces.py does):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/block_pieces_test.cpp -o block_pieces_test
// The offsets against the formula — a piece of b bytes starts where its predecessor's (b' ? b' : 1) bytes end, rounded up to 256 — for
// sizes of zero, on and around the step and large ones; the results' mark with pieces before it, behind it and on either side alone; and
// pieces written end to end into a buffer of exactly `tot` bytes: none overlaps another or leaves the buffer.  Prints "ok <pieces>".
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
  printf("ok %ld\n", pieces);
  return 0;
}
