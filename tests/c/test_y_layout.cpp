// tests/c/test_y_layout.cpp -- host check of the mixed-spectra image Y (sdr-server_amd/csrc/xl_y_layout.h): the address the mix
// kernels store element (column group, segment, column, bin) at equals the one the inverse kernels load it from -- the tile's base
// plus bin * CW + column in the tile --, the map covers the image exactly once, every tile is one contiguous run of M * CW elements,
// and xly_bytes is the size the engine has always allocated.  M in {64, 128, 256}, 1 and 3 column groups, 1 and 5 segments.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sdr-server_amd/csrc/xl_y_layout.h"

static int fails = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      if (fails++ < 10) printf(__VA_ARGS__);   \
    }                                          \
  } while (0)

int main() {
  const uint32_t Ms[3] = {64u, 128u, 256u}, ncgs[2] = {1u, 3u}, caps[2] = {1u, 5u};
  for (uint32_t M : Ms)
    for (uint32_t ncg : ncgs)
      for (uint32_t cap : caps) {
        const uint32_t CW = xly_tile_columns(M), NSUB = XLY_COLS / CW;
        CHECK(CW * NSUB == XLY_COLS && (size_t)M * CW * 8u == 32768u, "M %u: a tile is not 32 KB of whole columns\n", M);
        const size_t bytes = xly_bytes(ncg, cap, M), n = bytes / 8u;
        CHECK(bytes == (size_t)ncg * cap * M * XLY_COLS * 8u, "M %u ncg %u cap %u: xly_bytes = %zu\n", M, ncg, cap, bytes);
        CHECK(xly_seg_stride(M) == (size_t)M * XLY_COLS, "M %u: segment stride %zu\n", M, xly_seg_stride(M));
        std::vector<uint8_t> seen(n, 0);
        for (uint32_t cg = 0; cg < ncg; ++cg)
          for (uint32_t s = 0; s < cap; ++s) {
            for (uint32_t sub = 0; sub < NSUB; ++sub) {  // tiles: whole multiples of a tile, in (cg, s, sub) order back to back
              const size_t t = xly_tile(cap, M, cg, s, sub);
              CHECK(t == (((size_t)cg * cap + s) * NSUB + sub) * M * CW, "M %u: tile (%u, %u, %u) at %zu\n", M, cg, s, sub, t);
            }
            for (uint32_t col = 0; col < XLY_COLS; ++col)
              for (uint32_t m = 0; m < M; ++m) {
                const size_t e = xly_elem(cap, M, cg, s, col, m);  // the writers' address
                const size_t r = xly_tile(cap, M, cg, s, col / CW) + (size_t)m * CW + col % CW;  // the readers'
                CHECK(e == r, "M %u ncg %u cap %u: (cg %u, s %u, col %u, m %u) written at %zu, read at %zu\n", M, ncg, cap, cg, s, col, m, e, r);
                CHECK(e == xly_row(cap, M, cg, s, col, m) + xly_col_in_tile(M, col), "M %u: row + column of (%u, %u, %u, %u)\n", M, cg, s, col, m);
                // the mix kernels take segment 0 and step by the segment stride
                CHECK(e == xly_elem(cap, M, cg, 0u, col, m) + s * xly_seg_stride(M), "M %u: segment step of (%u, %u, %u, %u)\n", M, cg, s, col, m);
                // inside its tile's run
                const size_t t = xly_tile(cap, M, cg, s, col / CW);
                CHECK(e >= t && e < t + (size_t)M * CW, "M %u: (%u, %u, %u, %u) outside its tile\n", M, cg, s, col, m);
                if (e < n) {
                  CHECK(!seen[e], "M %u ncg %u cap %u: element %zu addressed twice\n", M, ncg, cap, e);
                  seen[e] = 1;
                } else {
                  CHECK(false, "M %u ncg %u cap %u: element %zu beyond the image of %zu\n", M, ncg, cap, e, n);
                }
              }
          }
        size_t covered = 0;
        for (size_t i = 0; i < n; ++i) covered += seen[i];
        CHECK(covered == n, "M %u ncg %u cap %u: %zu of %zu elements addressed\n", M, ncg, cap, covered, n);
      }
  if (fails) {
    printf("Y layout: %d FAILURES\n", fails);
    return 1;
  }
  printf("Y layout: ok\n");
  return 0;
}
