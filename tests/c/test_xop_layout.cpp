// tests/c/test_xop_layout.cpp -- host check of the operand-form image of the shared spectra (sdr-server_amd/csrc/xl_xop_layout.h):
// an image written the way xlp_forward_kernel<M, 4, true> writes it -- workgroup = (pass, group of four branches), lane = (segment,
// bin), 16-byte slots at xop_bin_base() + xop_in_bin() -- and staged slot by slot the way xlp_mix_mfma_kernel<NKB, false, true> stages
// it (the re row as loaded, the im row derived from its bits) must equal, byte for byte, the LDS contents the converting staging of xlp_mix_mfma_kernel<NKB, false> writes from the
// float32 spectra of the same (pass, bin): NKB = 1 .. 8, D in {8, 21, 42, 64} and every other D that fits, the zero rows between D and
// 8 NKB included.  The float -> two halves split is restated here in integer arithmetic (round to nearest even, subnormal halves,
// no _Float16 needed from the host compiler); both sides use it, as both kernels use xlp_split_h.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sdr-server_amd/csrc/xl_xop_layout.h"

static const float XSCALE = 128.0f;  // XLP_H_XSCALE
static const uint32_t SEG = 16;      // XLP_SEG

static uint32_t f2u(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
static float u2f(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// float32 -> binary16 bits, round to nearest even
static uint16_t f2h(float f) {
  const uint32_t u = f2u(f), sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
  if (a >= 0x7F800000u) return (uint16_t)(sign | 0x7C00u | (a > 0x7F800000u ? 0x200u : 0u));
  if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // rounds to >= 2^16
  if (a < 0x33000000u) return (uint16_t)sign;               // < 2^-25: zero (2^-25 itself ties to even = 0)
  const int e = (int)(a >> 23) - 127;
  uint32_t mant = (a & 0x7FFFFFu) | 0x800000u;
  int shift = e >= -14 ? 13 : 13 + (-14 - e);  // bits dropped
  uint32_t q = mant >> shift, rem = mant & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
  if (rem > halfway || (rem == halfway && (q & 1u))) ++q;
  // normal: q in [2^10, 2^11] -> exponent field e + 15, mantissa q - 2^10 (a carry rolls into the exponent by plain addition)
  const uint32_t h = e >= -14 ? ((uint32_t)(e + 14) << 10) + q : q;
  return (uint16_t)(sign | h);
}
static float h2f(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, ex = (h >> 10) & 31u, m = h & 0x3FFu;
  float v;
  if (ex == 31u) return u2f(sign | 0x7F800000u | (m << 13));
  if (ex == 0u) v = ldexpf((float)m, -24);
  else v = ldexpf((float)(m | 0x400u), (int)ex - 25);
  return sign ? -v : v;
}
// xlp_split_h
static void split(float v, uint16_t &h1, uint16_t &h2) {
  h1 = f2h(v);
  h2 = f2h(v - h2f(h1));
}
static uint32_t pack(uint16_t lo, uint16_t hi) { return (uint32_t)lo | ((uint32_t)hi << 16); }
static uint16_t neg(uint16_t h) { return (uint16_t)(h ^ 0x8000u); }

static int failures = 0;
#define CHECK(c, ...)                \
  do {                               \
    if (!(c)) {                      \
      if (failures++ < 20) {         \
        printf("FAIL: " __VA_ARGS__); \
        printf("\n");                \
      }                              \
    }                                \
  } while (0)

struct Spectra {  // X[pass][m][b][segment] (re, im)
  uint32_t passes, M, D;
  std::vector<float> v;
  float &at(uint32_t pass, uint32_t m, uint32_t b, uint32_t s, uint32_t c) { return v[((((size_t)pass * M + m) * D + b) * SEG + s) * 2 + c]; }
};

// the converting staging of xlp_mix_mfma_kernel<NKB, false, false> for one (pass, bin): xs[term][k-block][slot][dword]
static void stage_old(Spectra &X, uint32_t nkb, uint32_t pass, uint32_t m, std::vector<uint32_t> &xs) {
  for (uint32_t w = 0; w < 4; ++w)
    for (uint32_t q = 0; q < (nkb + 3) / 4; ++q)
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t j = xlm_stage_kblock(w, q);
        if (j >= nkb) continue;
        const uint32_t bb = xlm_stage_branch_in_block(lane), sp = xlm_stage_segment_pair(lane), b = 8 * j + bb;
        float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (b < X.D)
          for (uint32_t e = 0; e < 4; ++e) g[e] = X.at(pass, m, b, 2 * sp + (e >> 1), e & 1u);
        uint16_t f1[4], f2[4];
        for (int e = 0; e < 4; ++e) split(g[e] * XSCALE, f1[e], f2[e]);
        for (uint32_t u = 0; u < 2; ++u) {
          const uint32_t sre = xlm_lds_slot(xlm_lane(xlm_half(bb), xlm_row(2 * sp + u, 0)));
          const uint32_t sim = xlm_lds_slot(xlm_lane(xlm_half(bb), xlm_row(2 * sp + u, 1)));
          xs[((0 * nkb + j) * 64 + sre) * 4 + xlm_dword(bb)] = pack(f1[2 * u], f1[2 * u + 1]);
          xs[((0 * nkb + j) * 64 + sim) * 4 + xlm_dword(bb)] = pack(f1[2 * u + 1], neg(f1[2 * u]));
          xs[((1 * nkb + j) * 64 + sre) * 4 + xlm_dword(bb)] = pack(f2[2 * u], f2[2 * u + 1]);
          xs[((1 * nkb + j) * 64 + sim) * 4 + xlm_dword(bb)] = pack(f2[2 * u + 1], neg(f2[2 * u]));
        }
      }
}

// the forward launch's epilogue: every workgroup (pass, group), every lane (segment h, bin m) -- whole 16-byte slots
static void forward_new(Spectra &X, uint32_t nkb, std::vector<uint32_t> &img, std::vector<uint8_t> &written) {
  const uint32_t ngrp = (X.D + XOP_GROUP - 1) / XOP_GROUP;
  for (uint32_t pass = 0; pass < X.passes; ++pass)
    for (uint32_t grp = 0; grp < ngrp; ++grp)
      for (uint32_t m = 0; m < X.M; ++m)
        for (uint32_t h = 0; h < SEG; ++h) {
          const uint32_t b0 = XOP_GROUP * grp;
          uint32_t hp[2][4];  // [term][n]: (re half, im half)
          for (uint32_t n = 0; n < XOP_GROUP; ++n) {
            uint16_t r1, r2, i1, i2;
            const bool real = b0 + n < X.D;
            split((real ? X.at(pass, m, b0 + n, h, 0) : 1.0f) * XSCALE, r1, r2);  // (the kernel transforms real samples there and drops them)
            split((real ? X.at(pass, m, b0 + n, h, 1) : -3.0f) * XSCALE, i1, i2);
            hp[0][n] = real ? pack(r1, i1) : 0u;
            hp[1][n] = real ? pack(r2, i2) : 0u;
          }
          for (uint32_t term = 0; term < 2; ++term) {
            const size_t slot = xop_bin_base(X.M, nkb, pass, m) + xop_in_bin(nkb, term, grp, h);
            CHECK((slot + 1) * 16 <= xop_bytes(X.passes, X.M, nkb), "slot %zu beyond the image", slot);
            CHECK(!written[slot], "slot %zu written twice", slot);
            written[slot] = 1;
            for (uint32_t n = 0; n < XOP_GROUP; ++n) {
              CHECK(hp[term][n] == xop_re_dword(hp[term][n] & 0xFFFFu, hp[term][n] >> 16), "xop_re_dword");
              img[slot * 4 + n] = hp[term][n];
            }
          }
        }
}

int main() {
  // the split itself, at the values the layout test leans on
  {
    uint16_t a, b;
    split(0.0f, a, b);
    CHECK(a == 0 && b == 0, "split(+0)");
    split(-0.0f, a, b);
    CHECK(a == 0x8000 && (b & 0x7FFF) == 0, "split(-0)");
    split(1.0f + ldexpf(1.0f, -12), a, b);  // second half 2^-12: normal
    CHECK(a == 0x3C00 && b == f2h(ldexpf(1.0f, -12)), "split(1 + 2^-12)");
    split(ldexpf(1.0f, -3) + ldexpf(1.0f, -20), a, b);  // second half 2^-20: subnormal
    CHECK(a == 0x3000 && b == 0x0010, "split(2^-3 + 2^-20): %04x %04x", a, b);
    CHECK(f2h(65504.0f) == 0x7BFF && f2h(65520.0f) == 0x7C00 && f2h(ldexpf(1.0f, -24)) == 1 && f2h(ldexpf(1.0f, -25)) == 0, "f2h edges");
    CHECK(f2h(2049.0f) == f2h(2048.0f) && f2h(2051.0f) == f2h(2052.0f), "ties to even");
  }
  const float big = (float)(256.0 * sqrt(2.0) * 127.5 / 128.0);  // times XLP_H_XSCALE: +-M sqrt 2 x 127.5, the bound of the cu8 spectra
  const float special[] = {0.0f, -0.0f, big, -big, ldexpf(1.0f, -10) + ldexpf(1.0f, -27), -(ldexpf(1.0f, -10) + ldexpf(1.0f, -29)),
                           ldexpf(1.0f, -40), 1.0f + ldexpf(1.0f, -11), -181.0193f, ldexpf(1.0f, -31)};
  const uint32_t nspecial = sizeof(special) / sizeof(special[0]);
  uint32_t cases = 0;
  for (uint32_t nkb = 1; nkb <= 8; ++nkb)
    for (uint32_t D = 8 * (nkb - 1) + 1; D <= 8 * nkb; ++D) {  // every D of the class (8, 21, 42, 64 among them)
      Spectra X;
      X.passes = 2, X.M = 3, X.D = D;  // (the index algebra is linear in M: three bins show every stride)
      X.v.resize((size_t)X.passes * X.M * D * SEG * 2);
      uint32_t rng = 12345u + 977u * D;
      for (size_t i = 0; i < X.v.size(); ++i) {
        rng = rng * 1664525u + 1013904223u;
        const uint32_t r = rng >> 8;
        X.v[i] = (r % 7u == 0u) ? special[(r / 7u) % nspecial] : ((float)(int32_t)(r & 0xFFFFu) - 32768.0f) * (362.0f / 32768.0f) * ((r >> 16) & 1u ? 1.0f : 1e-3f);
      }
      for (uint32_t k = 0; k < nspecial && k < X.v.size(); ++k) X.v[(size_t)k * 37u % X.v.size()] = special[k];
      // the image: cleared once (as the engine clears it), then written by the forward launch
      std::vector<uint32_t> img(xop_bytes(X.passes, X.M, nkb) / 4, 0u);
      std::vector<uint8_t> written(img.size() / 4, 0);
      forward_new(X, nkb, img, written);
      for (uint32_t pass = 0; pass < X.passes; ++pass)
        for (uint32_t m = 0; m < X.M; ++m) {
          const uint32_t nlds = 2u * nkb * 64u;  // xs[buf]: [term][k-block][slot]
          std::vector<uint32_t> want((size_t)nlds * 4, 0xDEADBEEFu), got((size_t)nlds * 4, 0x55555555u);
          stage_old(X, nkb, pass, m, want);
          // the mix's staging: slot i of the bin's part (thread tid, round q: i = tid + 256 q) -> its re row and its im row in xs[buf]
          for (uint32_t i = 0; i < xop_bin_slots(nkb); ++i) {
            const uint32_t *v = &img[(xop_bin_base(X.M, nkb, pass, m) + i) * 4];
            const uint32_t ire = xop_lds_index(i, 0), iim = xop_lds_index(i, 1);
            CHECK(ire < nlds && iim < nlds && got[(size_t)ire * 4] == 0x55555555u && got[(size_t)iim * 4] == 0x55555555u, "LDS slot written twice or out of range");
            for (uint32_t n = 0; n < 4; ++n) got[(size_t)ire * 4 + n] = v[n], got[(size_t)iim * 4 + n] = xop_im_dword(v[n]);
          }
          for (uint32_t term = 0; term < 2; ++term)
            for (uint32_t j = 0; j < nkb; ++j)
              for (uint32_t slot = 0; slot < 64; ++slot) {
                const size_t i = (size_t)(term * nkb + j) * 64 + slot;
                CHECK(memcmp(&got[i * 4], &want[i * 4], 16) == 0,
                      "nkb %u D %u pass %u bin %u term %u k-block %u slot %u: %08x %08x %08x %08x, staging writes %08x %08x %08x %08x", nkb, D, pass,
                      m, term, j, slot, got[i * 4], got[i * 4 + 1], got[i * 4 + 2], got[i * 4 + 3], want[i * 4], want[i * 4 + 1], want[i * 4 + 2],
                      want[i * 4 + 3]);
              }
        }
      // slots nobody wrote are exactly those of the groups beyond ceil(D / 4)
      const uint32_t ngrp = (D + XOP_GROUP - 1) / XOP_GROUP;
      size_t nw = 0;
      for (uint8_t f : written) nw += f;
      CHECK(nw == (size_t)X.passes * X.M * 2u * ngrp * 16u, "nkb %u D %u: %zu slots written", nkb, D, nw);
      ++cases;
    }
  if (failures) {
    printf("operand image layout: %d failures\n", failures);
    return 1;
  }
  printf("operand image layout: ok (%u classes)\n", cases);
  return 0;
}
