// Poseidon2 over the 31-bit fields: the permutation and the hash of one message, as one lane computes them. No HIP runtime in here, so
// tests/poseidon2_host_harness.cpp compiles the same code with g++. The kernels over it are poseidon2.hip, the parameters
// poseidon2_params.h.
//
// The state of T words stays in registers: T is a template argument, every state index a compile-time constant. The state is in
// Montgomery form (SmallField<PR>) from the moment it is loaded until the digest is stored, and so are the constants in memory.
// The rounds are one rolled loop with the full and the partial round behind a branch that is uniform over the grid, so that each
// round body exists once per (field, T); within a round everything is unrolled.
//   full round     x_i = (x_i + c_i)^alpha for all i, then M_E
//   partial round  x_0 = (x_0 + c)^alpha, then M_I
//   M_E            t = 2, 3: x_i + sum(x). t = 4: M4 by its addition chain of 8 additions and 4 doublings (Poseidon2, section 5.1).
//                  t = 4k: M4 on every group of four, then x_(4g+j) += sum over the groups of x_(4h+j) -- 2 M4 on the diagonal.
//   M_I            sum(x) + (d_i - 1) x_i, the d_i - 1 stored behind the round constants
// Semantics of the reference's CPU backend (backend/cpu/src/hash/cpu_poseidon2.cpp): the digest is state[1]. A message of exactly T
// elements (T - 1 with a domain tag, which then is state[0]) is one permutation; every permutation starts with one M_E. Any other
// size is a sponge over a zero state: state[0] is the tag or else the first element, the rest is added into state[1 .. T-1], T - 1
// elements per permutation, an incomplete last block is padded with 1, 0, 0, .. (a complete one is not padded); fewer than T
// elements are one permutation.
#pragma once
#include <cstdint>
#include <vector>
#include "hash_readers.hpp"
#include "smallfield.hpp"

namespace icicle_hip {

  // smallest a >= 3 coprime to p - 1, at compile time (poseidon2_params.h derives the same at run time)
  constexpr int poseidon2_alpha(uint32_t p)
  {
    for (int a = 3;; a++) {
      uint32_t x = p - 1, y = (uint32_t)a;
      while (y) {
        const uint32_t r = x % y;
        x = y, y = r;
      }
      if (x == 1) return a;
    }
  }

  // what a lane needs beside its message
  struct Poseidon2Ctx {
    const uint32_t* consts; // Montgomery: r_f T + r_p round constants in round order, then T values d_i - 1
    int half_f, r_p;        // r_f / 2 full rounds, r_p partial rounds, r_f / 2 full rounds
    uint32_t tag;           // Montgomery
    uint32_t has_tag;       // 0 or 1
  };

  // host: the constants as Poseidon2Ctx::consts points to them, from the canonical round constants and the diagonal of M_I
  template <class PR>
  inline std::vector<uint32_t> poseidon2_device_constants(const std::vector<uint32_t>& rc, const std::vector<uint32_t>& diag)
  {
    using F = SmallField<PR>;
    std::vector<uint32_t> out;
    out.reserve(rc.size() + diag.size());
    for (uint32_t v : rc)
      out.push_back(F::to_mont(v));
    for (uint32_t d : diag)
      out.push_back(F::to_mont(F::sub(d, 1)));
    return out;
  }

  // element i of a message
  struct Poseidon2Words { // 4-aligned
    const uint32_t* p;
    ICICLE_HD uint32_t elem(uint64_t i) const { return p[i]; }
  };
  struct Poseidon2Padded { // a layer-0 chunk of a tree that reaches into the padding
    ReadPadded rd;
    ICICLE_HD uint32_t elem(uint64_t i) const { return rd.byte(4 * i) | rd.byte(4 * i + 1) << 8 | rd.byte(4 * i + 2) << 16 | rd.byte(4 * i + 3) << 24; }
  };

  template <class PR, int T>
  struct Poseidon2 {
    using F = SmallField<PR>;
    static constexpr int ALPHA = poseidon2_alpha(PR::P);
    static_assert(ALPHA == 3 || ALPHA == 7, "S-box of BabyBear (x^7) and KoalaBear (x^3)");
    static_assert(T == 2 || T == 3 || (T % 4 == 0 && T >= 4 && T <= 24), "width");

    static ICICLE_HD uint32_t sbox(uint32_t x)
    {
      const uint32_t x2 = F::mul(x, x), x3 = F::mul(x2, x);
      if constexpr (ALPHA == 3) {
        return x3;
      } else {
        return F::mul(F::mul(x3, x3), x);
      }
    }
    static ICICLE_HD uint32_t dbl(uint32_t x) { return F::add(x, x); }

    static ICICLE_HD void external(uint32_t (&s)[T])
    {
      if constexpr (T < 4) {
        uint32_t sum = s[0];
#pragma unroll
        for (int i = 1; i < T; i++)
          sum = F::add(sum, s[i]);
#pragma unroll
        for (int i = 0; i < T; i++)
          s[i] = F::add(s[i], sum);
      } else {
#pragma unroll
        for (int g = 0; g < T; g += 4) { // rows (5 7 1 3), (4 6 1 1), (1 3 5 7), (1 1 4 6)
          const uint32_t t0 = F::add(s[g], s[g + 1]), t1 = F::add(s[g + 2], s[g + 3]);
          const uint32_t t2 = F::add(dbl(s[g + 1]), t1), t3 = F::add(dbl(s[g + 3]), t0);
          const uint32_t t4 = F::add(dbl(dbl(t1)), t3), t5 = F::add(dbl(dbl(t0)), t2);
          s[g] = F::add(t3, t5), s[g + 1] = t5, s[g + 2] = F::add(t2, t4), s[g + 3] = t4;
        }
        if constexpr (T > 4) {
          uint32_t col[4];
#pragma unroll
          for (int j = 0; j < 4; j++) {
            col[j] = s[j];
#pragma unroll
            for (int g = 4; g < T; g += 4)
              col[j] = F::add(col[j], s[g + j]);
          }
#pragma unroll
          for (int i = 0; i < T; i++)
            s[i] = F::add(s[i], col[i & 3]);
        }
      }
    }

    static ICICLE_HD void internal(uint32_t (&s)[T], const uint32_t* dm1)
    {
      uint32_t sum = s[0];
#pragma unroll
      for (int i = 1; i < T; i++)
        sum = F::add(sum, s[i]);
#pragma unroll
      for (int i = 0; i < T; i++)
        s[i] = F::add(sum, F::mul(dm1[i], s[i]));
    }

    static ICICLE_HD void permute(uint32_t (&s)[T], const Poseidon2Ctx& c)
    {
      external(s);
      const uint32_t* rc = c.consts;
      const uint32_t* dm1 = c.consts + (2 * c.half_f * T + c.r_p);
      const int rounds = 2 * c.half_f + c.r_p;
#pragma unroll 1
      for (int r = 0; r < rounds; r++) {
        if (r < c.half_f || r >= c.half_f + c.r_p) {
#pragma unroll
          for (int i = 0; i < T; i++)
            s[i] = sbox(F::add(s[i], rc[i]));
          external(s);
          rc += T;
        } else {
          s[0] = sbox(F::add(s[0], rc[0]));
          internal(s, dm1);
          rc += 1;
        }
      }
    }

    // the digest of the n elements of rd, canonical
    template <class RD>
    static ICICLE_HD uint32_t hash(const RD& rd, uint64_t n, const Poseidon2Ctx& c)
    {
      uint32_t s[T];
      const uint64_t tagged = c.has_tag;
      const bool exact = n == (uint64_t)T - tagged;
      const uint64_t off = 1 - tagged, rest = n - off; // without a tag the first element is state[0]; n >= 1 then
      s[0] = tagged ? c.tag : F::to_mont(rd.elem(0));
#pragma unroll
      for (int i = 1; i < T; i++)
        s[i] = exact ? F::to_mont(rd.elem(i - tagged)) : 0;
      const uint64_t blocks = exact || rest + 1 < (uint64_t)T + tagged ? 1 : (rest + T - 2) / (T - 1);
      // one call site of the permutation
#pragma unroll 1
      for (uint64_t b = 0; b < blocks; b++) {
        if (!exact) {
#pragma unroll
          for (int i = 0; i < T - 1; i++) {
            const uint64_t idx = b * (T - 1) + i;
            uint32_t v = 0;
            if (idx < rest)
              v = F::to_mont(rd.elem(off + idx));
            else if (idx == rest) // reached only inside an incomplete last block
              v = F::one();
            s[1 + i] = F::add(s[1 + i], v);
          }
        }
        permute(s, c);
      }
      return F::from_mont(s[1]);
    }
  };

} // namespace icicle_hip
