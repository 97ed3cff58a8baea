// Poseidon2 over Goldilocks, p = 2^64 - 2^32 + 1: the permutation and the hash of one message, as one lane computes them. No HIP
// runtime in here, so tests/poseidon2_gold_host_harness.cpp compiles the same code with g++. The kernels over it are
// poseidon2_gold.hip, the parameters poseidon2_gold_params.h.
//
// The layout is that of poseidon2.hpp: the state of T elements stays in registers, T is a template argument and every state index
// a compile-time constant; the rounds are one rolled loop with the full and the partial round behind a branch that is uniform over
// the grid, and within a round everything is unrolled. What differs is the arithmetic (goldfield.hpp): an element is one canonical
// 64-bit value, there is no Montgomery form, and a product is 64 x 64 -> 128 bits reduced by the shape of p
// (FieldOps<goldilocks_params>::reduce128). The S-box is x^7 for every width: x^2, x^3 = x^2 x, x^4 = (x^2)^2, x^7 = x^3 x^4.
//   full round     x_i = (x_i + c_i)^7 for all i, then M_E
//   partial round  x_0 = (x_0 + c)^7, then M_I
//   M_E            t = 2, 3: x_i + sum(x). t = 4: M4 by its addition chain of 8 additions and 4 doublings (Poseidon2, section 5.1).
//                  t = 4k: M4 on every group of four, then x_(4g+j) += sum over the groups of x_(4h+j) -- 2 M4 on the diagonal.
//                  Computed on lazy 128-bit sums of the canonical inputs -- an output is at most 16 * 7 = 112 inputs, below 2^71 --
//                  with one reduce128 per output; profiles/poseidon2_notes.md has this form timed against canonical additions.
//   M_I            sum(x) + (d_i - 1) x_i, the d_i - 1 stored behind the round constants. The d_i are full 64-bit values, so this is
//                  a product per element; the 128-bit product (at most (p - 1)^2 = 2^128 - 2^97 + ..) and the sum of T <= 24
//                  canonical values (below 2^69) are added before the one reduce128 that serves both.
// The semantics are those stated at the top of poseidon2.hpp, from the reference's backend/cpu/src/hash/cpu_poseidon2.cpp: the
// digest is state[1]; a message of exactly T elements (T - 1 beside a tag, which then is state[0]) is one permutation; any other
// size is a sponge over a zero state, T - 1 elements per permutation, only an incomplete last block padded with 1, 0, 0, ..; a
// message shorter than T is one permutation. An input word in [p, 2^64) is brought below p, as FieldOps<goldilocks_params>::unpack.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "goldfield.hpp"
#include "hash_readers.hpp"

namespace icicle_hip {

  // what a lane needs beside its message
  struct Poseidon2GoldCtx {
    const uint64_t* consts; // canonical: r_f T + r_p round constants in round order, then T values d_i - 1
    int half_f, r_p;        // r_f / 2 full rounds, r_p partial rounds, r_f / 2 full rounds
    uint64_t tag;           // canonical
    uint32_t has_tag;       // 0 or 1
  };

  // host: the constants as Poseidon2GoldCtx::consts points to them, from the round constants and the diagonal of M_I
  inline std::vector<uint64_t> poseidon2_gold_device_constants(const std::vector<uint64_t>& rc, const std::vector<uint64_t>& diag)
  {
    std::vector<uint64_t> out(rc);
    out.reserve(rc.size() + diag.size());
    for (uint64_t d : diag)
      out.push_back(d ? d - 1 : goldilocks_params::P - 1);
    return out;
  }

  // element i of a message, as stored: any 64-bit word
  struct Poseidon2GoldWords { // 8-aligned
    const uint8_t* p;
    ICICLE_HD uint64_t elem(uint64_t i) const { return ReadAligned{p, false}.word(8 * i); }
  };
  struct Poseidon2GoldPadded { // a layer-0 chunk of a tree that reaches into the padding
    ReadPadded rd;
    ICICLE_HD uint64_t elem(uint64_t i) const { return rd.word(8 * i); }
  };

  template <int T>
  struct Poseidon2Gold {
    using F = FieldOps<goldilocks_params>;
    static constexpr uint64_t P = goldilocks_params::P;
    static_assert(T == 2 || T == 3 || (T % 4 == 0 && T >= 4 && T <= 24), "width");

    // a 128-bit value below 2^128 as two words: the lazy sums of both linear layers
    struct Wide {
      uint64_t lo, hi;
    };
    static ICICLE_HD Wide wide(uint64_t v) { return Wide{v, 0}; }
    static ICICLE_HD Wide wadd(const Wide& a, const Wide& b)
    {
      const uint64_t lo = a.lo + b.lo;
      return Wide{lo, a.hi + b.hi + (lo < a.lo ? 1u : 0u)};
    }
    static ICICLE_HD Wide wdbl(const Wide& a) { return Wide{a.lo << 1, a.hi << 1 | a.lo >> 63}; }
    static ICICLE_HD Wide wmul(uint64_t a, uint64_t b)
    {
#if defined(__HIP_DEVICE_COMPILE__)
      return Wide{a * b, __umul64hi(a, b)};
#else
      const unsigned __int128 m = (unsigned __int128)a * b;
      return Wide{(uint64_t)m, (uint64_t)(m >> 64)};
#endif
    }
    static ICICLE_HD uint64_t wreduce(const Wide& a) { return F::reduce128(a.hi, a.lo); }

    static ICICLE_HD uint64_t canon(uint64_t v) { return v >= P ? v - P : v; }
    static ICICLE_HD uint64_t add(uint64_t a, uint64_t b) { return F::add(F::make(a), F::make(b)).v; }
    static ICICLE_HD uint64_t mul(uint64_t a, uint64_t b) { return F::mul(F::make(a), F::make(b)).v; }

    static ICICLE_HD uint64_t sbox(uint64_t x)
    {
      const uint64_t x2 = mul(x, x), x3 = mul(x2, x), x4 = mul(x2, x2);
      return mul(x3, x4);
    }

    static ICICLE_HD void external(uint64_t (&s)[T])
    {
      if constexpr (T < 4) {
        Wide sum = wide(s[0]);
#pragma unroll
        for (int i = 1; i < T; i++)
          sum = wadd(sum, wide(s[i]));
#pragma unroll
        for (int i = 0; i < T; i++)
          s[i] = wreduce(wadd(sum, wide(s[i])));
      } else {
        Wide w[T];
#pragma unroll
        for (int g = 0; g < T; g += 4) { // rows (5 7 1 3), (4 6 1 1), (1 3 5 7), (1 1 4 6)
          const Wide a = wide(s[g]), b = wide(s[g + 1]), c = wide(s[g + 2]), d = wide(s[g + 3]);
          const Wide t0 = wadd(a, b), t1 = wadd(c, d);
          const Wide t2 = wadd(wdbl(b), t1), t3 = wadd(wdbl(d), t0);
          const Wide t4 = wadd(wdbl(wdbl(t1)), t3), t5 = wadd(wdbl(wdbl(t0)), t2);
          w[g] = wadd(t3, t5), w[g + 1] = t5, w[g + 2] = wadd(t2, t4), w[g + 3] = t4;
        }
        if constexpr (T > 4) {
          Wide col[4];
#pragma unroll
          for (int j = 0; j < 4; j++) {
            col[j] = w[j];
#pragma unroll
            for (int g = 4; g < T; g += 4)
              col[j] = wadd(col[j], w[g + j]);
          }
#pragma unroll
          for (int i = 0; i < T; i++)
            w[i] = wadd(w[i], col[i & 3]);
        }
#pragma unroll
        for (int i = 0; i < T; i++)
          s[i] = wreduce(w[i]);
      }
    }

    static ICICLE_HD void internal(uint64_t (&s)[T], const uint64_t* dm1)
    {
      Wide sum = wide(s[0]);
#pragma unroll
      for (int i = 1; i < T; i++)
        sum = wadd(sum, wide(s[i]));
#pragma unroll
      for (int i = 0; i < T; i++)
        s[i] = wreduce(wadd(wmul(dm1[i], s[i]), sum)); // (p - 1)^2 + 24 (p - 1) < 2^128
    }

    static ICICLE_HD void permute(uint64_t (&s)[T], const Poseidon2GoldCtx& c)
    {
      external(s);
      const uint64_t* rc = c.consts;
      const uint64_t* dm1 = c.consts + (2 * c.half_f * T + c.r_p);
      const int rounds = 2 * c.half_f + c.r_p;
#pragma unroll 1
      for (int r = 0; r < rounds; r++) {
        if (r < c.half_f || r >= c.half_f + c.r_p) {
#pragma unroll
          for (int i = 0; i < T; i++)
            s[i] = sbox(add(s[i], rc[i]));
          external(s);
          rc += T;
        } else {
          s[0] = sbox(add(s[0], rc[0]));
          internal(s, dm1);
          rc += 1;
        }
      }
    }

    // the digest of the n elements of rd, canonical
    template <class RD>
    static ICICLE_HD uint64_t hash(const RD& rd, uint64_t n, const Poseidon2GoldCtx& c)
    {
      uint64_t s[T];
      const uint64_t tagged = c.has_tag;
      const bool exact = n == (uint64_t)T - tagged;
      const uint64_t off = 1 - tagged, rest = n - off; // without a tag the first element is state[0]; n >= 1 then
      s[0] = tagged ? c.tag : canon(rd.elem(0));
#pragma unroll
      for (int i = 1; i < T; i++)
        s[i] = exact ? canon(rd.elem(i - tagged)) : 0;
      const uint64_t blocks = exact || rest + 1 < (uint64_t)T + tagged ? 1 : (rest + T - 2) / (T - 1);
      // one call site of the permutation
#pragma unroll 1
      for (uint64_t b = 0; b < blocks; b++) {
        if (!exact) {
#pragma unroll
          for (int i = 0; i < T - 1; i++) {
            const uint64_t idx = b * (T - 1) + i;
            uint64_t v = 0;
            if (idx < rest)
              v = canon(rd.elem(off + idx));
            else if (idx == rest) // reached only inside an incomplete last block
              v = 1;
            s[1 + i] = add(s[1 + i], v);
          }
        }
        permute(s, c);
      }
      return s[1];
    }
  };

} // namespace icicle_hip
