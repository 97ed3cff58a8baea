// Poseidon2 over the 256-bit scalar fields: the permutation and the hash of one message, as one lane computes them. No HIP runtime in
// here, so tests/poseidon2_wide_host_harness.cpp compiles the same code with g++ (with -DBIGFIELD_BOUNDS the bound tracker of
// bigfield.hpp runs over every operation below). The kernels over it are poseidon2_wide.hip, the parameters
// poseidon2_wide_params.h.
//
// The semantics are those of poseidon2.hpp, which states them, over elements of 32 bytes: the digest is state[1]; every
// permutation opens with one M_E; a message is absorbed T - 1 elements per permutation into state[1 ..] over a zero state whose
// state[0] is the tag or else the first element, and only an incomplete last block is padded, with 1, 0, 0, .. A message of
// exactly T elements (T - 1 beside a tag) is the one-block case of that rule, so it has no path of its own here.
//
// The state of T elements stays in registers, in Montgomery form on nine 29-bit limbs (FieldOps<PR>) from load to store; the
// constants in memory are Montgomery limbs too, read through a pointer that is the same for every lane. The rounds are one rolled
// loop with the full and the partial round behind a branch that is uniform over the grid.
//   S-box          x^5 (BN254, Grumpkin, BLS12-381), x^11 by three squarings and two products (BLS12-377), x^3 (stark252): chosen
//                  at compile time from p, checked by the host against the derived alpha when a hasher is made
//   M_E            t = 2, 3: x_i + sum(x). t = 4: M4 by its addition chain. t = 8: M4 per group, then the column sums.
//   M_I            t = 4, 8: sum(x) + (d_i - 1) x_i, one product per element. t = 2, 3: the diagonal is (2, 3), (2, 2, 3), so d_i - 1 is
//                  1 or 2 and the layer is additions only (the host checks the derived diagonal)
// Bounds (units of p; R / p is 64 for BLS12-381 and more for the others, and no stored element may pass 64). The linear layers are
// lazy additions, and what keeps them in range is a few conditional subtractions (below<..>), placed by running the bound tracker
// over all five fields, not by eye:
//   an S-box input is below 14, its output then below 1.3 (x^5 at R / p = 64: 14^2 / 64 + 1 = 4.1, 4.1^2 / 64 + 1 = 1.26, 1.26 * 14 / 64 + 1)
//   M_E multiplies the bound by 3, 4, 16, 48 (its largest row sum): its input is an S-box output, or the reduced state when a
//   permutation opens; its output is brought below 4 (t = 2, 3: one subtraction) or 8 (t = 4: two, t = 8: four)
//   M_I, t = 4, 8: the sum of the state (below 1.3 + 3 * 9.2 and 1.3 + 7 * 8) is brought below 8 and 4 (two and five subtractions
//   on one element), a product is below 1.2, so the state stays below 9.2 and 5.2
//   M_I, t = 2, 3: x_0 is a fresh S-box output; x_1 = sum + x_1 (and at t = 2 sum + 2 x_1) is below 1.3 + 3 * 4 and takes two
//   subtractions back below 4, x_2 = sum + 2 x_2 below 1.3 + 16 takes three
#pragma once
#include <cstdint>
#include <vector>
#include "bigfield.hpp"
#include "hash_readers.hpp"
#include "poseidon.hpp" // PoseidonWords, PoseidonPadded: element i of a message as 8 little-endian words

namespace icicle_hip {

  constexpr int POSEIDON2_WIDE_LIMBS = 9; // of one constant

  // smallest a >= 3 coprime to p - 1, at compile time (poseidon2_wide_params.h derives the same at run time)
  template <class PR>
  constexpr int poseidon2_wide_alpha()
  {
    for (uint32_t a = 3;; a++) {
      uint64_t r = 0;
      for (int i = PR::NL32 - 1; i >= 0; i--)
        r = ((r << 32) | PR::P32[i]) % a;
      uint32_t x = a, y = (uint32_t)((r + a - 1) % a); // gcd(a, (p - 1) mod a)
      while (y) {
        const uint32_t q = x % y;
        x = y, y = q;
      }
      if (x == 1) return (int)a;
    }
  }

  // what a lane needs beside its message
  struct Poseidon2WideCtx {
    const uint32_t* consts; // Montgomery limbs, 9 per entry: r_f T + r_p round constants in round order, then T values d_i - 1
    int half_f, r_p;        // r_f / 2 full rounds, r_p partial rounds, r_f / 2 full rounds
    uint32_t has_tag;       // 0 or 1
    uint32_t tag[POSEIDON2_WIDE_LIMBS]; // Montgomery
  };

  // host: the constants as Poseidon2WideCtx::consts points to them. rc, diag: reduced Montgomery elements as derived
  template <class PR>
  inline std::vector<uint32_t> poseidon2_wide_device_constants(const std::vector<Fe<PR>>& rc, const std::vector<Fe<PR>>& diag)
  {
    using F = FieldOps<PR>;
    std::vector<uint32_t> out;
    out.reserve(POSEIDON2_WIDE_LIMBS * (rc.size() + diag.size()));
    for (const Fe<PR>& e : rc)
      out.insert(out.end(), e.l, e.l + POSEIDON2_WIDE_LIMBS);
    for (const Fe<PR>& d : diag) {
      const Fe<PR> m = F::reduce(F::template sub<1>(d, F::reduce(F::one())));
      out.insert(out.end(), m.l, m.l + POSEIDON2_WIDE_LIMBS);
    }
    return out;
  }

  template <class PR, int T>
  struct Poseidon2Wide {
    using F = FieldOps<PR>;
    using fe = Fe<PR>;
    static constexpr int N = PR::NL;
    static constexpr int ALPHA = poseidon2_wide_alpha<PR>();
    static_assert(N == POSEIDON2_WIDE_LIMBS && PR::NL32 == 8, "a 256-bit field on nine limbs");
    static_assert(ALPHA == 3 || ALPHA == 5 || ALPHA == 11, "S-box of stark252 (x^3), BN254 / Grumpkin / BLS12-381 (x^5) and BLS12-377 (x^11)");
    static_assert(T == 2 || T == 3 || T == 4 || T == 8, "width");

    static ICICLE_HD fe load(const uint32_t* c)
    {
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = c[i];
      BF_SET_BOUND(r, 1);
      return r;
    }

    // conditional subtractions of 16 p, 8 p, .. that take x from below FROM p to below TO p (powers of two; FROM <= 64)
    template <int FROM, int TO>
    static ICICLE_HD void below(fe& x)
    {
      static_assert(FROM <= 64 && TO >= 1 && TO <= 16, "range");
      if constexpr (FROM > 48) F::template cond_sub<16>(x);
      if constexpr (FROM > 32) F::template cond_sub<16>(x);
      if constexpr (FROM > 16) F::template cond_sub<16>(x);
      if constexpr (FROM > 8 && TO <= 8) F::template cond_sub<8>(x);
      if constexpr (FROM > 4 && TO <= 4) F::template cond_sub<4>(x);
      if constexpr (FROM > 2 && TO <= 2) F::template cond_sub<2>(x);
      if constexpr (FROM > 1 && TO <= 1) F::template cond_sub<1>(x);
    }

    static ICICLE_HD fe sbox(const fe& x)
    {
      const fe x2 = F::sqr(x);
      if constexpr (ALPHA == 3) {
        return F::mul(x2, x);
      } else if constexpr (ALPHA == 5) {
        return F::mul(F::sqr(x2), x);
      } else {
        const fe x8 = F::sqr(F::sqr(x2));
        return F::mul(F::mul(x8, x2), x);
      }
    }

    // rows (5 7 1 3), (4 6 1 1), (1 3 5 7), (1 1 4 6): 8 additions and 4 doublings (Poseidon2, section 5.1)
    static ICICLE_HD void m4(fe& a, fe& b, fe& c, fe& d)
    {
      const fe t0 = F::add(a, b), t1 = F::add(c, d);
      const fe t2 = F::add(F::dbl(b), t1), t3 = F::add(F::dbl(d), t0);
      const fe t4 = F::add(F::dbl(F::dbl(t1)), t3), t5 = F::add(F::dbl(F::dbl(t0)), t2);
      a = F::add(t3, t5), b = t5, c = F::add(t2, t4), d = t4;
    }

    // input below 1.3, output below 4 (T < 4) or 8
    static ICICLE_HD void external(fe (&s)[T])
    {
      if constexpr (T < 4) {
        fe sum = s[0];
#pragma unroll
        for (int i = 1; i < T; i++)
          sum = F::add(sum, s[i]);
#pragma unroll
        for (int i = 0; i < T; i++) {
          s[i] = F::add(s[i], sum);
          below<8, 4>(s[i]);
        }
      } else if constexpr (T == 4) {
        m4(s[0], s[1], s[2], s[3]);
#pragma unroll
        for (int i = 0; i < T; i++)
          below<32, 8>(s[i]);
      } else {
        m4(s[0], s[1], s[2], s[3]);
        m4(s[4], s[5], s[6], s[7]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const fe col = F::add(s[j], s[4 + j]);
          s[j] = F::add(s[j], col), s[4 + j] = F::add(s[4 + j], col);
          below<64, 8>(s[j]);
          below<64, 8>(s[4 + j]);
        }
      }
    }

    // s[0] is an S-box output; the rest below 4 (T < 4), 9.2 (T = 4) or 8 (T = 8), and so again on return
    static ICICLE_HD void internal(fe (&s)[T], const uint32_t* dm1)
    {
      fe sum = s[0];
#pragma unroll
      for (int i = 1; i < T; i++)
        sum = F::add(sum, s[i]);
      if constexpr (T < 4) {
        s[0] = F::add(sum, s[0]);
        if constexpr (T == 3) {
          s[1] = F::add(sum, s[1]);
          below<16, 4>(s[1]);
        }
        s[T - 1] = F::add(sum, F::dbl(s[T - 1]));
        below<(T == 3 ? 32 : 16), 4>(s[T - 1]);
      } else {
        if constexpr (T == 4)
          below<32, 8>(sum);
        else
          below<64, 4>(sum);
#pragma unroll
        for (int i = 0; i < T; i++)
          s[i] = F::add(sum, F::mul(load(dm1 + i * N), s[i]));
      }
    }

    // the wide state keeps the S-boxes of a full round rolled, as poseidon.hpp does and for its reason: registers cannot be indexed
    // by a loop counter, so the loop works at the ends of the array and moves the rest down by one place
    static constexpr bool ROLLED = T > 4;
    static ICICLE_HD void shift_in(fe (&a)[T], const fe& x)
    {
#pragma unroll
      for (int i = 0; i + 1 < T; i++)
        a[i] = a[i + 1];
      a[T - 1] = x;
    }

    // every element enters below p
    static ICICLE_HD void permute(fe (&s)[T], const Poseidon2WideCtx& c)
    {
      external(s);
      const uint32_t* rc = c.consts;
      const uint32_t* dm1 = c.consts + (size_t)N * (2 * c.half_f * T + c.r_p);
      const int rounds = 2 * c.half_f + c.r_p;
#pragma unroll 1
      for (int r = 0; r < rounds; r++) {
        if (r < c.half_f || r >= c.half_f + c.r_p) {
          if constexpr (ROLLED) {
#pragma unroll 1
            for (int i = 0; i < T; i++)
              shift_in(s, sbox(F::add(s[0], load(rc + i * N))));
          } else {
#pragma unroll
            for (int i = 0; i < T; i++)
              s[i] = sbox(F::add(s[i], load(rc + i * N)));
          }
          external(s);
          rc += T * N;
        } else {
          s[0] = sbox(F::add(s[0], load(rc)));
          internal(s, dm1);
          rc += N;
        }
      }
    }

    // the digest of the n elements of rd as 8 canonical words
    template <class RD>
    static ICICLE_HD void hash(const RD& rd, uint64_t n, const Poseidon2WideCtx& c, uint32_t* digest)
    {
      fe s[T];
      uint32_t w[8];
      const uint64_t tagged = c.has_tag;
      const uint64_t off = 1 - tagged, rest = n - off; // without a tag the first element is state[0]; n >= 1 then
      if (tagged) {
        s[0] = load(c.tag);
      } else {
        rd.elem(0, w);
        s[0] = F::from_canonical(w);
      }
#pragma unroll
      for (int i = 1; i < T; i++)
        s[i] = F::zero();
      const uint64_t whole = (rest + T - 2) / (T - 1), blocks = whole ? whole : 1; // fewer than T elements are one permutation
      // one call site of the permutation
#pragma unroll 1
      for (uint64_t b = 0; b < blocks; b++) {
#pragma unroll
        for (int i = 0; i < T - 1; i++) {
          const uint64_t idx = b * (T - 1) + i;
          fe v = F::zero();
          if (idx < rest) {
            rd.elem(off + idx, w);
            v = F::from_canonical(w);
          } else if (idx == rest) { // reached only inside an incomplete last block
            v = F::one();
          }
          s[1 + i] = F::add(s[1 + i], v);
        }
#pragma unroll
        for (int i = 0; i < T; i++)
          s[i] = F::reduce(s[i]);
        permute(s, c);
      }
      F::to_canonical(digest, s[1]);
    }
  };

} // namespace icicle_hip
