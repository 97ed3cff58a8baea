// Poseidon over the 256-bit scalar fields: the permutation and the hash of one message, as one lane computes them. No HIP runtime in
// here, so tests/poseidon_host_harness.cpp compiles the same code with g++ (with -DBIGFIELD_BOUNDS the bound tracker of
// bigfield.hpp runs over every operation below). The kernels over it are poseidon.hip, the parameters poseidon_params.h.
//
// The state of T elements stays in registers: T is a template argument, every state index a compile-time constant. The state is in
// Montgomery form on 29-bit limbs (FieldOps<PR>) from the moment it is loaded until the digest is stored, and so are the tables in
// memory. The optimized schedule (poseidon_params.h) runs as one rolled loop with the full and the partial round behind a branch
// that is uniform over the grid, so that each round body exists once per (field, T):
//   full round     x_i = x_i^5 + c_i for all i, then s <- s A with A = M, or P in the last round in front of the partial ones:
//                  T + 3 products per element
//   partial round  x_0 = x_0^5 + k, then new_0 = sum_i x_i col_i, new_j = x_0 v_j + x_j: 3 + T + (T - 1) products
//   last round     x_i = x_i^5, digest = sum_i x_i M[i][1] -- only state[1] leaves the permutation
// A matrix column times the state is ONE interleaved Montgomery reduction over all its products (dot below, the shared reduction
// of FieldOps::mul_add widened): a column accumulator of 64 bits holds the 9 (K + 1) products below 2^58 of K terms and the
// reduction for K <= 6, so T = 9 and T = 12 take two reductions per output (5 + 4 and 6 + 6 terms) and one addition.
// Bounds (units of p; R / p >= 64): a table entry is < 1, a dot of K terms of bound b is < K b / 64 + 1, x^5 of x < 4 is < 1.1,
// so the state never passes 4: the elements that a partial round only adds to are brought back below 4 p by one conditional
// subtraction per round.
// Every lane reads the same table entry at the same time: the tables are read through a pointer that is the same for every lane,
// entry by entry in the order of the schedule, so they arrive by scalar loads.
// Semantics of the reference's CPU backend (backend/cpu/src/hash/cpu_poseidon.cpp): the state is [tag, x_0 .. x_(T-2)] or
// [x_0 .. x_(T-1)], the digest is state[1]. A message is exactly one permutation's worth.
#pragma once
#include <cstdint>
#include <vector>
#include "bigfield.hpp"
#include "hash_readers.hpp"

namespace icicle_hip {

  constexpr int POSEIDON_LIMBS = 9; // of one table entry

  // what a lane needs beside its message
  struct PoseidonCtx {
    const uint32_t* tab; // Montgomery limbs, 9 per entry: 8 T + r_p round constants in the order of the schedule, M by columns, P by columns,
                         // then per partial round T entries of the first column and T - 1 of the first row
    int r_p;             // 4 full rounds, r_p partial rounds, 4 full rounds
    uint32_t has_tag;    // 0 or 1
    uint32_t tag[POSEIDON_LIMBS]; // Montgomery
  };

  // host: the tables as PoseidonCtx::tab points to them. `rc`, `sparse`: as derived; `mds`, `pre`: row-major as derived, stored by columns
  template <class FE>
  inline std::vector<uint32_t> poseidon_device_tables(int t, const std::vector<FE>& rc, const std::vector<FE>& mds, const std::vector<FE>& pre,
                                                      const std::vector<FE>& sparse)
  {
    std::vector<uint32_t> out;
    out.reserve(POSEIDON_LIMBS * (rc.size() + mds.size() + pre.size() + sparse.size()));
    auto put = [&](const FE& e) { out.insert(out.end(), e.l, e.l + POSEIDON_LIMBS); };
    for (const FE& e : rc)
      put(e);
    for (const std::vector<FE>* m : {&mds, &pre})
      for (int j = 0; j < t; j++)
        for (int i = 0; i < t; i++)
          put((*m)[(size_t)i * t + j]);
    for (const FE& e : sparse)
      put(e);
    return out;
  }

  // element i of a message: 8 little-endian words
  struct PoseidonWords { // 4-aligned
    const uint32_t* p;
    ICICLE_HD void elem(uint64_t i, uint32_t* w) const
    {
#pragma unroll
      for (int k = 0; k < 8; k++)
        w[k] = p[8 * i + k];
    }
  };
  struct PoseidonPadded { // a layer-0 chunk of a tree that reaches into the padding
    ReadPadded rd;
    ICICLE_HD void elem(uint64_t i, uint32_t* w) const
    {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint64_t o = 32 * i + 4 * k;
        w[k] = rd.byte(o) | rd.byte(o + 1) << 8 | rd.byte(o + 2) << 16 | rd.byte(o + 3) << 24;
      }
    }
  };

  template <class PR, int T>
  struct Poseidon {
    using F = FieldOps<PR>;
    using fe = Fe<PR>;
    static constexpr int N = PR::NL;
    static constexpr int HALF_F = 4;
    static_assert(N == POSEIDON_LIMBS && PR::NL32 == 8, "a 256-bit field on nine limbs");
    static_assert(T == 3 || T == 5 || T == 9 || T == 12, "width");
    // terms per reduction: 9 (K + 1) products below 2^58 and a carry below 2^36 in 64 bits
    static constexpr int DOT_MAX = 6;
    static_assert((DOT_MAX + 1) * N < 64, "column accumulator would overflow");

    static ICICLE_HD fe load(const uint32_t* c)
    {
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = c[i];
      BF_SET_BOUND(r, 1);
      return r;
    }

    static ICICLE_HD fe sbox(const fe& x)
    {
      const fe x2 = F::sqr(x);
      return F::mul(F::sqr(x2), x);
    }

    // (sum over q in [LO, HI) of s[q] c[q]) / R mod p (lazy), c: HI - LO .. table entries starting at index LO
    template <int LO, int HI>
    static ICICLE_HD fe dot_part(const fe (&s)[T], const uint32_t* c)
    {
      static_assert(HI - LO >= 1 && HI - LO <= DOT_MAX, "terms per reduction");
      fe r;
#ifdef BIGFIELD_BOUNDS
      double bsum = 0;
      for (int q = LO; q < HI; q++) {
        BF_ASSERT(s[q].bnd <= F::max_bound(), "dot input bound");
        bsum += s[q].bnd;
      }
#endif
      uint32_t m[N];
      uint64_t acc = 0;
#pragma unroll
      for (int k = 0; k < N; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) {
#pragma unroll
          for (int q = LO; q < HI; q++)
            acc += (uint64_t)s[q].l[i] * c[q * N + k - i];
          if (i < k) acc += (uint64_t)m[i] * PR::P[k - i];
        }
        m[k] = ((uint32_t)acc * PR::PINV) & RB_MASK;
        acc += (uint64_t)m[k] * PR::P[0];
        acc >>= RB;
      }
#pragma unroll
      for (int k = N; k < 2 * N - 1; k++) {
#pragma unroll
        for (int i = k - N + 1; i < N; i++) {
#pragma unroll
          for (int q = LO; q < HI; q++)
            acc += (uint64_t)s[q].l[i] * c[q * N + k - i];
          acc += (uint64_t)m[i] * PR::P[k - i];
        }
        r.l[k - N] = (uint32_t)acc & RB_MASK;
        acc >>= RB;
      }
      r.l[N - 1] = (uint32_t)acc;
      BF_SET_BOUND(r, bsum / F::r_over_p() + 1.0);
      return r;
    }
    // sum over all T: one reduction up to six terms, two beyond
    static ICICLE_HD fe dot(const fe (&s)[T], const uint32_t* c)
    {
      if constexpr (T <= DOT_MAX) {
        return dot_part<0, T>(s, c);
      } else {
        constexpr int H = (T + 1) / 2;
        return F::add(dot_part<0, H>(s, c), dot_part<H, T>(s, c));
      }
    }

    // The wide states keep the bodies over all T elements rolled, so that a full round is a few thousand instructions and not
    // T times as many: registers cannot be indexed by a loop counter, so the loop always works at the ends of the array and
    // moves the rest down by one place (9 (T - 1) moves beside at least 3 products of 81 multiply-adds and their reductions).
    static constexpr bool ROLLED = T > 5;
    static ICICLE_HD void shift_in(fe (&a)[T], const fe& x)
    {
#pragma unroll
      for (int i = 0; i + 1 < T; i++)
        a[i] = a[i + 1];
      a[T - 1] = x;
    }

    // x_i <- x_i^5 + c_i
    static ICICLE_HD void sbox_all(fe (&s)[T], const uint32_t* rc)
    {
      if constexpr (ROLLED) {
#pragma unroll 1
        for (int i = 0; i < T; i++)
          shift_in(s, F::add(sbox(s[0]), load(rc + i * N)));
      } else {
#pragma unroll
        for (int i = 0; i < T; i++)
          s[i] = F::add(sbox(s[i]), load(rc + i * N));
      }
    }

    // s <- s A, A by columns at `a`
    static ICICLE_HD void times_matrix(fe (&s)[T], const uint32_t* a)
    {
      fe r[T];
      if constexpr (ROLLED) {
#pragma unroll
        for (int j = 0; j < T; j++)
          r[j] = s[j]; // (every place is written T times below; this one keeps the tracker's records defined)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable) // (left alone the loop is interleaved by two: twice the registers)
        for (int j = 0; j < T; j++)
          shift_in(r, dot(s, a + j * T * N));
      } else {
        columns<0>(r, s, a);
      }
#pragma unroll
      for (int j = 0; j < T; j++)
        s[j] = r[j];
    }
    // r[J ..] = s A[.. , J ..]: unrolled by recursion -- a loop of T dots is past the size up to which the compiler honours an
    // unroll pragma at T = 5, and left rolled it would index r in scratch
    template <int J>
    static ICICLE_HD void columns(fe (&r)[T], const fe (&s)[T], const uint32_t* a)
    {
      r[J] = dot(s, a + J * T * N);
      if constexpr (J + 1 < T) columns<J + 1>(r, s, a);
    }

    // the digest in Montgomery form
    static ICICLE_HD fe permute(fe (&s)[T], const PoseidonCtx& c)
    {
      const uint32_t* rc = c.tab;
      const uint32_t* mds = c.tab + (size_t)N * (2 * HALF_F * T + c.r_p);
      const uint32_t* pre = mds + N * T * T;
      const uint32_t* sparse = pre + N * T * T;
#pragma unroll
      for (int i = 0; i < T; i++)
        s[i] = F::add(s[i], load(rc + i * N));
      rc += T * N;
      const int rounds = 2 * HALF_F + c.r_p - 1;
#pragma unroll 1
      for (int r = 0; r < rounds; r++) {
        if (r < HALF_F || r >= HALF_F + c.r_p) {
          sbox_all(s, rc);
          times_matrix(s, r == HALF_F - 1 ? pre : mds);
          rc += T * N;
        } else {
          s[0] = F::add(sbox(s[0]), load(rc));
          const fe first = dot(s, sparse);
#pragma unroll
          for (int j = 1; j < T; j++) {
            s[j] = F::add(s[j], F::mul(s[0], load(sparse + (T + j - 1) * N)));
            F::template cond_sub<4>(s[j]);
          }
          s[0] = first;
          rc += N, sparse += (2 * T - 1) * N;
        }
      }
      if constexpr (ROLLED) {
#pragma unroll 1
        for (int i = 0; i < T; i++)
          shift_in(s, sbox(s[0]));
      } else {
#pragma unroll
        for (int i = 0; i < T; i++)
          s[i] = sbox(s[i]);
      }
      return dot(s, mds + T * N); // column 1
    }

    // the digest of the message of rd as 8 canonical words
    template <class RD>
    static ICICLE_HD void hash(const RD& rd, const PoseidonCtx& c, uint32_t* digest)
    {
      fe s[T];
      const int tagged = (int)c.has_tag;
#pragma unroll
      for (int i = 0; i < T; i++) {
        if (i == 0 && tagged) {
          s[0] = load(c.tag);
        } else {
          uint32_t w[8];
          rd.elem((uint64_t)(i - tagged), w);
          s[i] = F::from_canonical(w);
        }
      }
      F::to_canonical(digest, permute(s, c));
    }
  };

} // namespace icicle_hip
