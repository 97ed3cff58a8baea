// Big prime-field arithmetic for gfx950, written around the one cheap wide integer op CDNA4 has:
// v_mad_u64_u32 (32x32+64 -> 64, ~1.25x the cost of a plain VALU op, measured in
// profiles/r01_alu_ubench.txt). There is NO carry-in on that instruction and carry chains through
// VCC cost a second VALU op per product, so instead of the reference's 32-bit limbs + carry chain
// (icicle/include/icicle/math/host_math.h:227-281, Barrett 438-470) elements are held in
// radix-2^29 limbs: a column of up to 2*NL 58-bit products accumulates in ONE 64-bit register pair
// with no carry handling at all, and Montgomery reduction (R = 2^(29*NL)) is interleaved in the
// same accumulator (product scanning / FIPS).
//
// Value discipline ("lazy reduction"): R/p >= 64 for every field here, so a Montgomery product of
// inputs < Ka*p, Kb*p is < (Ka*Kb/(R/p) + 1)*p. Nothing on the hot path is ever conditionally
// reduced; subtraction adds a multiple of p (K*p, K in {2,4,8,16}) big enough to stay positive.
// A normalised element has limbs 0..NL-2 in [0,2^29) and a non-negative top limb.
// In host debug builds (-DBIGFIELD_BOUNDS) every element carries its bound (in units of p) and each
// op asserts its precondition, so the bounds argument of ec.hpp is machine-checked by tests.
//
// I/O is the reference's canonical storage<N> (N x u32 little-endian, value in [0,p), NOT
// Montgomery unless a *_montgomery_form flag says so; modular_arithmetic.h:517-521, 583-585).
#pragma once
#include <cstdint>
#include "field_consts.h"
#include "mont_asm.hpp" // device builds: the products below as single inline-asm blocks (-DBIGFIELD_NO_ASM turns them off)

#if defined(__HIPCC__)
  #include <hip/hip_runtime.h>
  #define HD __host__ __device__ __forceinline__
#else
  #define HD inline __attribute__((always_inline))
#endif

#ifdef BIGFIELD_BOUNDS
  #include <cassert>
  #include <cstdio>
  // bnd: the unsigned operations' value bound. The signed layer's record (sg set; see "signed layer" below): value in
  // [slo, shi] units of p, limbs 0..N-2 in [llo, lhi], top limb in [tlo, thi]. An element of the signed layer has bnd = 1e300,
  // so every unsigned operation that is handed one trips its own precondition.
  #define BF_BOUND_DECL                                                                                                \
    double bnd = 0;                                                                                                    \
    bool sg = false;                                                                                                   \
    double slo = 0, shi = 0, llo = 0, lhi = 0, tlo = 0, thi = 0;
  #define BF_SET_BOUND(x, v) ((x).bnd = (v), (x).sg = false)
  #define BF_ASSERT(cond, msg)                                                                                         \
    do {                                                                                                               \
      if (!(cond)) {                                                                                                   \
        fprintf(stderr, "bigfield bound violation: %s (%s:%d)\n", msg, __FILE__, __LINE__);                            \
        assert(false);                                                                                                 \
      }                                                                                                                \
    } while (0)
#else
  #define BF_BOUND_DECL
  #define BF_SET_BOUND(x, v)
  #define BF_ASSERT(cond, msg)
#endif

namespace icicle_hip {

  template <class PR>
  struct Fe {
    uint32_t l[PR::NL];
    BF_BOUND_DECL
  };

  template <class PR>
  struct FieldOps {
    static constexpr int N = PR::NL;
    static constexpr int N32 = PR::NL32;
    static constexpr uint32_t MASK = RB_MASK;
    static constexpr bool TIGHT = false; // see fq2.hpp
    using fe = Fe<PR>;
    // R/p (lower bound) used only by the debug bound tracker
    static constexpr double r_over_p() { return (double)(1ull << (RB * N - PR::NBITS)); }
    // largest bound (units of p) a stored element may have: value < 2^(RB*N) and mul inputs sane
    static constexpr double max_bound() { return r_over_p() < 64.0 ? r_over_p() : 64.0; }

    static HD fe zero()
    {
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = 0;
      BF_SET_BOUND(r, 0);
      return r;
    }
    static HD fe one()
    { // Montgomery one
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = PR::ONE[i];
      BF_SET_BOUND(r, 1);
      return r;
    }
    // R^2 mod p as limbs: mul(x_plain, r2()) = x*R (into Montgomery form); also "1" in the doubly-scaled form x*R^2
    static HD fe r2()
    {
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = PR::R2[i];
      BF_SET_BOUND(r, 1);
      return r;
    }
    // the plain integer 1: mul(x, plain_one()) = x/R (one Montgomery scaling removed)
    static HD fe plain_one()
    {
      fe r = zero();
      r.l[0] = 1;
      BF_SET_BOUND(r, 1);
      return r;
    }
    using bfe = fe;
    static HD bfe base_r2() { return r2(); }
    static HD bfe base_plain_one() { return plain_one(); }
    static HD fe mul_base(const fe& a, const bfe& s) { return mul(a, s); }
    // constant given as [N] Montgomery limbs (< p)
    template <class ARR>
    static HD fe from_const(const ARR& c)
    {
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = c[i];
      BF_SET_BOUND(r, 1);
      return r;
    }
    template <int K>
    static HD uint32_t kp(int i)
    {
      static_assert(K == 1 || K == 2 || K == 4 || K == 8 || K == 16, "K");
      if constexpr (K == 1) return PR::P[i];
      if constexpr (K == 2) return PR::P2[i];
      if constexpr (K == 4) return PR::P4[i];
      if constexpr (K == 8) return PR::P8[i];
      return PR::P16[i];
    }

    // ---- Montgomery multiplication: r = a*b/R mod p (lazy), product scanning ----
    // Column k accumulates sum_{i+j=k} a_i*b_j + m_i*p_j in one 64-bit register: <= 2N products of
    // < 2^58 plus a < 2^35 carry; 2N*2^58 < 2^64 for N <= 31.
    static HD fe mul(const fe& a, const fe& b)
    {
      BF_ASSERT(a.bnd <= max_bound() && b.bnd <= max_bound(), "mul input bound");
      fe r;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BIGFIELD_NO_ASM)
      if constexpr (N == 9) {
        mont_mul_asm9<PR>(r.l, a.l, b.l);
        return r;
      } else if constexpr (N == 14) {
        mont_mul_asm14<PR>(r.l, a.l, b.l);
        return r;
      }
#endif
      uint32_t m[N];
      uint64_t acc = 0;
#pragma unroll
      for (int k = 0; k < N; k++) {
#pragma unroll
        for (int i = 0; i < k; i++) {
          acc += (uint64_t)a.l[i] * b.l[k - i];
          acc += (uint64_t)m[i] * PR::P[k - i];
        }
        acc += (uint64_t)a.l[k] * b.l[0];
        m[k] = ((uint32_t)acc * PR::PINV) & MASK;
        acc += (uint64_t)m[k] * PR::P[0];
        acc >>= RB;
      }
#pragma unroll
      for (int k = N; k < 2 * N - 1; k++) {
#pragma unroll
        for (int i = k - N + 1; i < N; i++) {
          acc += (uint64_t)a.l[i] * b.l[k - i];
          acc += (uint64_t)m[i] * PR::P[k - i];
        }
        r.l[k - N] = (uint32_t)acc & MASK;
        acc >>= RB;
      }
      r.l[N - 1] = (uint32_t)acc;
      BF_SET_BOUND(r, a.bnd * b.bnd / r_over_p() + 1.0);
      return r;
    }

    // a <- a*b/R (same value and bound as mul). On the device the result is produced in a's own registers, so a
    // loop-carried accumulator coordinate needs no copies at the back edge (mont_asm.hpp).
    static HD void mul_inplace(fe& a, const fe& b)
    {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BIGFIELD_NO_ASM)
      if constexpr (N == 9) {
        mont_mul_inplace_asm9<PR>(a.l, b.l);
        return;
      } else if constexpr (N == 14) {
        mont_mul_inplace_asm14<PR>(a.l, b.l);
        return;
      }
#endif
      a = mul(a, b);
    }

    // r = (a*b + c*d)/R mod p with ONE interleaved reduction: both products share the column
    // accumulators (3N products of < 2^58 per column: < 2^64 for N <= 21).
    static HD fe mul_add(const fe& a, const fe& b, const fe& c, const fe& d)
    {
      BF_ASSERT(a.bnd <= max_bound() && b.bnd <= max_bound() && c.bnd <= max_bound() && d.bnd <= max_bound(), "mul_add input bound");
      static_assert(N <= 21, "column accumulator would overflow");
      fe r;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BIGFIELD_NO_ASM)
      if constexpr (N == 9) {
        mont_mul_add_asm9<PR>(r.l, a.l, b.l, c.l, d.l);
        return r;
      } else if constexpr (N == 14) {
        mont_mul_add_asm14<PR>(r.l, a.l, b.l, c.l, d.l);
        return r;
      }
#endif
      uint32_t m[N];
      uint64_t acc = 0;
#pragma unroll
      for (int k = 0; k < N; k++) {
#pragma unroll
        for (int i = 0; i < k; i++) {
          acc += (uint64_t)a.l[i] * b.l[k - i];
          acc += (uint64_t)c.l[i] * d.l[k - i];
          acc += (uint64_t)m[i] * PR::P[k - i];
        }
        acc += (uint64_t)a.l[k] * b.l[0];
        acc += (uint64_t)c.l[k] * d.l[0];
        m[k] = ((uint32_t)acc * PR::PINV) & MASK;
        acc += (uint64_t)m[k] * PR::P[0];
        acc >>= RB;
      }
#pragma unroll
      for (int k = N; k < 2 * N - 1; k++) {
#pragma unroll
        for (int i = k - N + 1; i < N; i++) {
          acc += (uint64_t)a.l[i] * b.l[k - i];
          acc += (uint64_t)c.l[i] * d.l[k - i];
          acc += (uint64_t)m[i] * PR::P[k - i];
        }
        r.l[k - N] = (uint32_t)acc & MASK;
        acc >>= RB;
      }
      r.l[N - 1] = (uint32_t)acc;
      BF_SET_BOUND(r, (a.bnd * b.bnd + c.bnd * d.bnd) / r_over_p() + 1.0);
      return r;
    }

    // c <- (a*b + c*d)/R, result in c's own registers on the device (see mul_inplace)
    static HD void mul_add_inplace_c(fe& c, const fe& a, const fe& b, const fe& d)
    {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BIGFIELD_NO_ASM)
      if constexpr (N == 9) {
        mont_mul_add_inplace_c_asm9<PR>(c.l, a.l, b.l, d.l);
        return;
      } else if constexpr (N == 14) {
        mont_mul_add_inplace_c_asm14<PR>(c.l, a.l, b.l, d.l);
        return;
      }
#endif
      c = mul_add(a, b, c, d);
    }

    // Squaring: the a_i*a_j cross terms are computed once and doubled (N(N+1)/2 instead of N^2
    // products for the a*a half; the m*p half is unchanged).
    static HD fe sqr(const fe& a)
    {
      BF_ASSERT(a.bnd <= max_bound(), "sqr input bound");
      fe r;
      uint32_t m[N];
      uint32_t a2[N]; // 2*a_i (< 2^30)
#pragma unroll
      for (int i = 0; i < N; i++)
        a2[i] = a.l[i] << 1;
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BIGFIELD_NO_ASM)
      if constexpr (N == 9) {
        mont_sqr_asm9<PR>(r.l, a.l, a2);
        return r;
      } else if constexpr (N == 14) {
        mont_sqr_asm14<PR>(r.l, a.l, a2);
        return r;
      }
#endif
      uint64_t acc = 0;
#pragma unroll
      for (int k = 0; k < 2 * N - 1; k++) {
        // a*a part of column k: pairs (i, k-i) with i < k-i use the doubled limb, plus the square
        const int lo = (k < N) ? 0 : k - N + 1;
        const int hi = (k < N) ? k : N - 1;
#pragma unroll
        for (int i = lo; i <= hi; i++) {
          const int j = k - i;
          if (i < j) acc += (uint64_t)a2[i] * a.l[j];
          if (i == j) acc += (uint64_t)a.l[i] * a.l[i];
        }
        if (k < N) {
#pragma unroll
          for (int i = 0; i < k; i++)
            acc += (uint64_t)m[i] * PR::P[k - i];
          m[k] = ((uint32_t)acc * PR::PINV) & MASK;
          acc += (uint64_t)m[k] * PR::P[0];
        } else {
#pragma unroll
          for (int i = k - N + 1; i < N; i++)
            acc += (uint64_t)m[i] * PR::P[k - i];
          r.l[k - N] = (uint32_t)acc & MASK;
        }
        acc >>= RB;
      }
      r.l[N - 1] = (uint32_t)acc;
      BF_SET_BOUND(r, a.bnd * a.bnd / r_over_p() + 1.0);
      return r;
    }

    // ---- add / sub with carry normalisation ----
    static HD fe add(const fe& a, const fe& b)
    {
      fe r;
      uint32_t c = 0;
#pragma unroll
      for (int i = 0; i < N - 1; i++) {
        uint32_t t = a.l[i] + b.l[i] + c;
        r.l[i] = t & MASK;
        c = t >> RB;
      }
      r.l[N - 1] = a.l[N - 1] + b.l[N - 1] + c;
      BF_SET_BOUND(r, a.bnd + b.bnd);
      BF_ASSERT(r.bnd <= max_bound(), "add result bound");
      return r;
    }
    static HD fe dbl(const fe& a) { return add(a, a); }

    // r = a - b + K*p ; requires b < K*p (so the value stays non-negative)
    template <int K>
    static HD fe sub(const fe& a, const fe& b)
    {
      BF_ASSERT(b.bnd <= (double)K, "sub: subtrahend exceeds K*p");
      fe r;
      int32_t c = 0;
#pragma unroll
      for (int i = 0; i < N - 1; i++) {
        int32_t t = (int32_t)(a.l[i] - b.l[i] + kp<K>(i)) + c;
        r.l[i] = (uint32_t)t & MASK;
        c = t >> RB; // arithmetic
      }
      r.l[N - 1] = a.l[N - 1] - b.l[N - 1] + kp<K>(N - 1) + (uint32_t)c;
      BF_SET_BOUND(r, a.bnd + (double)K);
      BF_ASSERT(r.bnd <= max_bound(), "sub result bound");
      return r;
    }
    template <int K>
    static HD fe neg(const fe& a)
    {
      return sub<K>(zero(), a);
    }

    // r = cond ? a : b (branch-free select)
    static HD fe select(bool cond, const fe& a, const fe& b)
    {
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = cond ? a.l[i] : b.l[i];
#ifdef BIGFIELD_BOUNDS
      r.bnd = a.bnd > b.bnd ? a.bnd : b.bnd;
#endif
      return r;
    }

    // ---- signed layer: the same radix, SIGNED limbs, no carry chains ------------------------------------------------------
    // The operations above keep every limb in [0, 2^29): a subtraction adds K*p to stay non-negative and every add / sub walks a
    // serial carry chain (3-4 instructions per limb). Nothing downstream needs that: v_mad_i64_i32 issues at the rate of
    // v_mad_u64_u32 (profiles/r02_alu_ubench.txt), so a product can take signed limbs into a signed column accumulator, and
    // then every linear step is ONE instruction per limb with no carry and no K*p. An element of this layer is the integer
    // sum_i (int32)l[i] * 2^(29 i), which may be negative; the limbs stay in uint32_t storage and are reinterpreted (two's
    // complement), so nothing here is undefined behaviour.
    //   sadd / ssub / sneg / sadd2 (2a + b) / scneg   limb-wise, no carry: limb ranges add up
    //   snormalise                                    one signed carry pass: limbs 0..N-2 back in [0, 2^29), signed top limb
    //   smul_small<K>                                 K a for a small constant K with the carry pass folded in: normalised
    //   smul / ssqr / smul_add / *_inplace            Montgomery products of signed operands: (a b + m p) / R with 0 <= m < R, so a
    //                                                 result lies in (a b / R, a b / R + p) and comes out normalised (signed top)
    //   to_unsigned<K>                                a + K p, carry-normalised: back to the operations above (cold paths)
    // What bounds the limbs is the column accumulator: |sum of products| + m p + carry must stay below 2^63, and a limb-wise
    // result must fit an int32. Under -DBIGFIELD_BOUNDS every element of this layer carries a two-sided value bound (units of
    // p), the range of its limbs 0..N-2 and the range of its top limb; every product asserts its columns one by one, every
    // linear operation asserts the int32 range. (Ranges, not magnitudes: the difference of two normalised elements has limbs
    // in (-2^29, 2^29), not below 2^30 -- ec.hpp's madd needs exactly that.) An element of the unsigned operations is a valid
    // operand here (limbs in [0, 2^29), value in [0, bnd p]); the reverse needs to_unsigned.
#ifdef BIGFIELD_BOUNDS
    struct SB {
      double lo, hi;   // value, units of p
      double llo, lhi; // limbs 0..N-2
      double tlo, thi; // limb N-1
    };
    static constexpr double I32_LIM = 2147483647.0;
    // top limb of a NORMALISED element (limbs 0..N-2 in [0, 2^29)) of value v in [lo, hi] p: floor(v / 2^(29 (N-1))), and
    // p < (P[N-1] + 1) 2^(29 (N-1)); one unit of slack for the rounding of the doubles
    static void top_range(double lo, double hi, double& tlo, double& thi)
    {
      const double pt = (double)PR::P[N - 1] + 1.0;
      tlo = lo < 0 ? __builtin_floor(lo * pt) - 1.0 : 0.0;
      thi = hi > 0 ? __builtin_ceil(hi * pt) + 1.0 : 0.0;
    }
    static SB normalised(double lo, double hi)
    {
      SB s;
      s.lo = lo, s.hi = hi, s.llo = 0, s.lhi = (double)MASK;
      top_range(lo, hi, s.tlo, s.thi);
      return s;
    }
    static SB sview(const fe& a)
    {
      if (!a.sg) return normalised(0, a.bnd);
      SB s;
      s.lo = a.slo, s.hi = a.shi, s.llo = a.llo, s.lhi = a.lhi, s.tlo = a.tlo, s.thi = a.thi;
      return s;
    }
    static void sset(fe& r, const SB& s)
    {
      BF_ASSERT(s.llo >= -I32_LIM && s.lhi <= I32_LIM && s.tlo >= -I32_LIM && s.thi <= I32_LIM, "signed layer: a limb can leave int32");
      r.sg = true, r.bnd = 1e300;
      r.slo = s.lo, r.shi = s.hi, r.llo = s.llo, r.lhi = s.lhi, r.tlo = s.tlo, r.thi = s.thi;
    }
    static double smag(const SB& s, int i)
    {
      const double lo = i == N - 1 ? s.tlo : s.llo, hi = i == N - 1 ? s.thi : s.lhi;
      return -lo > hi ? -lo : hi;
    }
    // worst case of every column of the product scanning: sum |x_i| |y_j| over the operand pairs + sum m_i p_j + carry < 2^63
    static void scolumns(const SB* x, const SB* y, int npairs)
    {
      unsigned __int128 carry = 0;
      for (int k = 0; k < 2 * N - 1; k++) {
        unsigned __int128 col = carry;
        const int lo = k < N ? 0 : k - N + 1, hi = k < N ? k : N - 1;
        for (int i = lo; i <= hi; i++) {
          for (int q = 0; q < npairs; q++)
            col += (unsigned __int128)(uint64_t)smag(x[q], i) * (uint64_t)smag(y[q], k - i);
          col += (unsigned __int128)MASK * PR::P[k - i];
        }
        BF_ASSERT(col < ((unsigned __int128)1 << 63), "signed product: a column accumulator can leave int64");
        carry = (col >> RB) + 1;
      }
    }
    static void prod_range(const SB& a, const SB& b, double& lo, double& hi)
    {
      const double v[4] = {a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi};
      lo = hi = v[0];
      for (int i = 1; i < 4; i++) {
        lo = v[i] < lo ? v[i] : lo;
        hi = v[i] > hi ? v[i] : hi;
      }
    }
    static void sset_mul(fe& r, const fe& a, const fe& b)
    {
      const SB x = sview(a), y = sview(b);
      scolumns(&x, &y, 1);
      double lo, hi;
      prod_range(x, y, lo, hi);
      sset(r, normalised(lo / r_over_p(), hi / r_over_p() + 1.0));
    }
    static void sset_mul_add(fe& r, const fe& a, const fe& b, const fe& c, const fe& d)
    {
      const SB x[2] = {sview(a), sview(c)}, y[2] = {sview(b), sview(d)};
      scolumns(x, y, 2);
      double lo0, hi0, lo1, hi1;
      prod_range(x[0], y[0], lo0, hi0);
      prod_range(x[1], y[1], lo1, hi1);
      sset(r, normalised((lo0 + lo1) / r_over_p(), (hi0 + hi1) / r_over_p() + 1.0));
    }
    // test hooks: claim a record for an element built by hand (as BF_SET_BOUND does for the unsigned operations)
    static void sclaim(fe& a, double lo, double hi, double llo, double lhi, double tlo, double thi)
    {
      SB s;
      s.lo = lo, s.hi = hi, s.llo = llo, s.lhi = lhi, s.tlo = tlo, s.thi = thi;
      sset(a, s);
    }
#endif
    // Tracker only: assert that a's value lies in [lo, hi] p and that it is normalised, then WIDEN its record to exactly that. A loop
    // that does this to its carried state at the top of every step proves "invariant in => invariant out" in one step,
    // whatever the history (ec.hpp madd).
    static HD void sassume_normalised(fe& a, double lo, double hi)
    {
#ifdef BIGFIELD_BOUNDS
      const SB s = sview(a);
      BF_ASSERT(s.lo >= lo && s.hi <= hi, "signed layer: value outside the stated invariant");
      BF_ASSERT(s.llo >= 0 && s.lhi <= (double)MASK, "signed layer: operand must be normalised");
      sset(a, normalised(lo, hi));
#else
      (void)a, (void)lo, (void)hi;
#endif
    }
    // Tracker only: a's limbs 0..N-2 lie in (-2^29, 2^29) and its value in [lo, hi] p (a gathered operand, negated limb-wise or not)
    static HD void sassert_operand(const fe& a, double lo, double hi)
    {
#ifdef BIGFIELD_BOUNDS
      const SB s = sview(a);
      BF_ASSERT(s.lo >= lo && s.hi <= hi, "signed layer: operand value outside the stated range");
      BF_ASSERT(s.llo >= -(double)MASK && s.lhi <= (double)MASK, "signed layer: operand limb outside (-2^29, 2^29)");
#else
      (void)a, (void)lo, (void)hi;
#endif
    }

    static HD fe sadd(const fe& a, const fe& b)
    {
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = a.l[i] + b.l[i];
#ifdef BIGFIELD_BOUNDS
      const SB x = sview(a), y = sview(b);
      sset(r, SB{x.lo + y.lo, x.hi + y.hi, x.llo + y.llo, x.lhi + y.lhi, x.tlo + y.tlo, x.thi + y.thi});
#endif
      return r;
    }
    static HD fe ssub(const fe& a, const fe& b)
    {
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = a.l[i] - b.l[i];
#ifdef BIGFIELD_BOUNDS
      const SB x = sview(a), y = sview(b);
      sset(r, SB{x.lo - y.hi, x.hi - y.lo, x.llo - y.lhi, x.lhi - y.llo, x.tlo - y.thi, x.thi - y.tlo});
#endif
      return r;
    }
    static HD fe sneg(const fe& a)
    {
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = 0u - a.l[i];
#ifdef BIGFIELD_BOUNDS
      const SB x = sview(a);
      sset(r, SB{-x.hi, -x.lo, -x.lhi, -x.llo, -x.thi, -x.tlo});
#endif
      return r;
    }
    // 2a + b (one v_lshl_add_u32 per limb)
    static HD fe sadd2(const fe& a, const fe& b)
    {
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = (a.l[i] << 1) + b.l[i];
#ifdef BIGFIELD_BOUNDS
      const SB x = sview(a), y = sview(b);
      sset(r, SB{2 * x.lo + y.lo, 2 * x.hi + y.hi, 2 * x.llo + y.llo, 2 * x.lhi + y.lhi, 2 * x.tlo + y.tlo, 2 * x.thi + y.thi});
#endif
      return r;
    }
    // negate ? -a : a, limb-wise: (l ^ s) + (s & 1) with s = 0 or ~0 (one v_xad_u32 per limb)
    static HD fe scneg(const fe& a, bool negate)
    {
      fe r;
      const uint32_t s = negate ? 0xffffffffu : 0u, o = negate ? 1u : 0u;
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = (a.l[i] ^ s) + o;
#ifdef BIGFIELD_BOUNDS
      const SB x = sview(a);
      auto mn = [](double u, double v) { return u < v ? u : v; };
      auto mx = [](double u, double v) { return u > v ? u : v; };
      sset(r, SB{mn(x.lo, -x.hi), mx(x.hi, -x.lo), mn(x.llo, -x.lhi), mx(x.lhi, -x.llo), mn(x.tlo, -x.thi), mx(x.thi, -x.tlo)});
#endif
      return r;
    }
    // one signed carry pass: same value, limbs 0..N-2 in [0, 2^29), signed top limb
    static HD fe snormalise(const fe& a)
    {
      fe r;
      int32_t c = 0;
#pragma unroll
      for (int i = 0; i < N - 1; i++) {
        const int32_t t = (int32_t)a.l[i] + c;
        r.l[i] = (uint32_t)t & MASK;
        c = t >> RB; // arithmetic
      }
      r.l[N - 1] = a.l[N - 1] + (uint32_t)c;
#ifdef BIGFIELD_BOUNDS
      const SB x = sview(a);
      double clo = 0, chi = 0;
      for (int i = 0; i < N - 1; i++) {
        BF_ASSERT(x.llo + clo >= -I32_LIM && x.lhi + chi <= I32_LIM, "snormalise: limb + carry can leave int32");
        clo = __builtin_floor((x.llo + clo) / (double)(1u << RB));
        chi = __builtin_floor((x.lhi + chi) / (double)(1u << RB));
      }
      BF_ASSERT(x.tlo + clo >= -I32_LIM && x.thi + chi <= I32_LIM, "snormalise: top limb + carry can leave int32");
      sset(r, normalised(x.lo, x.hi));
#endif
      return r;
    }
    // K a for a small integer constant K (3 b of a curve whose b is small, 3 X1 X2), normalised. K times a limb need not fit an
    // int32 (9 * 2^29 does not), so the product and the carry pass are one 64-bit multiply-add per limb: any int32 limb goes in.
    template <int K>
    static HD fe smul_small(const fe& a)
    {
      static_assert(K != 0 && K >= -64 && K <= 64, "a small constant");
      fe r;
      int64_t c = 0;
#pragma unroll
      for (int i = 0; i < N - 1; i++) {
        const int64_t t = (int64_t)(int32_t)a.l[i] * K + c;
        r.l[i] = (uint32_t)t & MASK;
        c = t >> RB; // arithmetic
      }
      r.l[N - 1] = (uint32_t)((int64_t)(int32_t)a.l[N - 1] * K + c);
#ifdef BIGFIELD_BOUNDS
      const SB x = sview(a);
      const double k = (double)K;
      double clo = 0, chi = 0; // (|K| * 2^31 + carry is far inside an int64 and exact in a double)
      for (int i = 0; i < N - 1; i++) {
        clo = __builtin_floor(((K > 0 ? x.llo : x.lhi) * k + clo) / (double)(1u << RB));
        chi = __builtin_floor(((K > 0 ? x.lhi : x.llo) * k + chi) / (double)(1u << RB));
      }
      BF_ASSERT((K > 0 ? x.tlo : x.thi) * k + clo >= -I32_LIM && (K > 0 ? x.thi : x.tlo) * k + chi <= I32_LIM, "smul_small: top limb can leave int32");
      sset(r, normalised(K > 0 ? k * x.lo : k * x.hi, K > 0 ? k * x.hi : k * x.lo));
#endif
      return r;
    }
    // a + K*p with the carry chain of sub<K>: requires a >= -K*p; the result is an element of the unsigned operations
    template <int K>
    static HD fe to_unsigned(const fe& a)
    {
      fe r;
      int32_t c = 0;
#pragma unroll
      for (int i = 0; i < N - 1; i++) {
        const int32_t t = (int32_t)(a.l[i] + kp<K>(i)) + c;
        r.l[i] = (uint32_t)t & MASK;
        c = t >> RB; // arithmetic
      }
      r.l[N - 1] = a.l[N - 1] + kp<K>(N - 1) + (uint32_t)c;
#ifdef BIGFIELD_BOUNDS
      const SB x = sview(a);
      BF_ASSERT(x.lo >= -(double)K, "to_unsigned: value can be below -K*p");
      BF_ASSERT(smag(x, 0) + (double)(1u << RB) + 8.0 <= I32_LIM && smag(x, N - 1) + (double)kp<K>(N - 1) + 8.0 <= I32_LIM, "to_unsigned: limb + K*p + carry can leave int32");
      BF_SET_BOUND(r, x.hi + (double)K);
      BF_ASSERT(r.bnd <= max_bound(), "to_unsigned result bound");
#endif
      return r;
    }

    // (a*b [+ c*d] + m*p) / R over signed limbs, int64_t column accumulators: the host's and -DBIGFIELD_NO_ASM's form of the products
    template <bool TWO>
    static HD void sprod_generic(fe& r, const fe& a, const fe& b, const fe& c, const fe& d)
    {
      uint32_t m[N], o[N];
      int64_t acc = 0;
      auto term = [](uint32_t x, uint32_t y) { return (int64_t)(int32_t)x * (int64_t)(int32_t)y; };
#pragma unroll
      for (int k = 0; k < N; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) {
          acc += term(a.l[i], b.l[k - i]);
          if constexpr (TWO) acc += term(c.l[i], d.l[k - i]);
          if (i < k) acc += (int64_t)m[i] * (int64_t)PR::P[k - i];
        }
        m[k] = ((uint32_t)acc * PR::PINV) & MASK;
        acc += (int64_t)m[k] * (int64_t)PR::P[0];
        acc >>= RB; // arithmetic, exact: the low 29 bits are zero
      }
#pragma unroll
      for (int k = N; k < 2 * N - 1; k++) {
#pragma unroll
        for (int i = k - N + 1; i < N; i++) {
          acc += term(a.l[i], b.l[k - i]);
          if constexpr (TWO) acc += term(c.l[i], d.l[k - i]);
          acc += (int64_t)m[i] * (int64_t)PR::P[k - i];
        }
        o[k - N] = (uint32_t)acc & MASK;
        acc >>= RB;
      }
      o[N - 1] = (uint32_t)acc; // the arithmetic remainder: signed top limb
#pragma unroll
      for (int i = 0; i < N; i++)
        r.l[i] = o[i]; // (r may be one of the operands)
    }
    static HD fe smul(const fe& a, const fe& b)
    {
      fe r;
#ifdef BIGFIELD_BOUNDS
      sset_mul(r, a, b);
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BIGFIELD_NO_ASM)
      if constexpr (N == 9) {
        mont_smul_asm9<PR>(r.l, a.l, b.l);
        return r;
      }
#endif
      sprod_generic<false>(r, a, b, a, b);
      return r;
    }
    static HD void smul_inplace(fe& a, const fe& b)
    {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BIGFIELD_NO_ASM)
      if constexpr (N == 9) {
        mont_smul_inplace_asm9<PR>(a.l, b.l);
        return;
      }
#endif
      a = smul(a, b);
    }
    static HD fe ssqr(const fe& a)
    {
      fe r;
#ifdef BIGFIELD_BOUNDS
      { // the asm form multiplies by a2 = 2a: those limbs must fit an int32 too; a square is never negative
        const SB x = sview(a);
        BF_ASSERT(2 * smag(x, 0) <= I32_LIM && 2 * smag(x, N - 1) <= I32_LIM, "ssqr: a doubled limb can leave int32");
        scolumns(&x, &x, 1);
        const double l2 = x.lo * x.lo, h2 = x.hi * x.hi;
        sset(r, normalised((x.lo <= 0 && x.hi >= 0) ? 0.0 : (l2 < h2 ? l2 : h2) / r_over_p(), (l2 > h2 ? l2 : h2) / r_over_p() + 1.0));
      }
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BIGFIELD_NO_ASM)
      if constexpr (N == 9) {
        uint32_t a2[N];
#pragma unroll
        for (int i = 0; i < N; i++)
          a2[i] = a.l[i] << 1;
        mont_ssqr_asm9<PR>(r.l, a.l, a2);
        return r;
      }
#endif
      sprod_generic<false>(r, a, a, a, a);
      return r;
    }
    static HD fe smul_add(const fe& a, const fe& b, const fe& c, const fe& d)
    {
      fe r;
#ifdef BIGFIELD_BOUNDS
      sset_mul_add(r, a, b, c, d);
#endif
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BIGFIELD_NO_ASM)
      if constexpr (N == 9) {
        mont_smul_add_asm9<PR>(r.l, a.l, b.l, c.l, d.l);
        return r;
      }
#endif
      sprod_generic<true>(r, a, b, c, d);
      return r;
    }
    // c <- (a*b + c*d)/R in c's own registers (see mul_add_inplace_c)
    static HD void smul_add_inplace_c(fe& c, const fe& a, const fe& b, const fe& d)
    {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(BIGFIELD_NO_ASM)
      if constexpr (N == 9) {
        mont_smul_add_inplace_c_asm9<PR>(c.l, a.l, b.l, d.l);
        return;
      }
#endif
      c = smul_add(a, b, c, d);
    }

    // ---- full reduction to [0,p) (output path only) ----
    // one conditional subtraction of K*p
    template <int K>
    static HD void cond_sub(fe& a)
    {
      uint32_t t[N];
      int32_t c = 0;
#pragma unroll
      for (int i = 0; i < N - 1; i++) {
        int32_t d = (int32_t)(a.l[i] - kp<K>(i)) + c;
        t[i] = (uint32_t)d & MASK;
        c = d >> RB;
      }
      int32_t top = (int32_t)(a.l[N - 1] - kp<K>(N - 1)) + c;
      const bool ge = top >= 0;
#pragma unroll
      for (int i = 0; i < N - 1; i++)
        a.l[i] = ge ? t[i] : a.l[i];
      a.l[N - 1] = ge ? (uint32_t)top : a.l[N - 1];
#ifdef BIGFIELD_BOUNDS
      a.bnd = (a.bnd - (double)K > (double)K) ? a.bnd - (double)K : (a.bnd < (double)K ? a.bnd : (double)K);
#endif
    }
    // value < 16p -> < 4p (two conditional subtractions); used by ec.hpp in Fq2Ops' TIGHT mode only
    static HD fe below4(const fe& a)
    {
      BF_ASSERT(a.bnd <= 16.0, "below4 input bound");
      fe r = a;
      cond_sub<8>(r);
      cond_sub<4>(r);
      return r;
    }
    static HD fe reduce(const fe& a)
    { // value < 32p  ->  [0,p)
      BF_ASSERT(a.bnd <= 32.0, "reduce input bound");
      fe r = a;
      cond_sub<16>(r);
      cond_sub<8>(r);
      cond_sub<4>(r);
      cond_sub<2>(r);
      cond_sub<1>(r);
      BF_SET_BOUND(r, 1);
      return r;
    }
    static HD bool is_zero_limbs(const fe& a)
    {
      uint32_t o = 0;
#pragma unroll
      for (int i = 0; i < N; i++)
        o |= a.l[i];
      return o == 0;
    }
    // exact test a == 0 (mod p) for any in-bound a
    static HD bool is_zero(const fe& a) { return is_zero_limbs(reduce(a)); }
    // Cheap NECESSARY condition for "a == 0 mod p" when a is a Montgomery-product output (< 4p):
    // then a is one of {0,p,2p,3p}, so its lowest limb is one of four constants. False positives
    // (~2^-27) must be followed by is_zero().
    static HD bool maybe_zero_mulout(const fe& a)
    {
      const uint32_t l0 = a.l[0];
      return (l0 == 0) | (l0 == PR::P[0]) | (l0 == ((2 * PR::P[0]) & MASK)) | (l0 == ((3 * PR::P[0]) & MASK));
    }
    static HD bool eq(const fe& a, const fe& b)
    {
      fe ra = reduce(a), rb = reduce(b);
      uint32_t o = 0;
#pragma unroll
      for (int i = 0; i < N; i++)
        o |= ra.l[i] ^ rb.l[i];
      return o == 0;
    }

    // a^(p-2) (Montgomery in, Montgomery out); a = 0 gives 0. Cold paths only (affine conversion).
    static HD fe inv(const fe& a)
    {
      fe r = one(), base = a;
      uint32_t borrow = 2; // exponent p - 2, word by word (BLS12-377's p ends in ...00000001: the borrow travels)
      for (int wi = 0; wi < N32; wi++) {
        const uint32_t w = PR::P32[wi];
        const uint32_t e = w - borrow;
        borrow = w < borrow ? 1u : 0u;
        for (int b = 0; b < 32; b++) {
          if ((e >> b) & 1) r = mul(r, base);
          base = sqr(base);
        }
      }
      return r;
    }

    // ---- packed 32-bit <-> 29-bit limbs ----
    static HD fe unpack(const uint32_t* w)
    { // w[N32] little-endian words -> normalised limbs (no Montgomery conversion)
      fe r;
#pragma unroll
      for (int i = 0; i < N; i++) {
        const int bit = RB * i;
        const int word = bit / 32, sh = bit % 32;
        uint64_t lo = word < N32 ? w[word] : 0;
        uint64_t hi = (word + 1) < N32 ? w[word + 1] : 0;
        uint32_t v = (uint32_t)(((hi << 32) | lo) >> sh);
        r.l[i] = (i == N - 1) ? v : (v & MASK);
      }
      BF_SET_BOUND(r, 1.2); // caller-supplied canonical value (< 2^NBITS may slightly exceed p)
      return r;
    }
    static HD void pack(uint32_t* w, const fe& a)
    { // a must be canonical ([0,p)), limbs normalised
#pragma unroll
      for (int j = 0; j < N32; j++) {
        const int bit = 32 * j;
        const int i = bit / RB, sh = bit % RB; // word j starts inside limb i at bit sh
        uint64_t v = (uint64_t)a.l[i] >> sh;
        int have = RB - sh;
        if (i + 1 < N) v |= (uint64_t)a.l[i + 1] << have;
        have += RB;
        if (have < 32 && i + 2 < N) v |= (uint64_t)a.l[i + 2] << have;
        w[j] = (uint32_t)v;
      }
    }

    // canonical words -> Montgomery element ; Montgomery element -> canonical words
    static HD fe from_canonical(const uint32_t* w)
    {
      fe r2;
#pragma unroll
      for (int i = 0; i < N; i++)
        r2.l[i] = PR::R2[i];
      BF_SET_BOUND(r2, 1);
      return mul(unpack(w), r2);
    }
    static HD fe from_refmont(const uint32_t* w)
    { // reference Montgomery form (x*2^(32*N32)) -> our Montgomery form
      fe c;
#pragma unroll
      for (int i = 0; i < N; i++)
        c.l[i] = PR::REFMONT_TO_MONT[i];
      BF_SET_BOUND(c, 1);
      return mul(unpack(w), c);
    }
    static HD void to_canonical(uint32_t* w, const fe& a)
    {
      fe o = zero();
      o.l[0] = 1;
      BF_SET_BOUND(o, 1);
      pack(w, reduce(mul(a, o)));
    }
    static HD void to_refmont(uint32_t* w, const fe& a)
    {
      fe c;
#pragma unroll
      for (int i = 0; i < N; i++)
        c.l[i] = PR::MONT_TO_REFMONT[i];
      BF_SET_BOUND(c, 1);
      pack(w, reduce(mul(a, c)));
    }
  };

} // namespace icicle_hip
