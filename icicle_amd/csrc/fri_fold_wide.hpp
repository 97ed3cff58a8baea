// The arithmetic of one FRI fold over FieldOps<PR> -- Goldilocks (goldfield.hpp) and the 256-bit scalar fields (bigfield.hpp) --
// for host and device: fri_wide.hip's kernel and its host verifier use it, and tests/fri_wide_host_harness.cpp compiles it with
// g++ and compares it with Python integers.
//
//   out = (lo + hi)/2 + alpha * ((lo - hi)/2 * tw)  =  ((lo + hi) + alpha * ((lo - hi) * tw)) / 2
//
// so there is ONE halving per coefficient, at the end. lo and hi are unpacked canonical values; tw and alpha are in the form the
// field multiplies by: Montgomery for the 256-bit fields (mul(canonical, x*R) is the canonical product, lazily reduced), plain for
// Goldilocks, which has no Montgomery form on the device. The result is fully reduced, ready to pack.
//
// Halving without a product: x/2 = (x + (x odd ? p : 0)) >> 1. The 256-bit fields carry it through their 29-bit limbs -- one
// limb-wise add of p under a mask and one funnel shift per limb, about 4 N VALU ops against the 2 N^2 multiply-adds of a product
// with 1/2, and it accepts the lazy sum as it is (< 4p in, < 2.5p out). For Goldilocks x + p does not fit in 64 bits:
// (x >> 1) + (x & 1) * ((p + 1)/2) is the same value and stays below p.
#pragma once
#include "bigfield.hpp"
#include "goldfield.hpp"

namespace icicle_hip {

  template <class PR>
  struct FriHalf {
    using F = FieldOps<PR>;
    using fe = typename F::fe;
    // u: normalised limbs, value < 32p; the result is u/2 mod p as a value, < (u + p)/2
    static HD fe half(const fe& u)
    {
      constexpr int N = F::N;
      const uint32_t odd = 0u - (u.l[0] & 1u); // all ones when p has to be added
      fe t, r;
      uint32_t c = 0;
#pragma unroll
      for (int i = 0; i < N - 1; i++) {
        const uint32_t s = u.l[i] + (PR::P[i] & odd) + c;
        t.l[i] = s & F::MASK;
        c = s >> RB;
      }
      t.l[N - 1] = u.l[N - 1] + (PR::P[N - 1] & odd) + c;
#pragma unroll
      for (int i = 0; i < N - 1; i++)
        r.l[i] = (t.l[i] >> 1) | ((t.l[i + 1] & 1u) << (RB - 1));
      r.l[N - 1] = t.l[N - 1] >> 1;
      BF_SET_BOUND(r, (u.bnd + 1.0) / 2);
      return r;
    }
  };
  template <>
  struct FriHalf<goldilocks_params> {
    using fe = GoldFe;
    static HD fe half(const fe& u) { return FieldOps<goldilocks_params>::make((u.v >> 1) + (u.v & 1) * ((goldilocks_params::P + 1) / 2)); }
  };

  template <class PR>
  struct FriWideFold {
    using F = FieldOps<PR>;
    using fe = typename F::fe;

    // one scalar fold
    static HD fe fold1(const fe& lo, const fe& hi, const fe& tw, const fe& alpha)
    {
      const fe odd = F::mul(F::mul(F::template sub<2>(lo, hi), tw), alpha);
      return F::reduce(FriHalf<PR>::half(F::add(F::add(lo, hi), odd)));
    }

    // one fold of a quadratic extension element a0 + a1 u, u^2 = NONRES: alpha = (a0, a1), a1n = NONRES * a1
    static HD void fold2(const fe* lo, const fe* hi, const fe& tw, const fe& a0, const fe& a1, const fe& a1n, fe* out)
    {
      const fe o0 = F::mul(F::template sub<2>(lo[0], hi[0]), tw), o1 = F::mul(F::template sub<2>(lo[1], hi[1]), tw);
      const fe r0 = F::add(F::mul(o0, a0), F::mul(o1, a1n)), r1 = F::add(F::mul(o0, a1), F::mul(o1, a0));
      out[0] = F::reduce(FriHalf<PR>::half(F::add(F::add(lo[0], hi[0]), r0)));
      out[1] = F::reduce(FriHalf<PR>::half(F::add(F::add(lo[1], hi[1]), r1)));
    }
  };

} // namespace icicle_hip
