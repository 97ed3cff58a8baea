// The extension-field elements of vecops_ext.hip behind the element interface of vecops_elem.hpp: the quartic extension
// F[x] / (x^4 - W) of BabyBear and KoalaBear (W = FriField<PR>::W, four canonical words, constant term first) and the quadratic
// extension c0 + c1 u, u^2 = goldilocks_params::EXT_NONRES, of Goldilocks (two canonical 64-bit values). 16 bytes either way.
//
// Reference: icicle/include/icicle/fields/quartic_extension.h (operator*, :247 inverse through the norm), complex_extension.h.
//
// As in vecops_elem.hpp a loaded word x of a 31-bit field is read as the Montgomery representative of x / R, coefficient by
// coefficient: mul_raw multiplies representatives and W enters as its own representative, so that a chain of mul_raw over any tree
// stays consistent and scale_pow settles the powers of R at its end. apply() is the element-wise interface: canonical in and out.
// norm() goes down the tower x^2 = y, y^2 = W to the base field and conj_times() is the numerator of the inverse:
// a^-1 = conj_times(a) / norm(a). Everything here is host and device code: tests/vecops_ext_host_harness.cpp runs it under g++.
#pragma once
#include "vecops_op.h"
#include "smallfield.hpp"
#include "goldfield.hpp"

namespace icicle_hip {

  struct Ext4 {
    uint32_t c[4];
  };

  template <class PR>
  struct SmallExtElem {
    using S = SmallField<PR>;
    static constexpr int W = 4;  // words per element
    static constexpr int BW = 1; // words per base-field element
    using T = Ext4;
    using BT = uint32_t; // a base-field representative
    static constexpr uint32_t NONRES = FriField<PR>::W;

    static SF_HD uint32_t wm() { return S::to_mont(NONRES); }            // the representative of W
    static SF_HD uint32_t wr2() { return S::to_mont(S::to_mont(NONRES)); } // W R^2: montmul(b, W R^2) = W b R

    static SF_HD T load(const uint32_t* p) { return T{{p[0], p[1], p[2], p[3]}}; }
    static SF_HD void store(uint32_t* p, const T& x)
    {
      p[0] = x.c[0], p[1] = x.c[1], p[2] = x.c[2], p[3] = x.c[3];
    }
    static SF_HD BT load_base(const uint32_t* p) { return *p; }
    static SF_HD T zero() { return T{{0, 0, 0, 0}}; }
    static SF_HD T one() { return T{{PR::ONE, 0, 0, 0}}; }
    static SF_HD bool is_zero(const T& a) { return (a.c[0] | a.c[1] | a.c[2] | a.c[3]) == 0; }
    static SF_HD T sum(const T& a, const T& b) { return T{{S::add(a.c[0], b.c[0]), S::add(a.c[1], b.c[1]), S::add(a.c[2], b.c[2]), S::add(a.c[3], b.c[3])}}; }
    static SF_HD T diff(const T& a, const T& b) { return T{{S::sub(a.c[0], b.c[0]), S::sub(a.c[1], b.c[1]), S::sub(a.c[2], b.c[2]), S::sub(a.c[3], b.c[3])}}; }

    // x0 y0 + x1 y1 in one reduction (the fri_dot2 of fri.hip): 2 p^2 < p 2^32
    static SF_HD uint32_t dot2(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1) { return S::mont_reduce((uint64_t)x0 * y0 + (uint64_t)x1 * y1); }
    // four products in one reduction: their sum is below 4 p^2 < 2 p 2^32, so one conditional subtraction of p 2^32 (which leaves
    // the residue alone) brings it under mont_reduce's bound
    static SF_HD uint32_t dot4(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2, uint32_t x3, uint32_t y3)
    {
      uint64_t t = (uint64_t)x0 * y0 + (uint64_t)x1 * y1 + (uint64_t)x2 * y2 + (uint64_t)x3 * y3;
      const uint64_t m = (uint64_t)PR::P << 32;
      t = t >= m ? t - m : t;
      return S::mont_reduce(t);
    }
    // a * b / R given bw[k] = W b[k], k = 1..3: 16 products in four reductions
    static SF_HD T mul_core(const T& a, const T& b, uint32_t bw1, uint32_t bw2, uint32_t bw3)
    {
      T r;
      r.c[0] = dot4(a.c[0], b.c[0], a.c[1], bw3, a.c[2], bw2, a.c[3], bw1);
      r.c[1] = dot4(a.c[0], b.c[1], a.c[1], b.c[0], a.c[2], bw3, a.c[3], bw2);
      r.c[2] = dot4(a.c[0], b.c[2], a.c[1], b.c[1], a.c[2], b.c[0], a.c[3], bw3);
      r.c[3] = dot4(a.c[0], b.c[3], a.c[1], b.c[2], a.c[2], b.c[1], a.c[3], b.c[0]);
      return r;
    }
    static SF_HD T mul_raw(const T& a, const T& b)
    {
      const uint32_t w = wm();
      return mul_core(a, b, S::mul(b.c[1], w), S::mul(b.c[2], w), S::mul(b.c[3], w));
    }
    // every coefficient times a base-field representative
    static SF_HD T mul_base_raw(const T& a, BT s) { return T{{S::mul(a.c[0], s), S::mul(a.c[1], s), S::mul(a.c[2], s), S::mul(a.c[3], s)}}; }
    static SF_HD T scale_pow(const T& a, uint64_t n) { return mul_base_raw(a, S::pow(PR::R2, n - 1)); }

    // canonical in, canonical out. A product first lifts b to b R and W b R (seven independent reductions), then a * (b R) / R
    static SF_HD T apply(int op, const T& a, const T& b)
    {
      if (op == VOP_ADD) return sum(a, b);
      if (op == VOP_SUB) return diff(a, b);
      const uint32_t r2 = PR::R2, w = wr2();
      const T bm = mul_base_raw(b, r2);
      return mul_core(a, bm, S::mul(b.c[1], w), S::mul(b.c[2], w), S::mul(b.c[3], w));
    }
    static SF_HD T apply_mixed(const T& a, BT b) { return mul_base_raw(a, S::mul(b, PR::R2)); } // a (extension) times b (base), canonical

    // a = A + x B with A = a0 + a2 y, B = a1 + a3 y, y = x^2, y^2 = W. Its norm over F[y] is A^2 - y B^2 = n0 + n1 y,
    //   n0 = a0^2 + W a2^2 - 2 W a1 a3,   n1 = 2 a0 a2 - a1^2 - W a3^2,
    // whose norm over F is n0^2 - W n1^2; and a (A - x B)(n0 - n1 y) is that norm, so the numerator of the inverse is
    //   (a0 n0 - W a2 n1) - (a1 n0 - W a3 n1) x + (a2 n0 - a0 n1) y - (a3 n0 - a1 n1) x y.
    // Returns the norm and leaves the numerator in `num`.
    static SF_HD BT norm_conj(const T& a, T& num)
    {
      const uint32_t w = wm();
      const uint32_t wa2 = S::mul(a.c[2], w), wa3 = S::mul(a.c[3], w);
      const uint32_t t0 = S::mul(a.c[1], wa3), t1 = S::mul(a.c[0], a.c[2]);
      const uint32_t n0 = S::sub(dot2(a.c[0], a.c[0], a.c[2], wa2), S::add(t0, t0));
      const uint32_t n1 = S::sub(S::add(t1, t1), dot2(a.c[1], a.c[1], a.c[3], wa3));
      const uint32_t m0 = PR::P - n0, m1 = PR::P - n1; // -n0, -n1 in [1, p]: the products below stay within dot2's bound
      num.c[0] = dot2(a.c[0], n0, wa2, m1);
      num.c[1] = dot2(wa3, n1, a.c[1], m0);
      num.c[2] = dot2(a.c[2], n0, a.c[0], m1);
      num.c[3] = dot2(a.c[1], n1, a.c[3], m0);
      return S::sub(S::mul(n0, n0), S::mul(S::mul(n1, w), n1));
    }
    static SF_HD BT norm(const T& a)
    {
      T num;
      return norm_conj(a, num);
    }
    static SF_HD T conj_times(const T& a)
    {
      T num;
      norm_conj(a, num);
      return num;
    }
  };

  struct GoldExt {
    GoldFe c[2];
  };

  struct GoldExtElem {
    using F = FieldOps<goldilocks_params>;
    static constexpr int W = 4;
    static constexpr int BW = 2;
    using T = GoldExt;
    using BT = GoldFe;

    static HD GoldFe nonres(const GoldFe& x) { return F::mul(x, F::make(goldilocks_params::EXT_NONRES)); } // u^2 x

    static HD T load(const uint32_t* p) { return T{{F::unpack(p), F::unpack(p + 2)}}; }
    static HD void store(uint32_t* p, const T& x)
    {
      F::pack(p, x.c[0]);
      F::pack(p + 2, x.c[1]);
    }
    static HD BT load_base(const uint32_t* p) { return F::unpack(p); }
    static HD T zero() { return T{{F::zero(), F::zero()}}; }
    static HD T one() { return T{{F::one(), F::zero()}}; }
    static HD bool is_zero(const T& a) { return (a.c[0].v | a.c[1].v) == 0; }
    static HD T sum(const T& a, const T& b) { return T{{F::add(a.c[0], b.c[0]), F::add(a.c[1], b.c[1])}}; }
    static HD T diff(const T& a, const T& b) { return T{{F::template sub<2>(a.c[0], b.c[0]), F::template sub<2>(a.c[1], b.c[1])}}; }
    // four independent products and the small one by u^2: Karatsuba's three would put two additions in front of a product and two
    // subtractions behind it, a longer dependent chain for one 64 x 64 product less
    static HD T mul_raw(const T& a, const T& b)
    {
      return T{{F::add(F::mul(a.c[0], b.c[0]), nonres(F::mul(a.c[1], b.c[1]))), F::add(F::mul(a.c[0], b.c[1]), F::mul(a.c[1], b.c[0]))}};
    }
    static HD T mul_base_raw(const T& a, const BT& s) { return T{{F::mul(a.c[0], s), F::mul(a.c[1], s)}}; }
    static HD T scale_pow(const T& a, uint64_t) { return a; }
    static HD T apply(int op, const T& a, const T& b)
    {
      if (op == VOP_ADD) return sum(a, b);
      if (op == VOP_SUB) return diff(a, b);
      return mul_raw(a, b);
    }
    static HD T apply_mixed(const T& a, const BT& b) { return mul_base_raw(a, b); }
    // (c0 + c1 u)(c0 - c1 u) = c0^2 - u^2 c1^2
    static HD BT norm_conj(const T& a, T& num)
    {
      num.c[0] = a.c[0];
      num.c[1] = F::template neg<2>(a.c[1]);
      return F::template sub<2>(F::sqr(a.c[0]), nonres(F::sqr(a.c[1])));
    }
    static HD BT norm(const T& a)
    {
      T num;
      return norm_conj(a, num);
    }
    static HD T conj_times(const T& a)
    {
      T num;
      norm_conj(a, num);
      return num;
    }
  };

#if defined(__HIPCC__)
  // Vec16<EL> is EL with one 16-byte access per element: what the kernels of vecops_tile.hpp are instantiated with where every
  // device pointer of a call is 16-byte aligned (aligned16; a staging buffer always is). EL itself goes word by word.
  template <class EL>
  struct Vec16 : EL {
    static __device__ __forceinline__ typename EL::T load(const uint32_t* p)
    {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      return EL::load(w);
    }
    static __device__ __forceinline__ void store(uint32_t* p, const typename EL::T& x)
    {
      uint32_t w[4];
      EL::store(w, x);
      *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    static __device__ __forceinline__ typename EL::BT load_base(const uint32_t* p)
    {
      if constexpr (EL::BW == 2) {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        const uint32_t w[2] = {v.x, v.y};
        return EL::load_base(w);
      } else {
        return EL::load_base(p);
      }
    }
  };
#endif

} // namespace icicle_hip
