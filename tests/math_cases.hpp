// TEST-ONLY: the case bodies that tests/host_math_harness.cpp (host build, bound tracker on) and tests/device_math_harness.hip
// (gfx950 build, one operand tuple per thread) both run, so that the CPU and the GPU legs execute the same header calls on the
// same operands and differ only in what the compiler made of them (on the device the products of N = 9 / N = 14 fields are the
// inline-asm blocks of mont_asm.hpp unless -DBIGFIELD_NO_ASM). Not part of the shipped library.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include "../icicle_amd/csrc/ec.hpp"
#include "../icicle_amd/csrc/ec_dbl_quad.hpp"
#include "../icicle_amd/csrc/smallfield.hpp"
#include "../icicle_amd/csrc/goldfield.hpp"

namespace math_cases {
  using namespace icicle_hip;

  template <class T>
  struct Tag {
    using type = T;
  };
  template <class F>
  struct is_gold : std::false_type {
  };
  template <>
  struct is_gold<FieldOps<goldilocks_params>> : std::true_type {
  };

  // field ids: 0..6 the 29-bit-radix parameter sets, 7 goldilocks, 8..10 Fq2 over the three G2 base fields
  template <class Fn>
  inline int with_field(int field, Fn&& fn)
  {
    switch (field) {
    case 0: return fn(Tag<FieldOps<bn254_fq_params>>{});
    case 1: return fn(Tag<FieldOps<bn254_fr_params>>{});
    case 2: return fn(Tag<FieldOps<bls12_381_fq_params>>{});
    case 3: return fn(Tag<FieldOps<bls12_381_fr_params>>{});
    case 4: return fn(Tag<FieldOps<bls12_377_fq_params>>{});
    case 5: return fn(Tag<FieldOps<bls12_377_fr_params>>{});
    case 6: return fn(Tag<FieldOps<stark252_fr_params>>{});
    case 7: return fn(Tag<FieldOps<goldilocks_params>>{});
    case 8: return fn(Tag<Fq2Ops<bn254_fq_params>>{});
    case 9: return fn(Tag<Fq2Ops<bls12_381_fq_params>>{});
    case 10: return fn(Tag<Fq2Ops<bls12_377_fq_params>>{});
    }
    return -1;
  }
  template <class Fn>
  inline int with_raw_field(int field, Fn&& fn)
  {
    return (field >= 0 && field <= 6) ? with_field(field, fn) : -1;
  }
  template <class Fn>
  inline int with_curve(int curve, Fn&& fn)
  {
    switch (curve) {
    case 0: return fn(Tag<bn254_g1>{});
    case 1: return fn(Tag<bls12_381_g1>{});
    case 2: return fn(Tag<bn254_g2>{});
    case 3: return fn(Tag<bls12_381_g2>{});
    case 4: return fn(Tag<bls12_377_g1>{});
    case 5: return fn(Tag<grumpkin_g1>{});
    case 6: return fn(Tag<bls12_377_g2>{});
    }
    return -1;
  }

  // ---- canonical mode: F::N32 words per operand in, from_canonical, op, to_canonical, F::N32 words out ------------------------
  // ops 0..9 are those of host_field_op; 10.. the ones only this tier reaches at field level
  template <class F>
  HD int field_case(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out)
  {
    using fe = typename F::fe;
    fe x = F::from_canonical(a), y = F::from_canonical(b), r;
    auto flag = [&](bool v) {
      for (int i = 0; i < F::N32; i++)
        out[i] = 0;
      out[0] = v ? 1 : 0;
      return 0;
    };
    switch (op) {
    case 0: r = F::mul(x, y); break;
    case 1: r = F::sqr(x); break;
    case 2: r = F::add(x, y); break;
    case 3: r = F::template sub<2>(x, y); break;
    case 4: r = F::template neg<2>(x); break;
    case 5: { // stress lazy bounds: ((x+y)+(x+y)) * (x - y + 8p) ...
      auto s = F::add(F::add(x, y), F::add(x, y));
      auto t = F::template sub<8>(x, F::add(F::add(y, y), F::add(y, y)));
      r = F::mul(s, t); // 2(x+y)(x-4y)
      break;
    }
    case 6: r = F::from_refmont(a); break; // from reference-Montgomery words -> canonical
    case 7: F::to_refmont(out, x); return 0; // canonical -> reference-Montgomery words
    case 8: return flag(F::is_zero(F::template sub<2>(x, y)));
    case 9: r = F::inv(x); break; // x^(p-2); 0 -> 0 (the reference's inverse(0) = 0, projective.h:55-59)
    case 15: r = F::dbl(x); break;
    case 16: r = F::select(true, x, y); break;
    case 17: r = F::select(false, x, y); break;
    case 18: return flag(F::eq(x, y));
    case 19: return flag(F::is_zero(x));
    default:
      if constexpr (!is_gold<F>::value) {
        fe z = F::from_canonical(c), w = F::from_canonical(d);
        switch (op) {
        case 10: r = F::mul_add(x, y, z, w); break; // a*b + c*d
        case 11: // a <- a*b
          r = x;
          F::mul_inplace(r, y);
          break;
        case 12: // a <- a*a, the operand aliased
          r = x;
          F::mul_inplace(r, r);
          break;
        case 13: // c <- a*b + c*d
          r = z;
          F::mul_add_inplace_c(r, x, y, w);
          break;
        case 14: // a aliases c: c <- c*b + c*d
          r = z;
          F::mul_add_inplace_c(r, r, y, w);
          break;
        case 20: // b and d alias c: c <- a*c + c*c
          r = z;
          F::mul_add_inplace_c(r, x, r, r);
          break;
        case 21: // constant operand: a <- a * R^2 (the limbs of from_canonical's constant)
          r = x;
          F::mul_inplace(r, F::r2());
          break;
        default: return -1;
        }
        break;
      }
      return -1;
    }
    F::to_canonical(out, r);
    return 0;
  }

  // ---- raw mode: 29-bit limbs in, ONE op, 29-bit limbs out, no conversion. kb[i] = the bound (units of p) the caller states for
  // operand i: the host build hands it to the tracker, so a tuple outside a precondition aborts on the CPU.
  template <class F, int K>
  HD typename F::fe raw_cond_sub(typename F::fe x)
  {
    F::template cond_sub<K>(x);
    return x;
  }
  template <class F>
  HD int raw_case(int op, int K, const int* kb, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out)
  {
    using fe = typename F::fe;
    constexpr int N = F::N;
    auto load = [&](const uint32_t* l, int k) {
      fe r;
      for (int i = 0; i < N; i++)
        r.l[i] = l[i];
      BF_SET_BOUND(r, (double)k);
      (void)k;
      return r;
    };
    auto flag = [&](bool v) {
      for (int i = 0; i < N; i++)
        out[i] = 0;
      out[0] = v ? 1 : 0;
      return 0;
    };
    const fe x = load(a, kb[0]), y = load(b, kb[1]);
    fe r;
    switch (op) {
    case 0: r = F::mul(x, y); break;
    case 1: r = F::sqr(x); break;
    case 2: r = F::mul_add(x, y, load(c, kb[2]), load(d, kb[3])); break;
    case 3: r = F::add(x, y); break;
    case 4:
      switch (K) {
      case 2: r = F::template sub<2>(x, y); break;
      case 4: r = F::template sub<4>(x, y); break;
      case 8: r = F::template sub<8>(x, y); break;
      case 16: r = F::template sub<16>(x, y); break;
      default: return -1;
      }
      break;
    case 5: r = F::reduce(x); break;
    case 6: r = F::below4(x); break;
    case 7:
      switch (K) {
      case 1: r = raw_cond_sub<F, 1>(x); break;
      case 2: r = raw_cond_sub<F, 2>(x); break;
      case 4: r = raw_cond_sub<F, 4>(x); break;
      case 8: r = raw_cond_sub<F, 8>(x); break;
      case 16: r = raw_cond_sub<F, 16>(x); break;
      default: return -1;
      }
      break;
    case 8: return flag(F::is_zero(x));
    case 9: return flag(F::eq(x, y));
    case 10: return flag(F::maybe_zero_mulout(x));
    case 11: // pack: canonical limbs -> N32 words (zero padded to N)
      for (int i = 0; i < N; i++)
        out[i] = 0;
      F::pack(out, x);
      return 0;
    case 12: r = F::unpack(a); break; // N32 words -> limbs
    default: return -1;
    }
    for (int i = 0; i < N; i++)
      out[i] = r.l[i];
    return 0;
  }

  // ---- 31-bit fields: canonical residues in and out -----------------------------------------------------------------------------
  template <class PR>
  HD int small_case(int op, uint32_t a, uint32_t b, uint32_t* out)
  {
    using S = SmallField<PR>;
    uint32_t x = S::to_mont(a), y = S::to_mont(b), r;
    switch (op) {
    case 0: r = S::mul(x, y); break;
    case 1: r = S::add(x, y); break;
    case 2: r = S::sub(x, y); break;
    case 3: r = S::pow(x, b); break; // x^b (b plain integer)
    case 4: r = S::inv(x); break;
    case 5: r = S::neg(x); break;
    default: return -1;
    }
    *out = S::from_mont(r);
    return 0;
  }

  // ---- EC tier. points: affine canonical words (x,y); identity (0,0). ops 0, 1, 2, 3, 4, 5, 6 of host_ec_op; 7 (add_signed) and 8
  // (EcDblSmallB::dbl) answer -1 for the curves that do not have them ---------------------------------------------------------------
  template <class C>
  HD int ec_case(int op, const uint32_t* pts, int n, const uint32_t* aux, uint32_t* out)
  {
    using E = EC<C>;
    using F = typename E::F;
    constexpr int N32 = E::N32;
    // Montgomery-form affine point (cold kernels: precompute, generator, complete adds)
    auto load = [&](const uint32_t* w) {
      typename E::Aff a;
      a.x = F::from_canonical(w);
      a.y = F::from_canonical(w + N32);
      return a;
    };
    switch (op) {
    case 0: { // XYZZ accumulate all points (aux[i]&1 = negate), output projective canonical
      typename E::XYZZ acc;
      bool empty = true;
      for (int i = 0; i < n; i++) {
        const uint32_t* w = pts + (size_t)i * 2 * N32;
        if (E::words_are_zero(w)) continue;
        // the hot loop consumes the canonical words exactly as they lie in HBM (ec.hpp scaling convention)
        auto a = E::cneg(E::load_plain(w), aux && (aux[i] & 1));
        E::madd(acc, empty, a);
      }
      E::store_proj_canonical(out, E::to_proj(acc, empty));
      return 0;
    }
    case 1: { // complete projective sum of all points (identity allowed)
      auto acc = E::proj_identity();
      for (int i = 0; i < n; i++) {
        const uint32_t* w = pts + (size_t)i * 2 * N32;
        if (E::words_are_zero(w)) {
          acc = E::add(acc, E::proj_identity());
          continue;
        }
        acc = E::add(acc, E::to_proj(E::cneg(load(w), aux && (aux[i] & 1))));
      }
      E::store_proj_canonical(out, acc);
      return 0;
    }
    case 2: { // mul_small: aux[0] * pts[0]
      auto p = E::words_are_zero(pts) ? E::proj_identity() : E::to_proj(load(pts));
      E::store_proj_canonical(out, E::mul_small(p, aux[0]));
      return 0;
    }
    case 3: { // generator
      E::store_proj_canonical(out, E::to_proj(E::generator()));
      return 0;
    }
    case 4: { // repeated doubling: 2^aux[0] * pts[0] via complete dbl
      auto p = E::to_proj(load(pts));
      for (uint32_t i = 0; i < aux[0]; i++)
        p = E::dbl(p);
      E::store_proj_canonical(out, p);
      return 0;
    }
    case 5: { // the window-combine chain: 2^aux[0] * pts[0] via to_jac / dbl_jac / from_jac
      auto p = E::words_are_zero(pts) ? E::proj_identity() : E::add(E::to_proj(load(pts)), E::proj_identity()); // a non-trivial Z
      auto j = E::to_jac(p);
      for (uint32_t i = 0; i < aux[0]; i++)
        j = E::dbl_jac(j);
      E::store_proj_canonical(out, E::from_jac(j));
      return 0;
    }
    case 6: { // msm_precompute_bases' chain: 2^aux[0] * pts[0] via dbl_jac_lazy from Z = 1, reduced at the end (bounds tracked)
      if (E::words_are_zero(pts)) {
        E::store_proj_canonical(out, E::proj_identity());
        return 0;
      }
      typename E::Jac j;
      const auto a = load(pts);
      j.x = a.x, j.y = a.y, j.z = F::one();
      for (uint32_t i = 0; i < aux[0]; i++)
        j = E::dbl_jac_lazy(j);
      j.x = F::reduce(j.x), j.y = F::reduce(j.y), j.z = F::reduce(j.z);
      E::store_proj_canonical(out, E::from_jac(j));
      return 0;
    }
    case 7: { // one lane of k_reduce_wave on the signed layer (the curves with SIGNED_MADD): the buckets b_0 .. b_{n-1} as they lie in memory
              // (unsigned normalised Proj, the identity as proj_identity()), tri = add_signed(tri, line); line = add_signed(line, b_i) from two
              // identities; output signed_to_unsigned(add_signed(tri, line)) = sum (n - i) b_i
      if constexpr (E::SIGNED_MADD) {
        auto tri = E::proj_identity(), line = E::proj_identity();
        for (int i = 0; i < n; i++) {
          const uint32_t* w = pts + (size_t)i * 2 * N32;
          const auto b = E::words_are_zero(w) ? E::proj_identity() : E::to_proj(E::cneg(load(w), aux && (aux[i] & 1)));
          tri = E::add_signed(tri, line);
          line = E::add_signed(line, b);
        }
        E::store_proj_canonical(out, E::signed_to_unsigned(E::add_signed(tri, line)));
        return 0;
      } else {
        return -1;
      }
    }
    case 8: { // op 5's chain by the complete doubling of ec_dbl_quad.hpp on one lane (the curves with a small 3 b): 2^aux[0] * pts[0]
      if constexpr (has_small_b3<C>::value) {
        auto p = E::words_are_zero(pts) ? E::proj_identity() : E::add(E::to_proj(load(pts)), E::proj_identity()); // a non-trivial Z
        for (uint32_t i = 0; i < aux[0]; i++)
          p = EcDblSmallB<C>::dbl(p);
        E::store_proj_canonical(out, p);
        return 0;
      } else {
        return -1;
      }
    }
    default: return -1;
    }
  }

  // ---- raw projective operands: (X, Y, Z), each coordinate F::N normalised 29-bit limbs per base-field component, taken as they are
  // (Montgomery form, no conversion); K = the bound (units of p) stated for every component, which the host build hands to the tracker
  template <class C>
  struct RawProj {
    using E = EC<C>;
    using F = typename E::F;
    static constexpr int ROW = 3 * (int)C::EXT_DEGREE * F::N; // limbs per point
    template <class BFE>
    static HD void comp(BFE& dst, const uint32_t* l, int K)
    {
      for (int i = 0; i < F::N; i++)
        dst.l[i] = l[i];
      BF_SET_BOUND(dst, (double)K);
      (void)K;
    }
    static HD typename E::Proj load(const uint32_t* l, int K)
    {
      typename E::Proj r;
      if constexpr (C::EXT_DEGREE == 2) {
        comp(r.x.c0, l, K), comp(r.x.c1, l + F::N, K);
        comp(r.y.c0, l + 2 * F::N, K), comp(r.y.c1, l + 3 * F::N, K);
        comp(r.z.c0, l + 4 * F::N, K), comp(r.z.c1, l + 5 * F::N, K);
      } else {
        comp(r.x, l, K), comp(r.y, l + F::N, K), comp(r.z, l + 2 * F::N, K);
      }
      return r;
    }
  };
  // the one-lane twins of the quad tier on raw operands (host: under the tracker). fn 0: E::add of two points, fn 2: EcDblSmallB::dbl of one
  template <class C>
  HD int ec_raw_case(int fn, int K, const uint32_t* limbs, uint32_t* out)
  {
    using E = EC<C>;
    using RP = RawProj<C>;
    if (fn == 0) {
      E::store_proj_canonical(out, E::add(RP::load(limbs, K), RP::load(limbs + RP::ROW, K)));
      return 0;
    }
    if (fn == 2) {
      if constexpr (has_small_b3<C>::value) {
        E::store_proj_canonical(out, EcDblSmallB<C>::dbl(RP::load(limbs, K)));
        return 0;
      }
    }
    return -1;
  }
} // namespace math_cases
