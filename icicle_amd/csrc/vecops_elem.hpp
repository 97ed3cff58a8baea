// The three kinds of base-field element behind one interface: one Montgomery word, nine 29-bit Montgomery limbs, one canonical
// 64-bit Goldilocks value. vecops_ext_elem.hpp holds the extension elements behind the same interface, vecops_tile.hpp the kernels.
//
// load / store / apply are the element-wise interface of vector_add / sub / mul. What follows them in each struct is what the
// inversion and the reductions need. There a loaded value x is never converted: it is read as the Montgomery representative of
// x / R, mul_raw multiplies representatives (for Goldilocks: plain values, R = 1) and one() is the representative of 1, so that a
// chain of mul_raw over any tree stays consistent and the powers of R are settled once at its end:
//   * the inverse of a representative x is R^2 / x (inv_raw, or the powers x^(2^t) by sqr_raw put together by the bits of p - 2,
//     pm2_bit, where WAVE_POW says that a wave shares that work), and every quotient of the shared inversion is linear in the one
//     inverse of a tile: unscale() takes one R off it, twice for plain inverses, once where a product with a numerator follows;
//   * a product of n loaded values through mul_raw is prod / R^(n-1): scale_pow(x, n) puts R^(n-1) back.
#pragma once
#include "common.h"
#include "vecops_op.h"
#include "bigfield.hpp"
#include "smallfield.hpp"
#include "goldfield.hpp"

namespace icicle_hip {

  template <class PR>
  struct SmallElem {
    using S = SmallField<PR>;
    static constexpr int W = 1;
    struct T {
      uint32_t v;
    };
    static __device__ __forceinline__ T load(const uint32_t* p) { return T{*p}; }
    static __device__ __forceinline__ void store(uint32_t* p, const T& x) { *p = x.v; }
    static __device__ __forceinline__ T apply(int op, const T& a, const T& b)
    {
      if (op == VOP_ADD) return T{S::add(a.v, b.v)};
      if (op == VOP_SUB) return T{S::sub(a.v, b.v)};
      return T{S::mul(S::mul(a.v, b.v), PR::R2)};
    }

    static __device__ __forceinline__ T zero() { return T{0}; }
    static __device__ __forceinline__ T one() { return T{PR::ONE}; }
    static __device__ __forceinline__ bool is_zero(const T& a) { return a.v == 0; }
    static __device__ __forceinline__ T sum(const T& a, const T& b) { return T{S::add(a.v, b.v)}; }
    static __device__ __forceinline__ T mul_raw(const T& a, const T& b) { return T{S::mul(a.v, b.v)}; }
    static constexpr bool WAVE_POW = false; // 31 squarings: not worth sharing
    static __device__ __forceinline__ T inv_raw(const T& a) { return T{S::inv(a.v)}; }
    static __device__ __forceinline__ T unscale(const T& a) { return T{S::from_mont(a.v)}; }
    static __device__ __forceinline__ T scale_pow(const T& a, uint64_t n) { return T{S::mul(a.v, S::pow(PR::R2, n - 1))}; }
  };

  template <class PR>
  struct BigElem {
    using F = FieldOps<PR>;
    static constexpr int W = F::N32;
    using T = typename F::fe;
    static __device__ __forceinline__ T load(const uint32_t* p)
    {
      uint32_t w[W];
#pragma unroll
      for (int i = 0; i < W; i++)
        w[i] = p[i];
      return F::unpack(w);
    }
    static __device__ __forceinline__ void store(uint32_t* p, const T& x)
    {
      uint32_t w[W];
      F::pack(w, F::reduce(x));
#pragma unroll
      for (int i = 0; i < W; i++)
        p[i] = w[i];
    }
    static __device__ __forceinline__ T apply(int op, const T& a, const T& b)
    {
      if (op == VOP_ADD) return F::add(a, b);
      if (op == VOP_SUB) return F::template sub<2>(a, b);
      return F::mul(F::mul(a, b), F::from_const(PR::R2));
    }

    // lazy bounds (bigfield.hpp): a loaded value is below 1.2 p, a product below 1.25 p, a sum is brought back below 4 p
    static __device__ __forceinline__ T zero() { return F::zero(); }
    static __device__ __forceinline__ T one() { return F::one(); }
    static __device__ __forceinline__ bool is_zero(const T& a) { return F::is_zero_limbs(a); } // of a loaded value
    static __device__ __forceinline__ T sum(const T& a, const T& b)
    {
      T r = F::add(a, b);
      F::template cond_sub<4>(r);
      return r;
    }
    static __device__ __forceinline__ T mul_raw(const T& a, const T& b) { return F::mul(a, b); }
    static constexpr bool WAVE_POW = true;
    static constexpr int NBITS = PR::NBITS;
    static __device__ __forceinline__ T sqr_raw(const T& a) { return F::sqr(a); }
    static __device__ __forceinline__ bool pm2_bit(int i) // bit i of p - 2, i < 32 W (the borrow travels: BLS12-377's p ends in ...00000001)
    {
      uint32_t borrow = 2, word = 0;
#pragma unroll
      for (int k = 0; k < W; k++) {
        const uint32_t w = PR::P32[k], e = w - borrow;
        borrow = w < borrow ? 1u : 0u;
        word = k == (i >> 5) ? e : word;
      }
      return (word >> (i & 31)) & 1;
    }
    static __device__ __forceinline__ T unscale(const T& a) { return F::mul(a, F::plain_one()); }
    static __device__ __forceinline__ T scale_pow(const T& a, uint64_t n)
    {
      T r = F::one(), base = F::r2(); // r2 represents R: the power below represents R^(n-1), which is R^n as it lies
      for (uint64_t e = n - 1; e; e >>= 1) {
        if (e & 1) r = F::mul(r, base);
        base = F::sqr(base);
      }
      return F::mul(a, r);
    }
  };

  struct GoldElem { // goldilocks: canonical 64-bit values, goldfield.hpp
    using F = FieldOps<goldilocks_params>;
    static constexpr int W = 2;
    using T = GoldFe;
    static __device__ __forceinline__ T load(const uint32_t* p) { return F::unpack(p); }
    static __device__ __forceinline__ void store(uint32_t* p, const T& x) { F::pack(p, x); }
    static __device__ __forceinline__ T apply(int op, const T& a, const T& b)
    {
      if (op == VOP_ADD) return F::add(a, b);
      if (op == VOP_SUB) return F::template sub<2>(a, b);
      return F::mul(a, b);
    }

    static __device__ __forceinline__ T zero() { return F::zero(); }
    static __device__ __forceinline__ T one() { return F::one(); }
    static __device__ __forceinline__ bool is_zero(const T& a) { return a.v == 0; }
    static __device__ __forceinline__ T sum(const T& a, const T& b) { return F::add(a, b); }
    static __device__ __forceinline__ T mul_raw(const T& a, const T& b) { return F::mul(a, b); }
    static constexpr bool WAVE_POW = false;
    static __device__ __forceinline__ T inv_raw(const T& a) { return F::inv(a); }
    static __device__ __forceinline__ T unscale(const T& a) { return a; }
    static __device__ __forceinline__ T scale_pow(const T& a, uint64_t) { return a; }
  };

} // namespace icicle_hip
