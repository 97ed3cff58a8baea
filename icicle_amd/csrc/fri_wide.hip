// FRI over the fields wider than 31 bits -- Goldilocks (8-byte elements) with its quadratic extension (16 bytes, a0 + a1 u with
// u^2 = 7, constant term first), and the 256-bit scalar fields stark252, BN254, BLS12-381, BLS12-377 (32 bytes): the fold kernel
// over FieldOps<PR> and the field kind that fri_protocol.hpp's prover and verifier are instantiated with.
//
// The fold: out[i] = (e[i] + e[i+h])/2 + alpha * ((e[i] - e[i+h])/2 * w_n^(-i)), h = n/2 (arithmetic: fri_fold_wide.hpp). Elements
// are canonical in memory. The twiddles are gathered from the current device's NTT domain (ntt_big.hip's BigDomain table, stride
// max/n): packed Montgomery values for the 256-bit fields, so that mul(canonical, Montgomery) is canonical and no conversion pass
// is needed, and alpha is brought into Montgomery form once on the host; Goldilocks has no Montgomery form on the device and its
// table is canonical. A lane moves 16 bytes per access: two consecutive Goldilocks scalars from each half, one extension element,
// or a 256-bit element as two accesses; pointers that are only word-aligned take the word-by-word variant.
#include "common.h"
#include "ntt_big_common.hpp"
#include "fri_fold_wide.hpp"
#include "fri_protocol.hpp"

namespace icicle_hip {

  template <class PR>
  struct FriWideField; // field index of ntt_big_domain_table
  template <>
  struct FriWideField<bn254_fr_params> {
    static constexpr int INDEX = 0;
  };
  template <>
  struct FriWideField<bls12_381_fr_params> {
    static constexpr int INDEX = 1;
  };
  template <>
  struct FriWideField<bls12_377_fr_params> {
    static constexpr int INDEX = 2;
  };
  template <>
  struct FriWideField<stark252_fr_params> {
    static constexpr int INDEX = 3;
  };
  template <>
  struct FriWideField<goldilocks_params> {
    static constexpr int INDEX = 4;
  };

  // alpha for the kernel, in the form the field multiplies by: a0 (scalar), or a0 + a1 u with a1n = 7 a1 (extension)
  template <class PR>
  struct WideFoldConsts {
    typename FieldOps<PR>::fe a0, a1, a1n;
  };

  // EW words of one element: VEC ? 16 bytes per access : word by word
  template <int EW, bool VEC>
  __device__ __forceinline__ void fri_load_words(uint32_t* dst, const uint32_t* __restrict__ src)
  {
    if constexpr (VEC) {
      static_assert(EW % 4 == 0, "whole 16-byte accesses");
#pragma unroll
      for (int q = 0; q < EW / 4; q++) {
        const uint4 v = reinterpret_cast<const uint4*>(src)[q];
        dst[4 * q] = v.x, dst[4 * q + 1] = v.y, dst[4 * q + 2] = v.z, dst[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < EW; q++)
        dst[q] = src[q];
    }
  }
  template <int EW, bool VEC>
  __device__ __forceinline__ void fri_store_words(uint32_t* __restrict__ dst, const uint32_t* src)
  {
    if constexpr (VEC) {
#pragma unroll
      for (int q = 0; q < EW / 4; q++)
        reinterpret_cast<uint4*>(dst)[q] = make_uint4(src[4 * q], src[4 * q + 1], src[4 * q + 2], src[4 * q + 3]);
    } else {
#pragma unroll
      for (int q = 0; q < EW; q++)
        dst[q] = src[q];
    }
  }

  // tw[(max - (max >> k) i) & (max - 1)] = w_n^(-i) for n = 2^k (the reference's tw_idx; i = 0 wraps to tw[0] = 1); W words each
  template <class PR>
  __device__ __forceinline__ typename FieldOps<PR>::fe fri_wide_twiddle(const uint32_t* __restrict__ tw, uint32_t log_max, uint32_t k, uint64_t i)
  {
    constexpr int W = FieldOps<PR>::N32;
    const uint64_t max = (uint64_t)1 << log_max;
    uint32_t w[W];
    loadw<W>(w, tw + ((max - ((max >> k) * i)) & (max - 1)) * W);
    return FieldOps<PR>::unpack(w);
  }

  // COEFFS = 1: scalars; with two-word elements (Goldilocks) and VEC a lane takes two consecutive i (h even), else one i per lane.
  // COEFFS = 2: one extension element per lane. VEC: 16-byte aligned pointers, 16 bytes per access; else word by word.
  // `lanes` = h / 2 (two-word scalars, VEC) or h.
  template <class PR, int COEFFS, bool VEC>
  __global__ __launch_bounds__(256) void k_fri_fold_wide(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ tw, WideFoldConsts<PR> c,
                                                         uint64_t h, uint64_t lanes, uint32_t k, uint32_t log_max)
  {
    using F = FieldOps<PR>;
    using fe = typename F::fe;
    using A = FriWideFold<PR>;
    constexpr int W = F::N32, EW = W * COEFFS;
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    if constexpr (EW == 2 && VEC) {
      uint32_t lo[4], hi[4], r[4];
      fri_load_words<4, true>(lo, in + 4 * t);
      fri_load_words<4, true>(hi, in + 2 * h + 4 * t);
#pragma unroll
      for (int j = 0; j < 2; j++)
        F::pack(r + 2 * j, A::fold1(F::unpack(lo + 2 * j), F::unpack(hi + 2 * j), fri_wide_twiddle<PR>(tw, log_max, k, 2 * t + j), c.a0));
      fri_store_words<4, true>(out + 4 * t, r);
    } else {
      constexpr bool V = VEC && EW % 4 == 0;
      uint32_t lo[EW], hi[EW], r[EW];
      fri_load_words<EW, V>(lo, in + EW * t);
      fri_load_words<EW, V>(hi, in + EW * (t + h));
      const fe w = fri_wide_twiddle<PR>(tw, log_max, k, t);
      if constexpr (COEFFS == 1) {
        F::pack(r, A::fold1(F::unpack(lo), F::unpack(hi), w, c.a0));
      } else {
        const fe l2[2] = {F::unpack(lo), F::unpack(lo + W)}, h2[2] = {F::unpack(hi), F::unpack(hi + W)};
        fe o[2];
        A::fold2(l2, h2, w, c.a0, c.a1, c.a1n, o);
        F::pack(r, o[0]), F::pack(r + W, o[1]);
      }
      fri_store_words<EW, V>(out + EW * t, r);
    }
  }

  // the field kind of fri_protocol.hpp: COEFFS = 1 (scalar) or 2 (Goldilocks' quadratic extension)
  template <class PR, int COEFFS>
  struct WideKind {
    using F = FieldOps<PR>;
    using fe = typename F::fe;
    static constexpr int W = F::N32, WORDS = W * COEFFS;
    static_assert(COEFFS == 1 || W == 2, "only Goldilocks has an extension here");

    struct Domain {
      const uint32_t* tw = nullptr;
      int log_max = 0;
    };
    static bool domain_for(uint32_t k, Domain* d) { return ntt_big_domain_table(FriWideField<PR>::INDEX, &d->tw, &d->log_max) && (int)k <= d->log_max; }

    static WideFoldConsts<PR> fold_consts(const uint32_t* alpha)
    {
      WideFoldConsts<PR> c;
      c.a0 = F::from_canonical(alpha);
      c.a1 = c.a1n = F::zero();
      if constexpr (COEFFS == 2) {
        const uint32_t nonres[2] = {PR::EXT_NONRES, 0};
        c.a1 = F::from_canonical(alpha + W);
        c.a1n = F::mul(c.a1, F::from_canonical(nonres));
      }
      return c;
    }

    // d_in: n = 2^k elements, d_out: n / 2, both on the device; d: the domain's table, k <= d.log_max
    static icicle_error_t fold_launch(const uint32_t* d_in, uint32_t* d_out, uint32_t k, const uint32_t* alpha, const Domain& d, hipStream_t st)
    {
      const uint64_t h = ((uint64_t)1 << k) / 2;
      const WideFoldConsts<PR> c = fold_consts(alpha);
      const bool aligned = (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0;
      const bool vec = aligned && (WORDS != 2 || h % 2 == 0);
      const uint64_t lanes = (WORDS == 2 && vec) ? h / 2 : h;
      const unsigned grid = (unsigned)((lanes + 255) / 256);
      if (vec)
        k_fri_fold_wide<PR, COEFFS, true><<<grid, 256, 0, st>>>(d_in, d_out, d.tw, c, h, lanes, k, (uint32_t)d.log_max);
      else
        k_fri_fold_wide<PR, COEFFS, false><<<grid, 256, 0, st>>>(d_in, d_out, d.tw, c, h, lanes, k, (uint32_t)d.log_max);
      LAUNCH_CHECK("k_fri_fold_wide", st);
      return ICICLE_SUCCESS;
    }

    static void from_digest(const uint8_t* digest, size_t len, uint32_t* out)
    {
      if constexpr (COEFFS == 1)
        fri_wide_from_digest(digest, len, PR::P32, W, out);
      else
        fri_gold_ext_from_digest(digest, len, PR::P32, out);
    }
    static bool canonical(const uint32_t* e)
    {
      for (int q = 0; q < COEFFS; q++)
        if (!words_lt_p<PR>(e + q * W)) return false;
      return true;
    }

    struct Collinear { // w_n^(-1) from the field's own root of unity, in the form the field multiplies by
      fe w_inv;
      explicit Collinear(uint32_t log_n)
      {
        fe w = F::from_canonical(PR::ROU32);
        for (int i = 0; i < PR::TWO_ADICITY - (int)log_n; i++)
          w = F::sqr(w);
        w_inv = F::inv(w);
      }
      void fold(const uint32_t* a, const uint32_t* b, const uint32_t* alpha, uint64_t e, uint32_t* out) const
      {
        const fe tw = BigNtt<PR>::pow_u64(w_inv, e); // e = 0: one()
        const WideFoldConsts<PR> c = fold_consts(alpha);
        if constexpr (COEFFS == 1) {
          F::pack(out, FriWideFold<PR>::fold1(F::unpack(a), F::unpack(b), tw, c.a0));
        } else {
          const fe l2[2] = {F::unpack(a), F::unpack(a + W)}, h2[2] = {F::unpack(b), F::unpack(b + W)};
          fe o[2];
          FriWideFold<PR>::fold2(l2, h2, tw, c.a0, c.a1, c.a1n, o);
          F::pack(out, o[0]), F::pack(out + W, o[1]);
        }
      }
    };
  };

  using GoldilocksKind = WideKind<goldilocks_params, 1>;
  using GoldilocksExtensionKind = WideKind<goldilocks_params, 2>;
  using Stark252Kind = WideKind<stark252_fr_params, 1>;
  using Bn254Kind = WideKind<bn254_fr_params, 1>;
  using Bls12381Kind = WideKind<bls12_381_fr_params, 1>;
  using Bls12377Kind = WideKind<bls12_377_fr_params, 1>;

} // namespace icicle_hip

DEFINE_FRI(goldilocks, icicle_hip::GoldilocksKind)
DEFINE_FRI(goldilocks_extension, icicle_hip::GoldilocksExtensionKind)
DEFINE_FRI(stark252, icicle_hip::Stark252Kind)
DEFINE_FRI(bn254, icicle_hip::Bn254Kind)
DEFINE_FRI(bls12_381, icicle_hip::Bls12381Kind)
DEFINE_FRI(bls12_377, icicle_hip::Bls12377Kind)
