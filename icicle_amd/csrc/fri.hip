// FRI over the 31-bit fields (BabyBear, KoalaBear), scalar and quartic extension: the fold kernel and the field kind that
// fri_protocol.hpp's prover and verifier (the reference's C ABI, src/fri/fri_c_api.cpp) are instantiated with. The wider fields
// are in fri_wide.hip.
//
// The fold: out[i] = (e[i] + e[i+h])/2 + alpha * ((e[i] - e[i+h])/2 * w_n^(-i)), h = n/2. Memory-bound: n elements in, n/2 out and
// n/2 twiddles gathered from the NTT domain's table with stride max/n. Elements are canonical in memory; alpha, alpha * W and the
// twiddles are in Montgomery form, and montmul(canonical, x*R) is canonical, so no conversion pass is needed; halving is a shift. A
// lane moves 16 bytes per access: one extension element, or four consecutive scalars from each half.
#include "common.h"
#include "smallfield.hpp"
#include "fri_protocol.hpp"

namespace icicle_hip {

  // FriField<PR> (the field's index in ntt_domain_table, and W of the extension F[x] / (x^4 - W)) is in smallfield.hpp, which the
  // extension vector operations share

  // alpha for the kernel, Montgomery form: a[k] = alpha_k, aw[k] = W * alpha_k (scalar: a[0] only)
  struct FoldConsts {
    uint32_t a[4], aw[4];
  };

  // x / 2 for a canonical x without a product: x + p is even when x is odd, and below 2^32
  template <class PR>
  SF_HD uint32_t fri_half(uint32_t x)
  {
    return (x + ((x & 1) ? PR::P : 0u)) >> 1;
  }

  template <class PR>
  SF_HD uint32_t fri_dot2(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
  { // x0 y0 + x1 y1 in one reduction: 2 p^2 < p 2^32
    return SmallField<PR>::mont_reduce((uint64_t)x0 * y0 + (uint64_t)x1 * y1);
  }

  // one scalar fold; tw = w_n^(-i), Montgomery
  template <class PR>
  SF_HD uint32_t fri_fold1(uint32_t lo, uint32_t hi, uint32_t tw, const FoldConsts& c)
  {
    using S = SmallField<PR>;
    const uint32_t even = fri_half<PR>(S::add(lo, hi));
    const uint32_t odd = S::mul(fri_half<PR>(S::sub(lo, hi)), tw);
    return S::add(even, S::mul(odd, c.a[0]));
  }

  // one extension fold: lo, hi, out = 4 coefficients, constant term first
  template <class PR>
  SF_HD void fri_fold4(const uint32_t* lo, const uint32_t* hi, uint32_t tw, const FoldConsts& c, uint32_t* out)
  {
    using S = SmallField<PR>;
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
      o[k] = S::mul(fri_half<PR>(S::sub(lo[k], hi[k])), tw);
    // (alpha * odd)_k = sum_{i <= k} o_i a_{k-i} + W sum_{i > k} o_i a_{k+4-i}
    const uint32_t r0 = S::add(fri_dot2<PR>(o[0], c.a[0], o[1], c.aw[3]), fri_dot2<PR>(o[2], c.aw[2], o[3], c.aw[1]));
    const uint32_t r1 = S::add(fri_dot2<PR>(o[0], c.a[1], o[1], c.a[0]), fri_dot2<PR>(o[2], c.aw[3], o[3], c.aw[2]));
    const uint32_t r2 = S::add(fri_dot2<PR>(o[0], c.a[2], o[1], c.a[1]), fri_dot2<PR>(o[2], c.a[0], o[3], c.aw[3]));
    const uint32_t r3 = S::add(fri_dot2<PR>(o[0], c.a[3], o[1], c.a[2]), fri_dot2<PR>(o[2], c.a[1], o[3], c.a[0]));
    out[0] = S::add(fri_half<PR>(S::add(lo[0], hi[0])), r0);
    out[1] = S::add(fri_half<PR>(S::add(lo[1], hi[1])), r1);
    out[2] = S::add(fri_half<PR>(S::add(lo[2], hi[2])), r2);
    out[3] = S::add(fri_half<PR>(S::add(lo[3], hi[3])), r3);
  }

  // tw[(max - (max >> k) i) & (max - 1)] = w_n^(-i) for n = 2^k (the reference's tw_idx; i = 0 wraps to tw[0] = 1)
  __device__ __forceinline__ uint32_t fri_twiddle(const uint32_t* __restrict__ tw, uint32_t log_max, uint32_t k, uint64_t i)
  {
    const uint64_t max = (uint64_t)1 << log_max;
    return tw[(max - ((max >> k) * i)) & (max - 1)];
  }

  // WORDS = 1: scalars, VEC ? four consecutive i per lane (h % 4 == 0, 16-byte aligned pointers) : one i per lane.
  // WORDS = 4: one extension element per lane, VEC ? as one 16-byte access : word by word (unaligned pointers).
  // `lanes` = h / 4 (WORDS = 1, VEC) or h.
  template <class PR, int WORDS, bool VEC>
  __global__ __launch_bounds__(256) void k_fri_fold(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, const uint32_t* __restrict__ tw, FoldConsts c, uint64_t h,
                                                    uint64_t lanes, uint32_t k, uint32_t log_max)
  {
    const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (t >= lanes) return;
    if constexpr (WORDS == 1 && VEC) {
      const uint4 lo = reinterpret_cast<const uint4*>(in)[t], hi = reinterpret_cast<const uint4*>(in + h)[t];
      const uint64_t i = 4 * t;
      uint4 r;
      r.x = fri_fold1<PR>(lo.x, hi.x, fri_twiddle(tw, log_max, k, i), c);
      r.y = fri_fold1<PR>(lo.y, hi.y, fri_twiddle(tw, log_max, k, i + 1), c);
      r.z = fri_fold1<PR>(lo.z, hi.z, fri_twiddle(tw, log_max, k, i + 2), c);
      r.w = fri_fold1<PR>(lo.w, hi.w, fri_twiddle(tw, log_max, k, i + 3), c);
      reinterpret_cast<uint4*>(out)[t] = r;
    } else if constexpr (WORDS == 1) {
      out[t] = fri_fold1<PR>(in[t], in[t + h], fri_twiddle(tw, log_max, k, t), c);
    } else {
      uint32_t lo[4], hi[4], r[4];
      if constexpr (VEC) {
        const uint4 a = reinterpret_cast<const uint4*>(in)[t], b = reinterpret_cast<const uint4*>(in)[t + h];
        lo[0] = a.x, lo[1] = a.y, lo[2] = a.z, lo[3] = a.w;
        hi[0] = b.x, hi[1] = b.y, hi[2] = b.z, hi[3] = b.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++)
          lo[q] = in[4 * t + q], hi[q] = in[4 * (t + h) + q];
      }
      fri_fold4<PR>(lo, hi, fri_twiddle(tw, log_max, k, t), c, r);
      if constexpr (VEC) {
        reinterpret_cast<uint4*>(out)[t] = make_uint4(r[0], r[1], r[2], r[3]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; q++)
          out[4 * t + q] = r[q];
      }
    }
  }

  template <class PR, int WORDS>
  static FoldConsts fold_consts(const uint32_t* alpha)
  {
    using S = SmallField<PR>;
    FoldConsts c{};
    const uint32_t w = S::to_mont(FriField<PR>::W);
    for (int q = 0; q < WORDS; q++) {
      c.a[q] = S::to_mont(alpha[q]);
      c.aw[q] = S::mul(c.a[q], w);
    }
    return c;
  }

  // d_in: n = 2^k elements, d_out: n / 2, both on the device; tw / log_max: the domain's table, k <= log_max
  template <class PR, int WORDS>
  static icicle_error_t fold_launch(const uint32_t* d_in, uint32_t* d_out, uint32_t k, const uint32_t* alpha, const uint32_t* tw, int log_max, hipStream_t st)
  {
    const uint64_t h = ((uint64_t)1 << k) / 2;
    const FoldConsts c = fold_consts<PR, WORDS>(alpha);
    const bool aligned = (((uintptr_t)d_in | (uintptr_t)d_out) & 15) == 0;
    const bool vec = aligned && (WORDS == 4 || h % 4 == 0);
    const uint64_t lanes = (WORDS == 1 && vec) ? h / 4 : h;
    const unsigned grid = (unsigned)((lanes + 255) / 256);
    if (vec)
      k_fri_fold<PR, WORDS, true><<<grid, 256, 0, st>>>(d_in, d_out, tw, c, h, lanes, k, (uint32_t)log_max);
    else
      k_fri_fold<PR, WORDS, false><<<grid, 256, 0, st>>>(d_in, d_out, tw, c, h, lanes, k, (uint32_t)log_max);
    LAUNCH_CHECK("k_fri_fold", st);
    return ICICLE_SUCCESS;
  }

  // a * b in F (canonical words in and out), host side of the verifier
  template <class PR, int WORDS>
  static void field_mul(const uint32_t* a, const uint32_t* b, uint32_t* out)
  {
    using S = SmallField<PR>;
    uint32_t bm[4], r[4] = {0, 0, 0, 0};
    for (int q = 0; q < WORDS; q++)
      bm[q] = S::to_mont(b[q]);
    const uint32_t w = S::to_mont(FriField<PR>::W);
    for (int i = 0; i < WORDS; i++)
      for (int j = 0; j < WORDS; j++) {
        uint32_t t = S::mul(a[i], bm[j]);
        if (i + j >= WORDS) t = S::mul(t, w);
        r[(i + j) % WORDS] = S::add(r[(i + j) % WORDS], t);
      }
    std::memcpy(out, r, WORDS * 4);
  }

  // the field kind of fri_protocol.hpp: WORDS_ = 1 (scalar) or 4 (quartic extension)
  template <class PR, int WORDS_>
  struct SmallKind {
    using S = SmallField<PR>;
    static constexpr int WORDS = WORDS_;
    struct Domain {
      const uint32_t* tw = nullptr;
      int log_max = 0;
    };
    static bool domain_for(uint32_t k, Domain* d) { return ntt_domain_table(FriField<PR>::INDEX, &d->tw, &d->log_max) && (int)k <= d->log_max; }
    static icicle_error_t fold_launch(const uint32_t* d_in, uint32_t* d_out, uint32_t k, const uint32_t* alpha, const Domain& d, hipStream_t st)
    {
      return icicle_hip::fold_launch<PR, WORDS>(d_in, d_out, k, alpha, d.tw, d.log_max, st);
    }
    static void from_digest(const uint8_t* digest, size_t len, uint32_t* out) { fri_field_from_digest(digest, len, PR::P, WORDS, out); }
    static bool canonical(const uint32_t* e)
    {
      for (int q = 0; q < WORDS; q++)
        if (e[q] >= PR::P) return false;
      return true;
    }
    struct Collinear { // w_n^(-1) from the field's own root of unity, 1/2, both Montgomery
      uint32_t w_inv, half;
      explicit Collinear(uint32_t log_n)
      {
        uint32_t w = S::to_mont(PR::ROU);
        for (int i = 0; i < PR::TWO_ADICITY - (int)log_n; i++)
          w = S::mul(w, w);
        w_inv = S::inv(w), half = S::to_mont((PR::P + 1) / 2);
      }
      void fold(const uint32_t* a, const uint32_t* b, const uint32_t* alpha, uint64_t e, uint32_t* out) const
      {
        uint32_t odd[4];
        const uint32_t twh = S::mul(S::pow(w_inv, e), half);
        for (int q = 0; q < WORDS; q++)
          odd[q] = S::mul(S::sub(a[q], b[q]), twh);
        field_mul<PR, WORDS>(odd, alpha, out);
        for (int q = 0; q < WORDS; q++)
          out[q] = S::add(out[q], S::mul(S::add(a[q], b[q]), half));
      }
    };
  };

  using BabybearKind = SmallKind<babybear_params, 1>;
  using BabybearExtensionKind = SmallKind<babybear_params, 4>;
  using KoalabearKind = SmallKind<koalabear_params, 1>;
  using KoalabearExtensionKind = SmallKind<koalabear_params, 4>;

} // namespace icicle_hip

DEFINE_FRI(babybear, icicle_hip::BabybearKind)
DEFINE_FRI(babybear_extension, icicle_hip::BabybearExtensionKind)
DEFINE_FRI(koalabear, icicle_hip::KoalabearKind)
DEFINE_FRI(koalabear_extension, icicle_hip::KoalabearExtensionKind)
