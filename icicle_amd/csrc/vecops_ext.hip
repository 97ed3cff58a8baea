// Extension-field vector operations for the three fields that have an extension type: babybear and koalabear (quartic) and
// goldilocks (quadratic). <F>_extension_vector_add / _sub / _mul / _div / _mixed_mul / _inv / _sum / _product and
// <F>_extension_scalar_add_vec / _sub_vec / _mul_vec; <F>_extension_bit_reverse is the 4-word instance of vecops_arith.hip's kernel.
//
// Reference semantics: icicle/src/vec_ops.cpp:24-64 (extension_vector_product / _sum), :87-97 (_add), :152-162 (_sub), :185-210
// (_mul, _mixed_mul), :233-243 (_div), :265-274 (_inv), :297-315 (scalar_add), :338-356 (scalar_sub), :378-396 (scalar_mul), :455-464
// (bit_reverse), over the element layout of vecops_ext_elem.hpp. They behave as the base-field functions of vecops_arith.hip and
// vecops_inv.hip do, over 16-byte elements.
//
// Element-wise kernels: one lane per element, one 16-byte access per operand where every device pointer is 16-byte aligned (VEC),
// word by word otherwise. Inversion: a lane computes the norm of each of its K elements in the base field and the numerator
// conj_times(a); the norms of a tile of 64 K elements share one base-field a^(p-2) chain exactly as vecops_inv.hip's elements do
// (Montgomery's trick over the wave), and each numerator is multiplied by the inverse of its norm. Sum and product are the shared
// two-launch reduction of vecops_tile.hpp with partials of extension elements.
#include "vecops_tile.hpp"
#include "vecops_ext_elem.hpp"

namespace icicle_hip {

  template <class EL>
  struct ExtBase; // the base-field element of vecops_elem.hpp under an extension element, and how a representative becomes one
  template <class PR>
  struct ExtBase<SmallExtElem<PR>> {
    using BE = SmallElem<PR>;
    static __device__ __forceinline__ typename BE::T wrap(uint32_t v) { return typename BE::T{v}; }
    static __device__ __forceinline__ uint32_t unwrap(const typename BE::T& x) { return x.v; }
  };
  template <>
  struct ExtBase<GoldExtElem> {
    using BE = GoldElem;
    static __device__ __forceinline__ GoldFe wrap(const GoldFe& v) { return v; }
    static __device__ __forceinline__ GoldFe unwrap(const GoldFe& x) { return x; }
  };

  // Elements per lane of an extension inversion tile: the numerator (four words), the norm and the running product of each stay in
  // registers, 6 K or 8 K VGPRs, so K is half the base fields'
  template <class EL>
  struct ExtInvTile {
    static constexpr int K = 8;
  };

  template <class EL, bool VEC>
  __device__ __forceinline__ typename EL::T ext_load(const uint32_t* p)
  {
    uint32_t w[4];
    if constexpr (VEC) {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
      w[0] = p[0], w[1] = p[1], w[2] = p[2], w[3] = p[3];
    }
    return EL::load(w);
  }
  template <class EL, bool VEC>
  __device__ __forceinline__ void ext_store(uint32_t* p, const typename EL::T& x)
  {
    uint32_t w[4];
    EL::store(w, x);
    if constexpr (VEC)
      *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    else
      p[0] = w[0], p[1] = w[1], p[2] = w[2], p[3] = w[3];
  }
  template <class EL, bool VEC>
  __device__ __forceinline__ typename EL::BT base_load(const uint32_t* p)
  {
    if constexpr (VEC && EL::BW == 2) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      const uint32_t w[2] = {v.x, v.y};
      return EL::load_base(w);
    } else {
      return EL::load_base(p);
    }
  }

  // the element interface of the shared reduction with 16-byte accesses
  template <class EL>
  struct Vec16 : EL {
    static __device__ __forceinline__ typename EL::T load(const uint32_t* p) { return ext_load<EL, true>(p); }
    static __device__ __forceinline__ void store(uint32_t* p, const typename EL::T& x) { ext_store<EL, true>(p, x); }
  };

  // out[i] = a[ai(i)] op b[i]; a_scalar: a holds one scalar per batch entry. out may be a or b.
  template <class EL, bool VEC>
  __global__ __launch_bounds__(256) void k_ext_vec2(const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t total, int op, bool a_scalar, uint64_t size, uint32_t batch, bool columns)
  {
    uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
      const uint64_t ai = !a_scalar ? i : (columns ? i % batch : i / size);
      const typename EL::T x = ext_load<EL, VEC>(a + ai * 4), y = ext_load<EL, VEC>(b + i * 4);
      ext_store<EL, VEC>(out + i * 4, EL::apply(op, x, y));
    }
  }

  // out[i] = a[i] (extension) * b[i] (base field)
  template <class EL, bool VEC>
  __global__ __launch_bounds__(256) void k_ext_mixed_mul(const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t total)
  {
    uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
      const typename EL::T x = ext_load<EL, VEC>(a + i * 4);
      const typename EL::BT y = base_load<EL, VEC>(b + i * EL::BW);
      ext_store<EL, VEC>(out + i * 4, EL::apply_mixed(x, y));
    }
  }

  // out[i] = 1 / den[i] (DIV: num[i] / den[i]), 0 where den[i] = 0. Lane l of a wave holds elements tile * 64 K + j * 64 + l, j < K,
  // as in k_vec_inv. num, den and out may be the same vector: a lane reads what it needs of an element before it writes that element.
  template <class EL, bool DIV, bool VEC>
  __global__ __launch_bounds__(256) void k_ext_inv(const uint32_t* num, const uint32_t* den, uint32_t* out, uint64_t total, uint64_t tiles)
  {
    using T = typename EL::T;
    using XB = ExtBase<EL>;
    using BE = typename XB::BE;
    using BT = typename BE::T;
    constexpr int K = ExtInvTile<EL>::K;
    const int lane = threadIdx.x & 63;
    for (uint64_t tile = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < tiles; tile += (uint64_t)gridDim.x * 4) {
      const uint64_t base = tile * (64 * K) + lane;
      T c[K];            // conj_times of each element
      BT x[K], pre[K];   // its norm; pre[j] = x[0] ... x[j-1]
      uint32_t masked = 0; // zeros and positions past the end: one in the chain
      BT run = BE::one();
#pragma unroll
      for (int j = 0; j < K; j++) {
        const uint64_t i = base + (uint64_t)j * 64;
        T d = EL::zero();
        if (i < total) d = ext_load<EL, VEC>(den + i * 4);
        const bool skip = EL::is_zero(d); // the norm of anything else is not zero
        const BT n = XB::wrap(EL::norm_conj(d, c[j]));
        x[j] = pick(skip, BE::one(), n);
        masked |= (skip ? 1u : 0u) << j;
        pre[j] = run;
        if (j == 0)
          run = x[j];
        else
          run = BE::mul_raw(run, x[j]);
      }
      // across the wave: the products of the lane totals before and after this lane, and the product of all
      BT incl = run, suff = run;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const BT lo = wave_read(incl, (lane - off) & 63), hi = wave_read(suff, (lane + off) & 63);
        const BT a = BE::mul_raw(incl, lo), b = BE::mul_raw(suff, hi);
        incl = pick(lane >= off, a, incl);
        suff = pick(lane + off < 64, b, suff);
      }
      const BT before = wave_read(incl, (lane - 1) & 63), after = wave_read(suff, (lane + 1) & 63);
      // one base-field inversion per tile, R^2 / x: a quotient takes one R back in its product with the numerator
      BT r = BE::unscale(wave_inv_raw<BE>(wave_read(incl, 63), lane));
      if (!DIV) r = BE::unscale(r);
      const BT rb = BE::mul_raw(r, before);
      r = pick(lane > 0, rb, r);
      const BT ra = BE::mul_raw(r, after);
      r = pick(lane < 63, ra, r);
      // r = 1 / (this lane's total): peel the norms off backwards
#pragma unroll
      for (int j = K - 1; j >= 0; j--) {
        const uint64_t i = base + (uint64_t)j * 64;
        BT q = r;
        if (j > 0) {
          q = BE::mul_raw(r, pre[j]);
          r = BE::mul_raw(r, x[j]);
        }
        if (i < total) {
          T o = EL::mul_base_raw(c[j], XB::unwrap(q));
          if (DIV) o = EL::mul_raw(o, ext_load<EL, VEC>(num + i * 4));
          ext_store<EL, VEC>(out + i * 4, pick((masked >> j) & 1, EL::zero(), o));
        }
      }
    }
  }

  static inline bool aligned16(const void* p, bool on_device) { return !on_device || ((uintptr_t)p & 15) == 0; } // staging buffers are aligned

  template <class EL, bool MIXED>
  static icicle_error_t ext_vec2_run(const void* a, const void* b, uint64_t size, const icicle_vec_ops_config_t* cfg, void* out, int op, bool a_scalar)
  {
    if (!cfg) return ICICLE_INVALID_POINTER;
    if (size == 0) return ICICLE_SUCCESS;
    if (!a || !b || !out) return ICICLE_INVALID_POINTER;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const uint32_t batch = (uint32_t)std::max(1, cfg->batch_size);
    const uint64_t total = size * batch;
    const size_t bytes = (size_t)total * 16;
    Staged sa, sb;
    ICICLE_TRY(sa.in(a, cfg->is_a_on_device, a_scalar ? (size_t)batch * 16 : bytes, st));
    ICICLE_TRY(sb.in(b, cfg->is_b_on_device, MIXED ? (size_t)total * EL::BW * 4 : bytes, st));
    TempBuf d_out_tmp;
    uint32_t* d_out = (uint32_t*)out;
    if (!cfg->is_result_on_device) {
      HIP_TRY(d_out_tmp.alloc(bytes, st), ICICLE_ALLOCATION_FAILED);
      d_out = d_out_tmp.as<uint32_t>();
    }
    const bool b_ok = MIXED ? (!cfg->is_b_on_device || ((uintptr_t)b & (EL::BW * 4 - 1)) == 0) : aligned16(b, cfg->is_b_on_device);
    const bool vec = aligned16(a, cfg->is_a_on_device) && b_ok && aligned16(out, cfg->is_result_on_device);
    const unsigned grid = (unsigned)std::min<uint64_t>((total + 255) / 256, 1u << 20);
    if (MIXED) {
      if (vec)
        k_ext_mixed_mul<EL, true><<<grid, 256, 0, st>>>(sa.dev, sb.dev, d_out, total);
      else
        k_ext_mixed_mul<EL, false><<<grid, 256, 0, st>>>(sa.dev, sb.dev, d_out, total);
      LAUNCH_CHECK("k_ext_mixed_mul", st);
    } else {
      if (vec)
        k_ext_vec2<EL, true><<<grid, 256, 0, st>>>(sa.dev, sb.dev, d_out, total, op, a_scalar, size, batch, cfg->columns_batch);
      else
        k_ext_vec2<EL, false><<<grid, 256, 0, st>>>(sa.dev, sb.dev, d_out, total, op, a_scalar, size, batch, cfg->columns_batch);
      LAUNCH_CHECK("k_ext_vec2", st);
    }
    return finish_out(out, d_out, cfg->is_result_on_device, cfg->is_async, bytes, st);
  }

  template <class EL, bool DIV>
  static icicle_error_t ext_inv_run(const void* a, const void* b, uint64_t size, const icicle_vec_ops_config_t* cfg, void* out)
  {
    if (!cfg) return ICICLE_INVALID_POINTER;
    if (size == 0) return ICICLE_SUCCESS;
    if (!a || (DIV && !b) || !out) return ICICLE_INVALID_POINTER;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const uint32_t batch = (uint32_t)std::max(1, cfg->batch_size);
    const uint64_t total = size * batch;
    const size_t bytes = (size_t)total * 16;
    Staged sa, sb;
    ICICLE_TRY(sa.in(a, cfg->is_a_on_device, bytes, st));
    if (DIV) ICICLE_TRY(sb.in(b, cfg->is_b_on_device, bytes, st));
    TempBuf d_out_tmp;
    uint32_t* d_out = (uint32_t*)out;
    if (!cfg->is_result_on_device) {
      HIP_TRY(d_out_tmp.alloc(bytes, st), ICICLE_ALLOCATION_FAILED);
      d_out = d_out_tmp.as<uint32_t>();
    }
    const bool vec = aligned16(a, cfg->is_a_on_device) && (!DIV || aligned16(b, cfg->is_b_on_device)) && aligned16(out, cfg->is_result_on_device);
    constexpr uint64_t TILE = 64 * ExtInvTile<EL>::K;
    const uint64_t tiles = (total + TILE - 1) / TILE;
    const unsigned grid = (unsigned)std::min<uint64_t>((tiles + 3) / 4, INV_MAX_GRID);
    const uint32_t* d_den = DIV ? sb.dev : sa.dev;
    if (vec)
      k_ext_inv<EL, DIV, true><<<grid, 256, 0, st>>>(sa.dev, d_den, d_out, total, tiles);
    else
      k_ext_inv<EL, DIV, false><<<grid, 256, 0, st>>>(sa.dev, d_den, d_out, total, tiles);
    LAUNCH_CHECK("k_ext_inv", st);
    return finish_out(out, d_out, cfg->is_result_on_device, cfg->is_async, bytes, st);
  }

  template <class EL, int OP>
  static icicle_error_t ext_reduce_run(const void* a, uint64_t size, const icicle_vec_ops_config_t* cfg, void* out)
  {
    if (cfg && aligned16(a, cfg->is_a_on_device) && aligned16(out, cfg->is_result_on_device)) return reduce_run<Vec16<EL>, OP>(a, size, cfg, out);
    return reduce_run<EL, OP>(a, size, cfg, out);
  }

} // namespace icicle_hip

using namespace icicle_hip;

#define GUARDED(expr)                                                                                                  \
  try {                                                                                                                \
    return (expr);                                                                                                     \
  } catch (...) {                                                                                                      \
    return ICICLE_INVALID_ARGUMENT;                                                                                    \
  }

#define EXT_ARGS2 const void* a, const void* b, uint64_t n, const icicle_vec_ops_config_t* c, void* o
#define EXT_ARGS1 const void* a, uint64_t n, const icicle_vec_ops_config_t* c, void* o
#define DEFINE_VEC_EXT(NAME, EL)                                                                                       \
  extern "C" icicle_error_t NAME##_extension_vector_add(EXT_ARGS2) { GUARDED((ext_vec2_run<EL, false>(a, b, n, c, o, XOP_ADD, false))); } \
  extern "C" icicle_error_t NAME##_extension_vector_sub(EXT_ARGS2) { GUARDED((ext_vec2_run<EL, false>(a, b, n, c, o, XOP_SUB, false))); } \
  extern "C" icicle_error_t NAME##_extension_vector_mul(EXT_ARGS2) { GUARDED((ext_vec2_run<EL, false>(a, b, n, c, o, XOP_MUL, false))); } \
  extern "C" icicle_error_t NAME##_extension_vector_mixed_mul(EXT_ARGS2) { GUARDED((ext_vec2_run<EL, true>(a, b, n, c, o, XOP_MUL, false))); } \
  extern "C" icicle_error_t NAME##_extension_scalar_add_vec(EXT_ARGS2) { GUARDED((ext_vec2_run<EL, false>(a, b, n, c, o, XOP_ADD, true))); } \
  extern "C" icicle_error_t NAME##_extension_scalar_sub_vec(EXT_ARGS2) { GUARDED((ext_vec2_run<EL, false>(a, b, n, c, o, XOP_SUB, true))); } \
  extern "C" icicle_error_t NAME##_extension_scalar_mul_vec(EXT_ARGS2) { GUARDED((ext_vec2_run<EL, false>(a, b, n, c, o, XOP_MUL, true))); } \
  extern "C" icicle_error_t NAME##_extension_vector_div(EXT_ARGS2) { GUARDED((ext_inv_run<EL, true>(a, b, n, c, o))); } \
  extern "C" icicle_error_t NAME##_extension_vector_inv(EXT_ARGS1) { GUARDED((ext_inv_run<EL, false>(a, nullptr, n, c, o))); } \
  extern "C" icicle_error_t NAME##_extension_vector_sum(EXT_ARGS1) { GUARDED((ext_reduce_run<EL, RED_SUM>(a, n, c, o))); } \
  extern "C" icicle_error_t NAME##_extension_vector_product(EXT_ARGS1) { GUARDED((ext_reduce_run<EL, RED_PRODUCT>(a, n, c, o))); }

DEFINE_VEC_EXT(babybear, SmallExtElem<babybear_params>)
DEFINE_VEC_EXT(koalabear, SmallExtElem<koalabear_params>)
DEFINE_VEC_EXT(goldilocks, GoldExtElem)

extern "C" int icicle_hip_extension_vector_inv_tile(int base_words_per_element)
{
  switch (base_words_per_element) {
  case 1: return 64 * ExtInvTile<SmallExtElem<babybear_params>>::K;
  case 2: return 64 * ExtInvTile<GoldExtElem>::K;
  default: return 0;
  }
}
