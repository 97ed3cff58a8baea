// Extension-field vector operations for the three fields that have an extension type: babybear and koalabear (quartic) and
// goldilocks (quadratic). <F>_extension_vector_add / _sub / _mul / _div / _mixed_mul / _inv / _sum / _product and
// <F>_extension_scalar_add_vec / _sub_vec / _mul_vec; <F>_extension_bit_reverse is the 4-word instance of vecops_arith.hip's kernel.
//
// Reference semantics: icicle/src/vec_ops.cpp:24-64 (extension_vector_product / _sum), :87-97 (_add), :152-162 (_sub), :185-210
// (_mul, _mixed_mul), :233-243 (_div), :265-274 (_inv), :297-315 (scalar_add), :338-356 (scalar_sub), :378-396 (scalar_mul), :455-464
// (bit_reverse), over the element layout of vecops_ext_elem.hpp. They behave as the base-field functions of vecops_arith.hip and
// vecops_inv.hip do, over 16-byte elements, and they are the same kernels (vecops_tile.hpp) over the extension elements: one lane per
// element, one 16-byte access per operand where every device pointer is 16-byte aligned (Vec16<>), word by word otherwise.
// Inversion: a lane computes the norm of each of its K elements in the base field and the numerator conj_times(a); the norms of a tile
// of 64 K elements share one base-field a^(p-2) chain (Montgomery's trick over the wave), and each numerator is multiplied by the
// inverse of its norm: InvTile<> below. Only mixed_mul, whose operands differ in type, has a kernel of its own here.
#include "vecops_tile.hpp"
#include "vecops_ext_elem.hpp"

namespace icicle_hip {

  // The inversion tile of an extension element chains its norm, a base-field element of vecops_elem.hpp, and keeps conj_times beside it.
  // The numerator (four words), the norm and the running product of each element stay in registers, 6 K or 8 K VGPRs, so K is half the
  // base fields'.
  template <class PR>
  struct InvTile<SmallExtElem<PR>> {
    using EL = SmallExtElem<PR>;
    using CE = SmallElem<PR>;
    using Num = typename EL::T;
    static constexpr int K = 8;
    static constexpr bool KEEP = true;
    static __device__ __forceinline__ typename CE::T chain(const Num& d, Num& num) { return typename CE::T{EL::norm_conj(d, num)}; }
    static __device__ __forceinline__ Num join(const typename CE::T& q, const Num& num) { return EL::mul_base_raw(num, q.v); }
  };
  template <>
  struct InvTile<GoldExtElem> {
    using CE = GoldElem;
    using Num = GoldExt;
    static constexpr int K = 8;
    static constexpr bool KEEP = true;
    static __device__ __forceinline__ GoldFe chain(const Num& d, Num& num) { return GoldExtElem::norm_conj(d, num); }
    static __device__ __forceinline__ Num join(const GoldFe& q, const Num& num) { return GoldExtElem::mul_base_raw(num, q); }
  };

  // out[i] = a[i] (extension) * b[i] (base field); out may be a (the contract stated at k_vec2)
  template <class EL>
  __global__ __launch_bounds__(256) void k_ext_mixed_mul(const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t total)
  {
    uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
      const typename EL::T x = EL::load(a + i * 4);
      const typename EL::BT y = EL::load_base(b + i * EL::BW);
      EL::store(out + i * 4, EL::apply_mixed(x, y));
    }
  }

  template <class EL>
  static icicle_error_t ext_mixed_mul_run(const void* a, const void* b, uint64_t size, const icicle_vec_ops_config_t* cfg, void* out)
  {
    if (!cfg) return ICICLE_INVALID_POINTER;
    if (size == 0) return ICICLE_SUCCESS;
    if (!a || !b || !out) return ICICLE_INVALID_POINTER;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const uint64_t total = size * (uint32_t)std::max(1, cfg->batch_size);
    const size_t bytes = (size_t)total * 16;
    Staged sa, sb;
    StagedOut so;
    ICICLE_TRY(sa.in(a, cfg->is_a_on_device, bytes, st));
    ICICLE_TRY(sb.in(b, cfg->is_b_on_device, (size_t)total * EL::BW * 4, st));
    ICICLE_TRY(so.out(out, cfg->is_result_on_device, bytes, st));
    const bool b_ok = !cfg->is_b_on_device || ((uintptr_t)b & (EL::BW * 4 - 1)) == 0;
    const unsigned grid = (unsigned)std::min<uint64_t>((total + 255) / 256, 1u << 20);
    if (aligned16(a, cfg->is_a_on_device) && b_ok && aligned16(out, cfg->is_result_on_device))
      k_ext_mixed_mul<Vec16<EL>><<<grid, 256, 0, st>>>(sa.dev, sb.dev, so.dev, total);
    else
      k_ext_mixed_mul<EL><<<grid, 256, 0, st>>>(sa.dev, sb.dev, so.dev, total);
    LAUNCH_CHECK("k_ext_mixed_mul", st);
    return so.finish(cfg->is_async);
  }

  template <class EL, int OP>
  static icicle_error_t ext_reduce_run(const void* a, uint64_t size, const icicle_vec_ops_config_t* cfg, void* out)
  {
    if (cfg && aligned16(a, cfg->is_a_on_device) && aligned16(out, cfg->is_result_on_device)) return reduce_run<Vec16<EL>, OP>(a, size, cfg, out);
    return reduce_run<EL, OP>(a, size, cfg, out);
  }

} // namespace icicle_hip

using namespace icicle_hip;

#define EXT_ARGS2 const void* a, const void* b, uint64_t n, const icicle_vec_ops_config_t* c, void* o
#define EXT_ARGS1 const void* a, uint64_t n, const icicle_vec_ops_config_t* c, void* o
#define DEFINE_VEC_EXT(NAME, EL)                                                                                       \
  extern "C" icicle_error_t NAME##_extension_vector_add(EXT_ARGS2) { GUARDED((vec2_run<EL>(a, b, n, c, o, VOP_ADD, false))); } \
  extern "C" icicle_error_t NAME##_extension_vector_sub(EXT_ARGS2) { GUARDED((vec2_run<EL>(a, b, n, c, o, VOP_SUB, false))); } \
  extern "C" icicle_error_t NAME##_extension_vector_mul(EXT_ARGS2) { GUARDED((vec2_run<EL>(a, b, n, c, o, VOP_MUL, false))); } \
  extern "C" icicle_error_t NAME##_extension_vector_mixed_mul(EXT_ARGS2) { GUARDED((ext_mixed_mul_run<EL>(a, b, n, c, o))); } \
  extern "C" icicle_error_t NAME##_extension_scalar_add_vec(EXT_ARGS2) { GUARDED((vec2_run<EL>(a, b, n, c, o, VOP_ADD, true))); } \
  extern "C" icicle_error_t NAME##_extension_scalar_sub_vec(EXT_ARGS2) { GUARDED((vec2_run<EL>(a, b, n, c, o, VOP_SUB, true))); } \
  extern "C" icicle_error_t NAME##_extension_scalar_mul_vec(EXT_ARGS2) { GUARDED((vec2_run<EL>(a, b, n, c, o, VOP_MUL, true))); } \
  extern "C" icicle_error_t NAME##_extension_vector_div(EXT_ARGS2) { GUARDED((inv_run<EL, true>(a, b, n, c, o))); }    \
  extern "C" icicle_error_t NAME##_extension_vector_inv(EXT_ARGS1) { GUARDED((inv_run<EL, false>(a, nullptr, n, c, o))); } \
  extern "C" icicle_error_t NAME##_extension_vector_sum(EXT_ARGS1) { GUARDED((ext_reduce_run<EL, RED_SUM>(a, n, c, o))); } \
  extern "C" icicle_error_t NAME##_extension_vector_product(EXT_ARGS1) { GUARDED((ext_reduce_run<EL, RED_PRODUCT>(a, n, c, o))); }

DEFINE_VEC_EXT(babybear, SmallExtElem<babybear_params>)
DEFINE_VEC_EXT(koalabear, SmallExtElem<koalabear_params>)
DEFINE_VEC_EXT(goldilocks, GoldExtElem)

extern "C" int icicle_hip_extension_vector_inv_tile(int base_words_per_element)
{
  switch (base_words_per_element) {
  case 1: return 64 * InvTile<SmallExtElem<babybear_params>>::K;
  case 2: return 64 * InvTile<GoldExtElem>::K;
  default: return 0;
  }
}
