// vector_inv / vector_div / vector_sum / vector_product for the eight fields of vecops_arith.hip.
//
// Reference semantics: icicle/src/vec_ops.cpp:9 (vector_product), :40 (vector_sum), :217 (vector_div), :250 (vector_inv); CPU backend
// icicle/backend/cpu/src/field/cpu_vec_ops.cpp:158-201, 386-503. Elements are canonical words in and out. inv and div are element-wise
// over size * batch_size elements with 1 / 0 = 0; sum and product write one element per batch entry, entry k holding its element j
// at k * size + j, or at j * batch_size + k with columns_batch.
//
// Inversion shares one a^(p-2) chain among the 64 * K elements of a tile (Montgomery's trick), one tile per wave: no LDS, no barrier.
// The reductions go lane -> wave (shuffles) -> block (LDS) -> one partial per block, and a second launch folds the partials of each
// batch entry. The powers of R of the Montgomery fields are settled once per tile or per entry (vecops_elem.hpp).
#include "vecops_tile.hpp" // InvTile, wave_read, pick, wave_inv_raw, Reduce, k_vec_reduce, k_vec_reduce_finish, reduce_run

namespace icicle_hip {

  // out[i] = 1 / den[i] (DIV: num[i] / den[i]), 0 where den[i] = 0. Lane l of a wave holds elements tile * 64 K + j * 64 + l, j < K.
  // num, den and out may be the same vector: a lane reads what it needs of an element before it writes that element.
  template <class EL, bool DIV>
  __global__ __launch_bounds__(256) void k_vec_inv(const uint32_t* num, const uint32_t* den, uint32_t* out, uint64_t total, uint64_t tiles)
  {
    using T = typename EL::T;
    constexpr int K = InvTile<EL>::K;
    constexpr bool KEEP = InvTile<EL>::KEEP;
    const int lane = threadIdx.x & 63;
    for (uint64_t tile = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < tiles; tile += (uint64_t)gridDim.x * 4) {
      const uint64_t base = tile * (64 * K) + lane;
      T x[KEEP ? K : 1], pre[K]; // pre[j] = x[0] ... x[j-1]
      uint32_t masked = 0; // zeros and positions past the end: one in the chain
      T run = EL::one();
#pragma unroll
      for (int j = 0; j < K; j++) {
        const uint64_t i = base + (uint64_t)j * 64;
        T v = EL::one();
        bool skip = true;
        if (i < total) {
          const T d = EL::load(den + i * EL::W);
          if (!EL::is_zero(d)) v = d, skip = false;
        }
        masked |= (skip ? 1u : 0u) << j;
        if (KEEP) x[j] = v;
        pre[j] = run;
        if (j == 0)
          run = v;
        else
          run = EL::mul_raw(run, v);
      }
      // across the wave: the products of the lane totals before and after this lane, and the product of all
      T incl = run, suff = run;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const T lo = wave_read(incl, (lane - off) & 63), hi = wave_read(suff, (lane + off) & 63);
        const T a = EL::mul_raw(incl, lo), b = EL::mul_raw(suff, hi);
        incl = pick(lane >= off, a, incl);
        suff = pick(lane + off < 64, b, suff);
      }
      const T before = wave_read(incl, (lane - 1) & 63), after = wave_read(suff, (lane + 1) & 63);
      // one inversion per tile, R^2 / x: a quotient takes one R back in its product
      T r = EL::unscale(wave_inv_raw<EL>(wave_read(incl, 63), lane));
      if (!DIV) r = EL::unscale(r);
      const T rb = EL::mul_raw(r, before);
      r = pick(lane > 0, rb, r);
      const T ra = EL::mul_raw(r, after);
      r = pick(lane < 63, ra, r);
      // r = 1 / (this lane's total): peel the elements off backwards
#pragma unroll
      for (int j = K - 1; j >= 0; j--) {
        const uint64_t i = base + (uint64_t)j * 64;
        T q = r;
        if (j > 0) q = EL::mul_raw(r, pre[j]);
        if (j > 0) {
          T xj = EL::one();
          if (KEEP)
            xj = x[j];
          else if (!((masked >> j) & 1))
            xj = EL::load(den + i * EL::W);
          r = EL::mul_raw(r, xj);
        }
        if (i < total) {
          if (DIV) q = EL::mul_raw(q, EL::load(num + i * EL::W));
          EL::store(out + i * EL::W, pick((masked >> j) & 1, EL::zero(), q));
        }
      }
    }
  }

  template <class EL, bool DIV>
  static icicle_error_t inv_run(const void* a, const void* b, uint64_t size, const icicle_vec_ops_config_t* cfg, void* out)
  {
    if (!cfg) return ICICLE_INVALID_POINTER;
    if (size == 0) return ICICLE_SUCCESS;
    if (!a || (DIV && !b) || !out) return ICICLE_INVALID_POINTER;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const uint32_t batch = (uint32_t)std::max(1, cfg->batch_size);
    const uint64_t total = size * batch;
    const size_t bytes = (size_t)total * EL::W * 4;
    Staged sa, sb;
    ICICLE_TRY(sa.in(a, cfg->is_a_on_device, bytes, st));
    if (DIV) ICICLE_TRY(sb.in(b, cfg->is_b_on_device, bytes, st));
    TempBuf d_out_tmp;
    uint32_t* d_out = (uint32_t*)out;
    if (!cfg->is_result_on_device) {
      HIP_TRY(d_out_tmp.alloc(bytes, st), ICICLE_ALLOCATION_FAILED);
      d_out = d_out_tmp.as<uint32_t>();
    }
    constexpr uint64_t TILE = 64 * InvTile<EL>::K;
    const uint64_t tiles = (total + TILE - 1) / TILE;
    const unsigned grid = (unsigned)std::min<uint64_t>((tiles + 3) / 4, INV_MAX_GRID);
    k_vec_inv<EL, DIV><<<grid, 256, 0, st>>>(sa.dev, DIV ? sb.dev : sa.dev, d_out, total, tiles);
    LAUNCH_CHECK("k_vec_inv", st);
    return finish_out(out, d_out, cfg->is_result_on_device, cfg->is_async, bytes, st);
  }


} // namespace icicle_hip

using namespace icicle_hip;

#define GUARDED(expr)                                                                                                  \
  try {                                                                                                                \
    return (expr);                                                                                                     \
  } catch (...) {                                                                                                      \
    return ICICLE_INVALID_ARGUMENT;                                                                                    \
  }

#define DEFINE_VEC_INV(NAME, EL)                                                                                       \
  extern "C" icicle_error_t NAME##_vector_inv(const void* a, uint64_t n, const icicle_vec_ops_config_t* c, void* o) { GUARDED((inv_run<EL, false>(a, nullptr, n, c, o))); } \
  extern "C" icicle_error_t NAME##_vector_div(const void* a, const void* b, uint64_t n, const icicle_vec_ops_config_t* c, void* o) { GUARDED((inv_run<EL, true>(a, b, n, c, o))); } \
  extern "C" icicle_error_t NAME##_vector_sum(const void* a, uint64_t n, const icicle_vec_ops_config_t* c, void* o) { GUARDED((reduce_run<EL, RED_SUM>(a, n, c, o))); } \
  extern "C" icicle_error_t NAME##_vector_product(const void* a, uint64_t n, const icicle_vec_ops_config_t* c, void* o) { GUARDED((reduce_run<EL, RED_PRODUCT>(a, n, c, o))); }

DEFINE_VEC_INV(babybear, SmallElem<babybear_params>)
DEFINE_VEC_INV(koalabear, SmallElem<koalabear_params>)
DEFINE_VEC_INV(bn254, BigElem<bn254_fr_params>)
DEFINE_VEC_INV(bls12_381, BigElem<bls12_381_fr_params>)
DEFINE_VEC_INV(bls12_377, BigElem<bls12_377_fr_params>)
DEFINE_VEC_INV(grumpkin, BigElem<bn254_fq_params>)
DEFINE_VEC_INV(stark252, BigElem<stark252_fr_params>)
DEFINE_VEC_INV(goldilocks, GoldElem)

extern "C" int icicle_hip_vector_inv_tile(int words_per_element)
{
  switch (words_per_element) {
  case 1: return 64 * InvTile<SmallElem<babybear_params>>::K;
  case 2: return 64 * InvTile<GoldElem>::K;
  case 8: return 64 * InvTile<BigElem<bn254_fr_params>>::K;
  default: return 0;
  }
}
