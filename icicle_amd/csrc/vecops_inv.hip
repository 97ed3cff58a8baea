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
#include "vecops_elem.hpp"

namespace icicle_hip {

  // Elements per lane of an inversion tile. The K running products of a lane live in registers, and so do its K elements where
  // they are one or two words. At nine limbs that would be 18 K VGPRs, so there only the products are kept (9 K) and the walk back
  // reads each element a second time, from the cache: these fields are bound by their arithmetic, not by memory.
  template <class EL>
  struct InvTile {
    static constexpr int K = 16;
    static constexpr bool KEEP = EL::W < 8;
  };
  constexpr unsigned INV_MAX_GRID = 2048; // blocks of four waves; beyond INV_MAX_GRID * 4 tiles a wave walks on to its next tile

  // the value lane `src` of the wave holds, word by word
  template <class T>
  __device__ __forceinline__ T wave_read(const T& x, int src)
  {
    static_assert(sizeof(T) % 4 == 0, "whole words");
    constexpr int NW = sizeof(T) / 4;
    uint32_t w[NW];
    __builtin_memcpy(w, &x, sizeof(T));
#pragma unroll
    for (int q = 0; q < NW; q++)
      w[q] = (uint32_t)__shfl((int)w[q], src);
    T r;
    __builtin_memcpy(&r, w, sizeof(T));
    return r;
  }

  // c ? a : b word by word (the conditional operator on two structs selects between their addresses, which puts them in scratch)
  template <class T>
  __device__ __forceinline__ T pick(bool c, const T& a, const T& b)
  {
    constexpr int NW = sizeof(T) / 4;
    uint32_t wa[NW], wb[NW];
    __builtin_memcpy(wa, &a, sizeof(T));
    __builtin_memcpy(wb, &b, sizeof(T));
#pragma unroll
    for (int q = 0; q < NW; q++)
      wa[q] = c ? wa[q] : wb[q];
    T r;
    __builtin_memcpy(&r, wa, sizeof(T));
    return r;
  }

  // R^2 / x = x^(p-2) on representatives, for an x that every lane of the wave holds. Where the chain is long (256-bit fields) the wave
  // shares it: all lanes square along, x^(2^t) for t < NBITS, lane l keeps the powers t = l, l + 64, l + 128, l + 192 on the way,
  // multiplies those of them whose bit of p - 2 is set, and the 64 factors are multiplied across the wave: NBITS squarings and ten
  // products in a row, where the chain of one lane has NBITS squarings and about NBITS / 2 products.
  template <class EL>
  __device__ __forceinline__ typename EL::T wave_inv_raw(const typename EL::T& x, int lane)
  {
    using T = typename EL::T;
    if constexpr (EL::WAVE_POW) {
      constexpr int GROUPS = (EL::NBITS + 63) / 64;
      T kept[GROUPS];
      T pw = x;
#pragma unroll
      for (int j = 0; j < GROUPS; j++) {
        kept[j] = EL::one();
        const int steps = EL::NBITS - 64 * j < 64 ? EL::NBITS - 64 * j : 64;
#pragma unroll 1
        for (int s = 0; s < steps; s++) {
          kept[j] = pick(lane == s, pw, kept[j]);
          pw = EL::sqr_raw(pw);
        }
      }
      T f = pick(EL::pm2_bit(lane), kept[0], EL::one());
#pragma unroll
      for (int j = 1; j < GROUPS; j++)
        f = EL::mul_raw(f, pick(EL::pm2_bit(64 * j + lane), kept[j], EL::one()));
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1)
        f = EL::mul_raw(f, wave_read(f, lane ^ off));
      return f;
    } else {
      return EL::inv_raw(x);
    }
  }

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

  enum { RED_SUM = 0, RED_PRODUCT = 1 };

  template <class EL, int OP>
  struct Reduce {
    using T = typename EL::T;
    static __device__ __forceinline__ T identity()
    {
      if constexpr (OP == RED_SUM)
        return EL::zero();
      else
        return EL::one();
    }
    static __device__ __forceinline__ T op(const T& a, const T& b)
    {
      if constexpr (OP == RED_SUM)
        return EL::sum(a, b);
      else
        return EL::mul_raw(a, b);
    }
    static __device__ __forceinline__ T wave_all(T acc, int lane) // every lane ends with the wave's result
    {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1)
        acc = op(acc, wave_read(acc, lane ^ off));
      return acc;
    }
  };

  // partials[k * chunks + c] = the reduction of elements j in [c * chunk_len, (c + 1) * chunk_len) of entry k; blockIdx.x = c.
  // along_k false: blockIdx.y walks the entries, the lanes of the block run along j (element (k, j) at k * sk + j * sj).
  // along_k true (columns_batch with 64 entries or more): blockIdx.y walks groups of 64 entries, lanes run along k and the
  // waves of the block along j, so that a wave reads 64 neighbouring elements of one row j.
  template <class EL, int OP>
  __global__ __launch_bounds__(256) void k_vec_reduce(const uint32_t* __restrict__ a, typename EL::T* __restrict__ partials, uint64_t size, uint32_t batch, uint64_t chunk_len,
                                                      uint32_t chunks, uint64_t sj, uint64_t sk, uint32_t groups, bool along_k)
  {
    using T = typename EL::T;
    using R = Reduce<EL, OP>;
    constexpr int NW = sizeof(T) / 4;
    __shared__ uint32_t smem[4 * NW * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const uint64_t j0 = blockIdx.x * chunk_len, j1 = j0 + chunk_len < size ? j0 + chunk_len : size;
    for (uint32_t g = blockIdx.y; g < groups; g += gridDim.y) {
      T acc = R::identity();
      uint64_t k;
      if (along_k) {
        k = (uint64_t)g * 64 + lane;
        if (k < batch) {
#pragma unroll 4
          for (uint64_t j = j0 + wave; j < j1; j += waves)
            acc = R::op(acc, EL::load(a + (j * batch + k) * EL::W));
        }
      } else {
        k = g;
#pragma unroll 4
        for (uint64_t j = j0 + threadIdx.x; j < j1; j += blockDim.x)
          acc = R::op(acc, EL::load(a + (k * sk + j * sj) * EL::W));
        acc = R::wave_all(acc, lane);
      }
      uint32_t w[NW];
      if (waves > 1) {
        __builtin_memcpy(w, &acc, sizeof(T));
#pragma unroll
        for (int q = 0; q < NW; q++)
          smem[(wave * NW + q) * 64 + lane] = w[q];
        __syncthreads();
      }
      if (wave == 0) {
        for (int v = 1; v < waves; v++) {
#pragma unroll
          for (int q = 0; q < NW; q++)
            w[q] = smem[(v * NW + q) * 64 + lane];
          T o;
          __builtin_memcpy(&o, w, sizeof(T));
          acc = R::op(acc, o);
        }
        if (along_k ? k < batch : lane == 0) partials[k * chunks + blockIdx.x] = acc;
      }
      if (waves > 1) __syncthreads();
    }
  }

  // out[k] = the reduction of partials[k * chunks ..], one wave per entry; a product gets its powers of R back (vecops_elem.hpp)
  template <class EL, int OP>
  __global__ __launch_bounds__(64) void k_vec_reduce_finish(const typename EL::T* __restrict__ partials, uint32_t chunks, uint32_t batch, uint64_t size, uint32_t* __restrict__ out)
  {
    using T = typename EL::T;
    using R = Reduce<EL, OP>;
    const int lane = threadIdx.x;
    for (uint32_t k = blockIdx.x; k < batch; k += gridDim.x) {
      T acc = R::identity();
      for (uint32_t c = lane; c < chunks; c += 64)
        acc = R::op(acc, partials[(uint64_t)k * chunks + c]);
      acc = R::wave_all(acc, lane);
      if (lane == 0) {
        if (OP == RED_PRODUCT) acc = EL::scale_pow(acc, size);
        EL::store(out + (uint64_t)k * EL::W, acc);
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

  template <class EL, int OP>
  static icicle_error_t reduce_run(const void* a, uint64_t size, const icicle_vec_ops_config_t* cfg, void* out)
  {
    using T = typename EL::T;
    if (!cfg) return ICICLE_INVALID_POINTER;
    if (size == 0) return ICICLE_SUCCESS;
    if (!a || !out) return ICICLE_INVALID_POINTER;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const uint32_t batch = (uint32_t)std::max(1, cfg->batch_size);
    const bool columns = cfg->columns_batch && batch > 1;
    const size_t ebytes = (size_t)EL::W * 4, out_bytes = (size_t)batch * ebytes;
    Staged sa;
    ICICLE_TRY(sa.in(a, cfg->is_a_on_device, (size_t)size * batch * ebytes, st));
    TempBuf d_out_tmp;
    uint32_t* d_out = (uint32_t*)out;
    if (!cfg->is_result_on_device) {
      HIP_TRY(d_out_tmp.alloc(out_bytes, st), ICICLE_ALLOCATION_FAILED);
      d_out = d_out_tmp.as<uint32_t>();
    }
    // One launch covers every entry: `groups` rows of blocks (entries, or groups of 64 entries) times `chunks` blocks along j.
    // A chunk is about 16 elements per lane, fewer chunks where the entries alone fill the device.
    const bool along_k = columns && batch >= 64;
    const uint32_t groups = along_k ? (batch + 63) / 64 : batch;
    const uint64_t per_block = along_k ? 64 : 4096;
    const uint64_t want = (size + per_block - 1) / per_block, room = std::max<uint64_t>(1, 8192 / groups);
    const uint32_t chunks = (uint32_t)std::min(want, room);
    const uint64_t chunk_len = (size + chunks - 1) / chunks;
    const unsigned threads = along_k ? (chunk_len > 1 ? 256 : 64) : (chunk_len > 64 ? 256 : 64);
    TempBuf partials;
    HIP_TRY(partials.alloc((size_t)batch * chunks * sizeof(T), st), ICICLE_ALLOCATION_FAILED);
    k_vec_reduce<EL, OP><<<dim3(chunks, std::min(groups, 65535u)), threads, 0, st>>>(sa.dev, partials.as<T>(), size, batch, chunk_len, chunks, columns ? batch : 1,
                                                                                       columns ? 1 : size, groups, along_k);
    LAUNCH_CHECK("k_vec_reduce", st);
    k_vec_reduce_finish<EL, OP><<<std::min(batch, 1u << 20), 64, 0, st>>>(partials.as<T>(), chunks, batch, size, d_out);
    LAUNCH_CHECK("k_vec_reduce_finish", st);
    return finish_out(out, d_out, cfg->is_result_on_device, cfg->is_async, out_bytes, st);
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
