// What vecops_inv.hip and vecops_ext.hip share on the device: the wave helpers of the shared inversion (one a^(p-2) chain per tile,
// Montgomery's trick) and the deterministic two-launch reduction, both generic over the element interface of vecops_elem.hpp.
#pragma once
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
