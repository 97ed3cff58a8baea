// The kernels that vecops_arith.hip, vecops_inv.hip, vecops_ext.hip and vecops_poly.hip share, generic over the element interface of
// vecops_elem.hpp and vecops_ext_elem.hpp, each with its run function over the host frame of vecops_host.hpp: the element-wise kernel,
// the shared inversion (one a^(p-2) chain per tile, Montgomery's trick) with its wave helpers, and the deterministic two-launch
// reduction.
#pragma once
#include "vecops_elem.hpp"
#include "vecops_host.hpp"

namespace icicle_hip {

  // 16-byte elements (EL::W == 4: the extension fields) have a second form with one 16-byte access per element, Vec16<EL> of
  // vecops_ext_elem.hpp. A run function picks it where every device pointer of the call allows it; a staging buffer always does.
  template <class EL>
  struct Vec16;
  static inline bool aligned16(const void* p, bool on_device) { return !on_device || ((uintptr_t)p & 15) == 0; }

  // ================================================================ element-wise ================================================================
  // out[i] = a[ai(i)] op b[i]; a_scalar: a holds one scalar per batch entry.
  // The contract of this kernel and of every other element-wise kernel of these files (k_convert_*, k_ext_mixed_mul, k_vec_inv): out
  // may be a or b. A lane reads its own element completely before it writes it and touches no other element, so no pointer is
  // __restrict__.
  template <class EL>
  __global__ __launch_bounds__(256) void k_vec2(const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t total, int op, bool a_scalar, uint64_t size, uint32_t batch, bool columns)
  {
    uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
      const uint64_t ai = !a_scalar ? i : (columns ? i % batch : i / size);
      const typename EL::T x = EL::load(a + ai * EL::W), y = EL::load(b + i * EL::W);
      EL::store(out + i * EL::W, EL::apply(op, x, y));
    }
  }

  template <class EL>
  static icicle_error_t vec2_run(const void* a, const void* b, uint64_t size, const icicle_vec_ops_config_t* cfg, void* out, int op, bool a_scalar)
  {
    if (!cfg) return ICICLE_INVALID_POINTER;
    if (size == 0) return ICICLE_SUCCESS;
    if (!a || !b || !out) return ICICLE_INVALID_POINTER;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const uint32_t batch = (uint32_t)std::max(1, cfg->batch_size);
    const uint64_t total = size * batch;
    const size_t ebytes = (size_t)EL::W * 4, bytes = (size_t)total * ebytes;
    Staged sa, sb;
    StagedOut so;
    ICICLE_TRY(sa.in(a, cfg->is_a_on_device, a_scalar ? (size_t)batch * ebytes : bytes, st));
    ICICLE_TRY(sb.in(b, cfg->is_b_on_device, bytes, st));
    ICICLE_TRY(so.out(out, cfg->is_result_on_device, bytes, st));
    const unsigned grid = (unsigned)std::min<uint64_t>((total + 255) / 256, 1u << 20);
    bool vec = false;
    if constexpr (EL::W == 4) {
      vec = aligned16(a, cfg->is_a_on_device) && aligned16(b, cfg->is_b_on_device) && aligned16(out, cfg->is_result_on_device);
      if (vec) k_vec2<Vec16<EL>><<<grid, 256, 0, st>>>(sa.dev, sb.dev, so.dev, total, op, a_scalar, size, batch, cfg->columns_batch);
    }
    if (!vec) k_vec2<EL><<<grid, 256, 0, st>>>(sa.dev, sb.dev, so.dev, total, op, a_scalar, size, batch, cfg->columns_batch);
    LAUNCH_CHECK("k_vec2", st);
    return so.finish(cfg->is_async);
  }

  // ================================================================ inversion ================================================================
  // What a lane of an inversion tile keeps of a divisor d, and how many divisors it takes. The tile shares one inversion among the
  // chain values, elements of CE: chain(d, num) is d's and leaves in `num` what join(q, num) makes d's inverse from, q = 1 / chain
  // value. Here, for the base fields, d is its own chain value and q its inverse; the extension elements chain their norms (vecops_ext.hip).
  // K divisors per lane: the K running products of a lane live in registers, and so do its K chain values (KEEP) where they are one or
  // two words. At nine limbs that would be 18 K VGPRs, so there only the products are kept (9 K) and the walk back reads each element a
  // second time, from the cache: these fields are bound by their arithmetic, not by memory.
  template <class EL>
  struct InvTile {
    using CE = EL;
    struct Num {};
    static constexpr int K = 16;
    static constexpr bool KEEP = EL::W < 8;
    static __device__ __forceinline__ typename EL::T chain(const typename EL::T& d, Num&) { return d; }
    static __device__ __forceinline__ typename EL::T join(const typename EL::T& q, const Num&) { return q; }
  };
  template <class EL>
  struct InvTile<Vec16<EL>> : InvTile<EL> {};
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
  // num, den and out may be the same vector (the contract stated at k_vec2).
  template <class EL, bool DIV>
  __global__ __launch_bounds__(256) void k_vec_inv(const uint32_t* num, const uint32_t* den, uint32_t* out, uint64_t total, uint64_t tiles)
  {
    using IT = InvTile<EL>;
    using CE = typename IT::CE;
    using C = typename CE::T;
    using Num = typename IT::Num;
    constexpr int K = IT::K;
    constexpr bool KEEP = IT::KEEP;
    const int lane = threadIdx.x & 63;
    for (uint64_t tile = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < tiles; tile += (uint64_t)gridDim.x * 4) {
      const uint64_t base = tile * (64 * K) + lane;
      Num c[K] = {};             // what join() needs of each divisor
      C x[KEEP ? K : 1], pre[K]; // its chain value; pre[j] = x[0] ... x[j-1]
      uint32_t masked = 0;       // zeros and positions past the end: one in the chain
      C run = CE::one();
#pragma unroll
      for (int j = 0; j < K; j++) {
        const uint64_t i = base + (uint64_t)j * 64;
        C v = CE::one();
        bool skip = true;
        if (i < total) {
          const typename EL::T d = EL::load(den + i * EL::W);
          if (!EL::is_zero(d)) v = IT::chain(d, c[j]), skip = false;
        }
        masked |= (skip ? 1u : 0u) << j;
        if (KEEP) x[j] = v;
        pre[j] = run;
        if (j == 0)
          run = v;
        else
          run = CE::mul_raw(run, v);
      }
      // across the wave: the products of the lane totals before and after this lane, and the product of all
      C incl = run, suff = run;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const C lo = wave_read(incl, (lane - off) & 63), hi = wave_read(suff, (lane + off) & 63);
        const C a = CE::mul_raw(incl, lo), b = CE::mul_raw(suff, hi);
        incl = pick(lane >= off, a, incl);
        suff = pick(lane + off < 64, b, suff);
      }
      const C before = wave_read(incl, (lane - 1) & 63), after = wave_read(suff, (lane + 1) & 63);
      // one inversion per tile, R^2 / x: a quotient takes one R back in its product with the numerator
      C r = CE::unscale(wave_inv_raw<CE>(wave_read(incl, 63), lane));
      if (!DIV) r = CE::unscale(r);
      const C rb = CE::mul_raw(r, before);
      r = pick(lane > 0, rb, r);
      const C ra = CE::mul_raw(r, after);
      r = pick(lane < 63, ra, r);
      // r = 1 / (this lane's total): peel the chain values off backwards
#pragma unroll
      for (int j = K - 1; j >= 0; j--) {
        const uint64_t i = base + (uint64_t)j * 64;
        C q = r;
        if (j > 0) {
          q = CE::mul_raw(r, pre[j]);
          C xj = CE::one();
          if (KEEP) {
            xj = x[j];
          } else if (!((masked >> j) & 1)) {
            Num unused;
            xj = IT::chain(EL::load(den + i * EL::W), unused);
          }
          r = CE::mul_raw(r, xj);
        }
        if (i < total) {
          typename EL::T o = IT::join(q, c[j]);
          if (DIV) o = EL::mul_raw(o, EL::load(num + i * EL::W));
          EL::store(out + i * EL::W, pick((masked >> j) & 1, EL::zero(), o));
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
    StagedOut so;
    ICICLE_TRY(sa.in(a, cfg->is_a_on_device, bytes, st));
    if (DIV) ICICLE_TRY(sb.in(b, cfg->is_b_on_device, bytes, st));
    ICICLE_TRY(so.out(out, cfg->is_result_on_device, bytes, st));
    constexpr uint64_t TILE = 64 * InvTile<EL>::K;
    const uint64_t tiles = (total + TILE - 1) / TILE;
    const unsigned grid = (unsigned)std::min<uint64_t>((tiles + 3) / 4, INV_MAX_GRID);
    const uint32_t* d_den = DIV ? sb.dev : sa.dev;
    bool vec = false;
    if constexpr (EL::W == 4) {
      vec = aligned16(a, cfg->is_a_on_device) && (!DIV || aligned16(b, cfg->is_b_on_device)) && aligned16(out, cfg->is_result_on_device);
      if (vec) k_vec_inv<Vec16<EL>, DIV><<<grid, 256, 0, st>>>(sa.dev, d_den, so.dev, total, tiles);
    }
    if (!vec) k_vec_inv<EL, DIV><<<grid, 256, 0, st>>>(sa.dev, d_den, so.dev, total, tiles);
    LAUNCH_CHECK("k_vec_inv", st);
    return so.finish(cfg->is_async);
  }

  // ================================================================ reductions ================================================================
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
    StagedOut so;
    ICICLE_TRY(sa.in(a, cfg->is_a_on_device, (size_t)size * batch * ebytes, st));
    ICICLE_TRY(so.out(out, cfg->is_result_on_device, out_bytes, st));
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
    k_vec_reduce_finish<EL, OP><<<std::min(batch, 1u << 20), 64, 0, st>>>(partials.as<T>(), chunks, batch, size, so.dev);
    LAUNCH_CHECK("k_vec_reduce_finish", st);
    return so.finish(cfg->is_async);
  }

} // namespace icicle_hip
