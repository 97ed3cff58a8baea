// slice, highest_non_zero_idx, poly_eval and poly_division for the eight fields of vecops_arith.hip.
//
// Reference semantics: icicle/src/vec_ops.cpp:472 (slice), :549 (highest_non_zero_idx), :621 (poly_eval), :648
// (poly_division); CPU backend icicle/backend/cpu/src/field/cpu_vec_ops.cpp:566-624, 682-780. Elements are canonical words in and out;
// every size is per batch entry, entry k holding its element j at k * size + j, or at j * batch_size + k with columns_batch. What is
// decided on the host -- argument rules, the route of poly_eval, the tile schedule of the division -- is poly_plan.h.
//
// Montgomery bookkeeping (vecops_elem.hpp): a loaded value x is read as the representative of x / R, mul_raw(a, b) = a b / R. Evaluation and
// division are linear in the coefficients, so coefficients are never converted: the multiplier is (x R for a point x, R / lc for the
// leading coefficient's inverse, b R for the denominator) and mul_raw(coefficient, multiplier) is the plain product, canonical words
// again once stored. Lazy bounds of BigElem (bigfield.hpp: a loaded value < 1.2 p, mul takes operands up to 64 p and returns less than
// (Ka Kb / 64 + 1) p, store reduces anything below 32 p) are stated where a chain is built.
#include "vecops_tile.hpp" // wave_read, pick, wave_inv_raw
#include "poly_plan.h"
#include <algorithm>

namespace icicle_hip {

  // what the polynomial kernels need beyond vecops_elem.hpp's interface
  template <class EL>
  struct PolyOps;
  template <class PR>
  struct PolyOps<SmallElem<PR>> {
    using T = typename SmallElem<PR>::T;
    using S = SmallField<PR>;
    static __device__ __forceinline__ T r2() { return T{PR::R2}; }
    static __device__ __forceinline__ T add_lazy(const T& a, const T& b) { return T{S::add(a.v, b.v)}; }
    static __device__ __forceinline__ T below4(const T& a) { return a; }
    static __device__ __forceinline__ T sub_small(const T& a, const T& b) { return T{S::sub(a.v, b.v)}; }
    static __device__ __forceinline__ T sub_sum(const T& a, const T& b) { return T{S::sub(a.v, b.v)}; }
    // (a b + c d) / R with one reduction: 2 p^2 < p 2^32, what mont_reduce takes
    static __device__ __forceinline__ T dot2(const T& a, const T& b, const T& c, const T& d) { return T{S::mont_reduce((uint64_t)a.v * b.v + (uint64_t)c.v * d.v)}; }
  };
  template <class PR>
  struct PolyOps<BigElem<PR>> {
    using F = FieldOps<PR>;
    using T = typename F::fe;
    static __device__ __forceinline__ T r2() { return F::r2(); }
    static __device__ __forceinline__ T add_lazy(const T& a, const T& b) { return F::add(a, b); } // no reduction: the caller keeps the sum below 16 p
    static __device__ __forceinline__ T below4(const T& a) { return F::below4(a); }               // < 16 p -> < 4 p
    static __device__ __forceinline__ T sub_small(const T& a, const T& b) // a < 4 p, b a product (< 2 p): a - b + 2 p < 6 p, brought back below 4 p
    {
      T r = F::template sub<2>(a, b);
      F::template cond_sub<4>(r);
      return r;
    }
    static __device__ __forceinline__ T sub_sum(const T& a, const T& b) { return F::template sub<4>(a, b); } // b < 4 p; the result (< a + 4 p) is stored at once
    static __device__ __forceinline__ T dot2(const T& a, const T& b, const T& c, const T& d) { return F::mul_add(a, b, c, d); } // one shared reduction
  };
  template <>
  struct PolyOps<GoldElem> {
    using F = FieldOps<goldilocks_params>;
    using T = GoldFe;
    static __device__ __forceinline__ T r2() { return F::one(); } // R = 1
    static __device__ __forceinline__ T add_lazy(const T& a, const T& b) { return F::add(a, b); }
    static __device__ __forceinline__ T below4(const T& a) { return a; }
    static __device__ __forceinline__ T sub_small(const T& a, const T& b) { return F::template sub<2>(a, b); }
    static __device__ __forceinline__ T sub_sum(const T& a, const T& b) { return F::template sub<2>(a, b); }
    static __device__ __forceinline__ T dot2(const T& a, const T& b, const T& c, const T& d) { return F::add(F::mul(a, b), F::mul(c, d)); } // no shared form
  };

  // element j of entry k of a batch of vectors of `size` elements
  __host__ __device__ __forceinline__ uint64_t batch_index(uint64_t k, uint64_t j, uint64_t size, uint32_t batch, bool columns) { return columns ? j * batch + k : k * size + j; }

  // ================================================================ slice ================================================================
  template <int W, bool VEC>
  __device__ __forceinline__ void copy_element(uint32_t* d, const uint32_t* s)
  {
    if constexpr (VEC && W == 2) {
      *reinterpret_cast<uint2*>(d) = *reinterpret_cast<const uint2*>(s);
    } else if constexpr (VEC && W >= 4) {
#pragma unroll
      for (int q = 0; q < W / 4; q++)
        reinterpret_cast<uint4*>(d)[q] = reinterpret_cast<const uint4*>(s)[q];
    } else {
#pragma unroll
      for (int w = 0; w < W; w++)
        d[w] = s[w];
    }
  }

  // out[k][t] = in[k][offset + t * stride], t < size_out: one lane per output element, W words per element
  template <int W, bool VEC>
  __global__ __launch_bounds__(256) void k_slice(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t offset, uint64_t stride, uint64_t size_in, uint64_t size_out,
                                                 uint32_t batch, bool columns)
  {
    const uint64_t total = size_out * batch, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total; i += step) {
      const uint64_t k = columns ? i % batch : i / size_out, t = columns ? i / batch : i % size_out;
      copy_element<W, VEC>(out + i * W, in + batch_index(k, offset + t * stride, size_in, batch, columns) * W);
    }
  }

  template <int W>
  static icicle_error_t slice_run(const void* in, uint64_t offset, uint64_t stride, uint64_t size_in, uint64_t size_out, const icicle_vec_ops_config_t* cfg, void* out)
  {
    const uint32_t batch = cfg ? (uint32_t)std::max(1, cfg->batch_size) : 1;
    switch (poly_slice_check(cfg != nullptr, in, cfg && cfg->is_a_on_device, out, cfg && cfg->is_result_on_device, offset, stride, size_in, size_out, batch, W * 4)) {
    case POLY_EMPTY: return ICICLE_SUCCESS;
    case POLY_BAD_POINTER: return ICICLE_INVALID_POINTER;
    case POLY_BAD_ARGUMENT: return ICICLE_INVALID_ARGUMENT;
    default: break;
    }
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const bool columns = cfg->columns_batch && batch > 1;
    const size_t out_bytes = (size_t)size_out * batch * W * 4;
    Staged sa;
    StagedOut so;
    ICICLE_TRY(sa.in(in, cfg->is_a_on_device, (size_t)size_in * batch * W * 4, st));
    ICICLE_TRY(so.out(out, cfg->is_result_on_device, out_bytes, st));
    constexpr uintptr_t ALIGN = W * 4 < 16 ? W * 4 : 16;
    const bool vec = (((uintptr_t)sa.dev | (uintptr_t)so.dev) & (ALIGN - 1)) == 0;
    const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)size_out * batch + 255) / 256, 1u << 20);
    if (vec)
      k_slice<W, true><<<grid, 256, 0, st>>>(sa.dev, so.dev, offset, stride, size_in, size_out, batch, columns);
    else
      k_slice<W, false><<<grid, 256, 0, st>>>(sa.dev, so.dev, offset, stride, size_in, size_out, batch, columns);
    LAUNCH_CHECK("k_slice", st);
    return so.finish(cfg->is_async);
  }

  // ======================================================== highest_non_zero_idx ========================================================
  __device__ __forceinline__ int64_t wave_max_i64(int64_t v)
  {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int64_t o = __shfl_xor((long long)v, off);
      v = o > v ? o : v;
    }
    return v;
  }

  // partials[k * chunks + c] = the largest j in [c * chunk_len, (c + 1) * chunk_len) with a non-zero element (any word), or -1;
  // blockIdx.x = c, blockIdx.y walks the entries: lane -> wave -> block -> one partial per block, as k_vec_reduce
  template <int W>
  __global__ __launch_bounds__(256) void k_hnz(const uint32_t* __restrict__ a, int64_t* __restrict__ partials, uint64_t size, uint32_t batch, uint64_t chunk_len, uint32_t chunks,
                                               bool columns)
  {
    __shared__ int64_t smem[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t j0 = blockIdx.x * chunk_len, j1 = j0 + chunk_len < size ? j0 + chunk_len : size;
    for (uint32_t k = blockIdx.y; k < batch; k += gridDim.y) {
      int64_t best = -1;
      for (uint64_t j = j0 + threadIdx.x; j < j1; j += 256) {
        const uint32_t* p = a + batch_index(k, j, size, batch, columns) * W;
        uint32_t o = 0;
#pragma unroll
        for (int w = 0; w < W; w++)
          o |= p[w];
        if (o) best = (int64_t)j; // j rises: the last hit is this lane's largest
      }
      best = wave_max_i64(best);
      if (lane == 0) smem[wave] = best;
      __syncthreads();
      if (threadIdx.x == 0) {
        for (int v = 1; v < 4; v++)
          best = smem[v] > best ? smem[v] : best;
        partials[(uint64_t)k * chunks + blockIdx.x] = best;
      }
      __syncthreads();
    }
  }

  // out[k] = the maximum of partials[k * chunks ..], one wave per entry
  __global__ __launch_bounds__(64) void k_hnz_finish(const int64_t* __restrict__ partials, uint32_t chunks, uint32_t batch, int64_t* __restrict__ out)
  {
    const int lane = threadIdx.x;
    for (uint32_t k = blockIdx.x; k < batch; k += gridDim.x) {
      int64_t best = -1;
      for (uint32_t c = lane; c < chunks; c += 64) {
        const int64_t v = partials[(uint64_t)k * chunks + c];
        best = v > best ? v : best;
      }
      best = wave_max_i64(best);
      if (lane == 0) out[k] = best;
    }
  }

  // both launches, device to device: d_out[k], k < batch (also the degree scan of the division)
  template <int W>
  static icicle_error_t hnz_launch(const uint32_t* d_in, uint64_t size, uint32_t batch, bool columns, int64_t* d_out, TempBuf& partials, hipStream_t st)
  {
    const PolyHnzPlan p = poly_hnz_plan(size);
    HIP_TRY(partials.alloc((size_t)batch * p.chunks * sizeof(int64_t), st), ICICLE_ALLOCATION_FAILED);
    k_hnz<W><<<dim3(p.chunks, std::min(batch, 65535u)), 256, 0, st>>>(d_in, partials.as<int64_t>(), size, batch, p.chunk_len, p.chunks, columns);
    LAUNCH_CHECK("k_hnz", st);
    k_hnz_finish<<<std::min(batch, 1u << 20), 64, 0, st>>>(partials.as<int64_t>(), p.chunks, batch, d_out);
    LAUNCH_CHECK("k_hnz_finish", st);
    return ICICLE_SUCCESS;
  }

  template <int W>
  static icicle_error_t hnz_run(const void* in, uint64_t size, const icicle_vec_ops_config_t* cfg, int64_t* out)
  {
    switch (poly_hnz_check(cfg != nullptr, in, out, size)) {
    case POLY_BAD_POINTER: return ICICLE_INVALID_POINTER;
    case POLY_BAD_ARGUMENT: return ICICLE_INVALID_ARGUMENT;
    default: break;
    }
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const uint32_t batch = (uint32_t)std::max(1, cfg->batch_size);
    const bool columns = cfg->columns_batch && batch > 1;
    const size_t out_bytes = (size_t)batch * sizeof(int64_t);
    Staged sa;
    StagedOut so;
    TempBuf partials;
    ICICLE_TRY(sa.in(in, cfg->is_a_on_device, (size_t)size * batch * W * 4, st));
    ICICLE_TRY(so.out(out, cfg->is_result_on_device, out_bytes, st));
    ICICLE_TRY(hnz_launch<W>(sa.dev, size, batch, columns, (int64_t*)so.dev, partials, st));
    return so.finish(cfg->is_async);
  }

  // ================================================================ poly_eval ================================================================
  // Point route: evals[k][e] = P_k(domain[e]), one lane per (k, e). blockIdx.y walks the entries, so every lane of a block reads the same
  // coefficient: its address depends on the block and the loop counter only (a uniform load, not one per lane).
  // BigElem: acc < 1.1 p + 1.2 p after every step, far below what mul takes; the store reduces.
  template <class EL>
  __global__ __launch_bounds__(256) void k_poly_eval_point(const uint32_t* __restrict__ coeffs, const uint32_t* __restrict__ domain, uint32_t* __restrict__ evals, uint64_t n,
                                                           uint64_t domain_size, uint32_t batch, bool columns)
  {
    using T = typename EL::T;
    using P = PolyOps<EL>;
    constexpr int W = EL::W;
    const uint64_t sj = columns ? batch : 1;
    for (uint32_t k = blockIdx.y; k < batch; k += gridDim.y) {
      const uint32_t* ck = coeffs + (columns ? (uint64_t)k : (uint64_t)k * n) * W;
      for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e < domain_size; e += (uint64_t)gridDim.x * blockDim.x) {
        const T x = EL::mul_raw(EL::load(domain + e * W), P::r2()); // x R
        T acc = EL::load(ck + (n - 1) * sj * W);
        for (uint64_t j = n - 1; j-- > 0;)
          acc = P::add_lazy(EL::mul_raw(acc, x), EL::load(ck + j * sj * W));
        EL::store(evals + batch_index(k, e, domain_size, batch, columns) * W, acc);
      }
    }
  }

  // Split route, one level: wave (p, c) evaluates chunk c -- values j in [c C, min(n, (c + 1) C)) of pair p's vector -- at the pair's point,
  // sum_i v[c C + i] x^i. Lane l runs Horner in x^64 over i = l, l + 64, ...; the 64 lane values V_l are then folded in six steps, step s
  // adding x^(2^s) V_(l + 2^s) to V_l, so that lane 0 ends with sum_l x^l V_l. FIRST: the vector is the caller's coefficients of entry
  // p / domain_size; else it is the previous level's chunk values, `n` per pair. One chunk per pair (chunks == 1) is the last level:
  // lane 0 stores the evaluation; else it writes the chunk value for the next level.
  // BigElem: a chunk value is kept below 4 p (below4 after the Horner loop, EL::sum in the fold), so the Horner sum of the next level is
  // below 1.1 p + 4 p. The point of a level is domain[e]^xpow (xpow = 1, then the product of the chunk lengths so far): every wave converts
  // its point once (x R) and raises it itself, a few products beside the Horner steps of its chunk, which saves the launches of a table.
  template <class EL, bool FIRST>
  __global__ __launch_bounds__(256) void k_poly_chunk(const uint32_t* __restrict__ coeffs, const typename EL::T* __restrict__ values, const uint32_t* __restrict__ domain,
                                                      uint64_t xpow, typename EL::T* __restrict__ out_values, uint32_t* __restrict__ evals, uint64_t n, uint64_t C, uint64_t chunks,
                                                      uint64_t pairs, uint64_t domain_size, uint32_t batch, bool columns)
  {
    using T = typename EL::T;
    using P = PolyOps<EL>;
    constexpr int W = EL::W;
    const int lane = threadIdx.x & 63;
    const uint64_t waves = pairs * chunks;
    for (uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < waves; w += (uint64_t)gridDim.x * 4) {
      const uint64_t p = w / chunks, c = w % chunks;
      const uint64_t k = p / domain_size, e = p % domain_size;
      const uint64_t base = c * C, len = n - base < C ? n - base : C;
      T pw[7]; // x^(2^s) R
      pw[0] = EL::mul_raw(EL::load(domain + e * W), P::r2());
      if (xpow > 1) { // square and multiply over the bits of xpow; EL::one() is the Montgomery one
        T b = pw[0];
        pw[0] = EL::one();
        for (uint64_t x = xpow; x; x >>= 1) {
          if (x & 1) pw[0] = EL::mul_raw(pw[0], b);
          b = EL::mul_raw(b, b);
        }
      }
#pragma unroll
      for (int s = 1; s < 7; s++)
        pw[s] = EL::mul_raw(pw[s - 1], pw[s - 1]);
      T acc = EL::zero();
      const uint64_t steps = (len + 63) / 64;
      for (uint64_t i = steps; i-- > 0;) {
        const uint64_t idx = (uint64_t)lane + 64 * i;
        T v = EL::zero();
        if (idx < len) {
          if constexpr (FIRST)
            v = EL::load(coeffs + batch_index(k, base + idx, n, batch, columns) * W);
          else
            v = values[p * n + base + idx];
        }
        acc = P::add_lazy(EL::mul_raw(acc, pw[6]), v);
      }
      acc = P::below4(acc);
#pragma unroll
      for (int s = 0; s < 6; s++) { // lane l (a multiple of 2^(s+1)) takes in lane l + 2^s
        const T other = wave_read(acc, (lane + (1 << s)) & 63);
        acc = EL::sum(acc, EL::mul_raw(other, pw[s]));
      }
      if (lane == 0) {
        if (chunks == 1)
          EL::store(evals + batch_index(k, e, domain_size, batch, columns) * W, acc);
        else
          out_values[p * chunks + c] = acc;
      }
    }
  }

  static inline int poly_eval_chunk_key(const icicle_vec_ops_config_t* cfg) { return (cfg && cfg->ext) ? reinterpret_cast<const ConfigExt*>(cfg->ext)->get_int("hip_poly_eval_chunk", 0) : 0; }

  template <class EL>
  static icicle_error_t poly_eval_run(const void* coeffs, uint64_t coeffs_size, const void* domain, uint64_t domain_size, const icicle_vec_ops_config_t* cfg, void* evals)
  {
    using T = typename EL::T;
    constexpr size_t EB = (size_t)EL::W * 4;
    const int key = poly_eval_chunk_key(cfg);
    switch (poly_eval_check(cfg != nullptr, coeffs, domain, evals, coeffs_size, domain_size, key)) {
    case POLY_BAD_POINTER: return ICICLE_INVALID_POINTER;
    case POLY_BAD_ARGUMENT: return ICICLE_INVALID_ARGUMENT;
    default: break;
    }
    const uint32_t batch = (uint32_t)std::max(1, cfg->batch_size);
    const size_t c_bytes = (size_t)coeffs_size * batch * EB, d_bytes = (size_t)domain_size * EB, out_bytes = (size_t)domain_size * batch * EB;
    if (poly_overlap(evals, out_bytes, cfg->is_result_on_device, coeffs, c_bytes, cfg->is_a_on_device) ||
        poly_overlap(evals, out_bytes, cfg->is_result_on_device, domain, d_bytes, cfg->is_b_on_device))
      return ICICLE_INVALID_ARGUMENT;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const bool columns = cfg->columns_batch && batch > 1;
    Staged sa, sb;
    StagedOut so;
    ICICLE_TRY(sa.in(coeffs, cfg->is_a_on_device, c_bytes, st));
    ICICLE_TRY(sb.in(domain, cfg->is_b_on_device, d_bytes, st));
    ICICLE_TRY(so.out(evals, cfg->is_result_on_device, out_bytes, st));
    const uint64_t pairs = (uint64_t)domain_size * batch;
    const PolyEvalPlan plan = poly_eval_plan(coeffs_size, pairs, key);
    TempBuf vals[2];
    if (!plan.split) {
      const unsigned threads = domain_size <= 64 ? 64 : 256;
      const unsigned gx = (unsigned)std::min<uint64_t>((domain_size + threads - 1) / threads, 1u << 20);
      k_poly_eval_point<EL><<<dim3(gx, std::min(batch, 65535u)), threads, 0, st>>>(sa.dev, sb.dev, so.dev, coeffs_size, domain_size, batch, columns);
      LAUNCH_CHECK("k_poly_eval_point", st);
    } else {
      uint64_t n = coeffs_size;
      const T* in_vals = nullptr;
      uint64_t xpow = 1;
      for (int level = 0;; level++) {
        const uint64_t C = level == 0 ? plan.chunk : poly_eval_chunk(n, pairs, key, false);
        const uint64_t chunks = (n + C - 1) / C;
        TempBuf& ob = vals[level & 1];
        T* out_vals = nullptr;
        if (chunks > 1) {
          HIP_TRY(ob.alloc((size_t)pairs * chunks * sizeof(T), st), ICICLE_ALLOCATION_FAILED);
          out_vals = ob.as<T>();
        }
        const unsigned grid = (unsigned)std::min<uint64_t>((pairs * chunks + 3) / 4, 1u << 20);
        if (level == 0)
          k_poly_chunk<EL, true><<<grid, 256, 0, st>>>(sa.dev, nullptr, sb.dev, xpow, out_vals, so.dev, n, C, chunks, pairs, domain_size, batch, columns);
        else
          k_poly_chunk<EL, false><<<grid, 256, 0, st>>>(nullptr, in_vals, sb.dev, xpow, out_vals, so.dev, n, C, chunks, pairs, domain_size, batch, columns);
        LAUNCH_CHECK("k_poly_chunk", st);
        if (chunks == 1) break;
        xpow *= C; // no overflow: another level exists only while about coeffs_size / xpow > 1 values are left
        in_vals = out_vals;
        n = chunks;
      }
    }
    return so.finish(cfg->is_async);
  }

  // ============================================================== poly_division ==============================================================
  // r[k][j] = j < num_size ? num[k][j] : 0 for j < r_size, and q = 0: both outputs are fully written
  template <int W>
  __global__ __launch_bounds__(256) void k_poly_div_init(const uint32_t* __restrict__ num, uint32_t* __restrict__ r, uint32_t* __restrict__ q, uint64_t num_size, uint64_t r_size,
                                                         uint64_t q_size, uint32_t batch, bool columns)
  {
    const uint64_t nr = r_size * batch, total = nr + q_size * batch;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
      if (i < nr) {
        const uint64_t k = columns ? i % batch : i / r_size, j = columns ? i / batch : i % r_size;
#pragma unroll
        for (int w = 0; w < W; w++)
          r[i * W + w] = j < num_size ? num[batch_index(k, j, num_size, batch, columns) * W + w] : 0u;
      } else {
#pragma unroll
        for (int w = 0; w < W; w++)
          q[(i - nr) * W + w] = 0u;
      }
    }
  }

  // lci[k] = R / lc(b_k): mul_raw(r, lci) = r / lc. One wave per entry, once per call (deg holds the numerators' degrees, then the
  // denominators'; the host has checked that no denominator is zero)
  template <class EL>
  __global__ __launch_bounds__(64) void k_poly_div_lcinv(const uint32_t* __restrict__ den, const int64_t* __restrict__ deg, uint32_t batch, uint64_t den_size, bool columns,
                                                         typename EL::T* __restrict__ lci)
  {
    const uint32_t k = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t db = deg[batch + k];
    if (db < 0) return;
    const typename EL::T x = EL::load(den + batch_index(k, (uint64_t)db, den_size, batch, columns) * EL::W);
    const typename EL::T r = EL::unscale(wave_inv_raw<EL>(x, lane));
    if (lane == 0) lci[k] = r;
  }

  // Tile kernel: one workgroup per entry, lane s owns quotient coefficient hi - s and the remainder coefficient deg_b + hi - s in a
  // register. Step s: lane s has its final remainder value, q = r / lc goes to LDS, and the lanes below it (within deg_b) subtract
  // q * b[deg_b - (s' - s)]. cnt barriers. LDS: bm (b R, the top min(T, deg_b + 1) of the denominator) and qs, T elements each:
  // 2 KiB for the one-word fields, 4 KiB for Goldilocks, 18 KiB for the 256-bit fields (36-byte limb form), of the 64 KiB a block may have.
  // BigElem: R stays below 4 p (sub_small); q = mul(R, lci) < 1.1 p; q * bm < 2 p.
  template <class EL>
  __global__ __launch_bounds__(POLY_DIV_TILE) void k_poly_div_tile(uint32_t* __restrict__ r, uint32_t* __restrict__ q, const uint32_t* __restrict__ den, const int64_t* __restrict__ deg,
                                                                   const typename EL::T* __restrict__ lci, uint32_t batch, uint64_t r_size, uint64_t q_size, uint64_t den_size,
                                                                   bool columns, int64_t tile)
  {
    using T = typename EL::T;
    using P = PolyOps<EL>;
    constexpr int W = EL::W;
    __shared__ T bm[POLY_DIV_TILE];
    __shared__ T qs[POLY_DIV_TILE];
    const uint32_t k = blockIdx.x;
    const int64_t s = threadIdx.x;
    const int64_t db = deg[batch + k];
    PolyDivTile w;
    if (!poly_div_tile(deg[k], db, POLY_DIV_TILE, tile, &w)) return; // the same for every lane of the block
    if (s < w.nb) bm[s] = EL::mul_raw(EL::load(den + batch_index(k, (uint64_t)(db - s), den_size, batch, columns) * W), P::r2());
    T R = EL::zero();
    if (s < w.cnt) R = EL::load(r + batch_index(k, (uint64_t)(db + w.hi - s), r_size, batch, columns) * W);
    const T L = lci[k];
    __syncthreads();
    for (int64_t step = 0; step < w.cnt; step++) {
      if (s == step) qs[step] = EL::mul_raw(R, L);
      __syncthreads();
      const int64_t d = s - step;
      if (d > 0 && s < w.cnt && d < w.nb) R = P::sub_small(R, EL::mul_raw(qs[step], bm[d]));
    }
    if (s < w.cnt) {
      EL::store(q + batch_index(k, (uint64_t)(w.hi - s), q_size, batch, columns) * W, qs[s]);
      uint32_t* rz = r + batch_index(k, (uint64_t)(db + w.hi - s), r_size, batch, columns) * W;
#pragma unroll
      for (int x = 0; x < W; x++)
        rz[x] = 0u;
    }
  }

  // Update kernel: r[i] -= sum_{s < cnt} q[hi - s] * b[i - hi + s] for i in [upd_lo, upd_lo + deg_b), 256 coefficients per block,
  // blockIdx.x = entry * blocks_per_entry + block. The tile's quotient (as q R) and the 255 + cnt denominator coefficients the block touches
  // (zero outside [0, deg_b]) are staged in LDS; the sum is a dot product, two products per reduction where the element type shares
  // one (PolyOps::dot2). BigElem: dot2 < 1.1 p, acc < 4 p (EL::sum), r - acc + 4 p < 5.2 p is stored at once.
  template <class EL>
  __global__ __launch_bounds__(256) void k_poly_div_update(uint32_t* __restrict__ r, const uint32_t* __restrict__ q, const uint32_t* __restrict__ den, const int64_t* __restrict__ deg,
                                                           uint32_t batch, uint64_t r_size, uint64_t q_size, uint64_t den_size, bool columns, int64_t tile, uint32_t blocks_per_entry)
  {
    using T = typename EL::T;
    using P = PolyOps<EL>;
    constexpr int W = EL::W;
    __shared__ T qm[POLY_DIV_TILE];
    __shared__ T bw[256 + POLY_DIV_TILE];
    const uint32_t k = blockIdx.x / blocks_per_entry, bx = blockIdx.x % blocks_per_entry;
    const int64_t db = deg[batch + k];
    PolyDivTile w;
    if (!poly_div_tile(deg[k], db, POLY_DIV_TILE, tile, &w)) return;
    const int64_t i0 = w.upd_lo + (int64_t)bx * 256, i_end = w.upd_lo + w.upd_cnt;
    if (i0 >= i_end) return;
    for (int64_t u = threadIdx.x; u < w.cnt; u += 256)
      qm[u] = EL::mul_raw(EL::load(q + batch_index(k, (uint64_t)(w.hi - u), q_size, batch, columns) * W), P::r2());
    for (int64_t u = threadIdx.x; u < 255 + w.cnt; u += 256) {
      const int64_t bi = i0 - w.hi + u;
      bw[u] = (bi >= 0 && bi <= db) ? EL::load(den + batch_index(k, (uint64_t)bi, den_size, batch, columns) * W) : EL::zero();
    }
    __syncthreads();
    const int64_t i = i0 + threadIdx.x;
    if (i < i_end) {
      T acc = EL::zero();
      int64_t s = 0;
      for (; s + 1 < w.cnt; s += 2)
        acc = EL::sum(acc, P::dot2(qm[s], bw[threadIdx.x + s], qm[s + 1], bw[threadIdx.x + s + 1]));
      if (s < w.cnt) acc = EL::sum(acc, EL::mul_raw(qm[s], bw[threadIdx.x + s]));
      uint32_t* ri = r + batch_index(k, (uint64_t)i, r_size, batch, columns) * W;
      EL::store(ri, P::sub_sum(EL::load(ri), acc));
    }
  }

  template <class EL>
  static icicle_error_t poly_division_run(const void* num, uint64_t num_size, const void* den, int64_t den_size, const icicle_vec_ops_config_t* cfg, void* q_out, uint64_t q_size,
                                          void* r_out, uint64_t r_size)
  {
    using T = typename EL::T;
    constexpr int W = EL::W;
    constexpr size_t EB = (size_t)W * 4;
    switch (poly_division_check(cfg != nullptr, num, den, q_out, r_out, num_size, den_size)) {
    case POLY_BAD_POINTER: return ICICLE_INVALID_POINTER;
    case POLY_BAD_ARGUMENT: return ICICLE_INVALID_ARGUMENT;
    default: break;
    }
    const uint32_t batch = (uint32_t)std::max(1, cfg->batch_size);
    if (q_size >= (1ull << 48) || r_size >= (1ull << 48)) return ICICLE_INVALID_ARGUMENT;
    const size_t n_bytes = (size_t)num_size * batch * EB, b_bytes = (size_t)den_size * batch * EB, q_bytes = (size_t)q_size * batch * EB, r_bytes = (size_t)r_size * batch * EB;
    const bool o_dev = cfg->is_result_on_device;
    if (poly_overlap(q_out, q_bytes, o_dev, num, n_bytes, cfg->is_a_on_device) || poly_overlap(q_out, q_bytes, o_dev, den, b_bytes, cfg->is_b_on_device) ||
        poly_overlap(r_out, r_bytes, o_dev, num, n_bytes, cfg->is_a_on_device) || poly_overlap(r_out, r_bytes, o_dev, den, b_bytes, cfg->is_b_on_device) ||
        poly_overlap(q_out, q_bytes, o_dev, r_out, r_bytes, o_dev))
      return ICICLE_INVALID_ARGUMENT;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const bool columns = cfg->columns_batch && batch > 1;
    Staged sa, sb;
    ICICLE_TRY(sa.in(num, cfg->is_a_on_device, n_bytes, st));
    ICICLE_TRY(sb.in(den, cfg->is_b_on_device, b_bytes, st));
    // the degrees plan the launches: both scans, then one synchronisation
    TempBuf d_deg, part_n, part_b;
    HIP_TRY(d_deg.alloc((size_t)2 * batch * sizeof(int64_t), st), ICICLE_ALLOCATION_FAILED);
    ICICLE_TRY(hnz_launch<W>(sa.dev, num_size, batch, columns, d_deg.as<int64_t>(), part_n, st));
    ICICLE_TRY(hnz_launch<W>(sb.dev, (uint64_t)den_size, batch, columns, d_deg.as<int64_t>() + batch, part_b, st));
    std::vector<int64_t> deg((size_t)2 * batch);
    HIP_TRY(hipMemcpyAsync(deg.data(), d_deg.ptr(), deg.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
    HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    uint64_t tiles = 0;
    int64_t max_db = 0;
    for (uint32_t k = 0; k < batch; k++) {
      if (poly_division_degree_check(deg[k], deg[batch + k], q_size, r_size) != POLY_OK) return ICICLE_INVALID_ARGUMENT;
      tiles = std::max(tiles, poly_division_tiles(deg[k], deg[batch + k], POLY_DIV_TILE));
      max_db = std::max(max_db, deg[batch + k]);
    }
    StagedOut sq, sr;
    TempBuf lci;
    ICICLE_TRY(sq.out(q_out, o_dev, q_bytes, st));
    ICICLE_TRY(sr.out(r_out, o_dev, r_bytes, st));
    uint32_t *const d_q = sq.dev, *const d_r = sr.dev;
    const uint64_t init_total = ((uint64_t)r_size + q_size) * batch;
    if (init_total) {
      k_poly_div_init<W><<<(unsigned)std::min<uint64_t>((init_total + 255) / 256, 1u << 20), 256, 0, st>>>(sa.dev, d_r, d_q, num_size, r_size, q_size, batch, columns);
      LAUNCH_CHECK("k_poly_div_init", st);
    }
    if (tiles) {
      HIP_TRY(lci.alloc((size_t)batch * sizeof(T), st), ICICLE_ALLOCATION_FAILED);
      k_poly_div_lcinv<EL><<<batch, 64, 0, st>>>(sb.dev, d_deg.as<int64_t>(), batch, (uint64_t)den_size, columns, lci.as<T>());
      LAUNCH_CHECK("k_poly_div_lcinv", st);
      const uint32_t bpe = (uint32_t)((max_db + 255) / 256);
      if ((uint64_t)bpe * batch >= (1ull << 31)) return ICICLE_INVALID_ARGUMENT;
      for (uint64_t t = 0; t < tiles; t++) {
        k_poly_div_tile<EL><<<batch, POLY_DIV_TILE, 0, st>>>(d_r, d_q, sb.dev, d_deg.as<int64_t>(), lci.as<T>(), batch, r_size, q_size, (uint64_t)den_size, columns, (int64_t)t);
        LAUNCH_CHECK("k_poly_div_tile", st);
        if (bpe) {
          k_poly_div_update<EL><<<bpe * batch, 256, 0, st>>>(d_r, d_q, sb.dev, d_deg.as<int64_t>(), batch, r_size, q_size, (uint64_t)den_size, columns, (int64_t)t, bpe);
          LAUNCH_CHECK("k_poly_div_update", st);
        }
      }
    }
    ICICLE_TRY(sq.copy_back());
    return sr.finish(cfg->is_async); // one synchronisation for both results
  }

} // namespace icicle_hip

using namespace icicle_hip;

#define DEFINE_VEC_POLY(NAME, EL)                                                                                      \
  extern "C" icicle_error_t NAME##_slice(const void* in, uint64_t offset, uint64_t stride, uint64_t size_in, uint64_t size_out, const icicle_vec_ops_config_t* c, void* o) \
  {                                                                                                                    \
    GUARDED((slice_run<EL::W>(in, offset, stride, size_in, size_out, c, o)));                                          \
  }                                                                                                                    \
  extern "C" icicle_error_t NAME##_highest_non_zero_idx(const void* in, uint64_t n, const icicle_vec_ops_config_t* c, int64_t* o) { GUARDED((hnz_run<EL::W>(in, n, c, o))); } \
  extern "C" icicle_error_t NAME##_poly_eval(const void* coeffs, uint64_t n, const void* domain, uint64_t m, const icicle_vec_ops_config_t* c, void* o) \
  {                                                                                                                    \
    GUARDED((poly_eval_run<EL>(coeffs, n, domain, m, c, o)));                                                          \
  }                                                                                                                    \
  extern "C" icicle_error_t NAME##_poly_division(const void* num, uint64_t n, const void* den, int64_t m, const icicle_vec_ops_config_t* c, void* q, uint64_t qn, void* r, \
                                                 uint64_t rn)                                                          \
  {                                                                                                                    \
    GUARDED((poly_division_run<EL>(num, n, den, m, c, q, qn, r, rn)));                                                 \
  }

DEFINE_VEC_POLY(babybear, SmallElem<babybear_params>)
DEFINE_VEC_POLY(koalabear, SmallElem<koalabear_params>)
DEFINE_VEC_POLY(bn254, BigElem<bn254_fr_params>)
DEFINE_VEC_POLY(bls12_381, BigElem<bls12_381_fr_params>)
DEFINE_VEC_POLY(bls12_377, BigElem<bls12_377_fr_params>)
DEFINE_VEC_POLY(grumpkin, BigElem<bn254_fq_params>)
DEFINE_VEC_POLY(stark252, BigElem<stark252_fr_params>)
DEFINE_VEC_POLY(goldilocks, GoldElem)

extern "C" int icicle_hip_poly_division_tile(int words_per_element) { return poly_division_tile(words_per_element); }
