// FRI over the 31-bit fields (BabyBear, KoalaBear), scalar and quartic extension: the fold kernel, and the prover and verifier
// of the reference's C ABI (src/fri/fri_c_api.cpp) composed from what hash.hip and ntt.hip provide.
//
// Reference semantics: backend/cpu/include/cpu_fri_backend.h:76-190 (commit-fold phase, proof of work, query phase),
// src/fri/fri.cpp:49-99,283-319 (verify), include/icicle/fri/fri_transcript.h (Fiat-Shamir). The host-only rules -- parameter
// checks, shapes, transcript bytes, sampler -- are in fri_plan.h.
//
// The fold: out[i] = (e[i] + e[i+h])/2 + alpha * ((e[i] - e[i+h])/2 * w_n^(-i)), h = n/2. Memory-bound: n elements in, n/2 out and
// n/2 twiddles gathered from the NTT domain's table with stride max/n. Elements are canonical in memory; alpha, alpha * W and the
// twiddles are in Montgomery form, and montmul(canonical, x*R) is canonical, so no conversion pass is needed; halving is a shift. A
// lane moves 16 bytes per access: one extension element, or four consecutive scalars from each half.
#include "common.h"
#include "smallfield.hpp"
#include "fri_plan.h"
#include <cstring>
#include <memory>
#include <new>

namespace icicle_hip {

  template <class PR>
  struct FriField; // field index of ntt_domain_table, and W of the extension F[x] / (x^4 - W)
  template <>
  struct FriField<babybear_params> {
    static constexpr int INDEX = 0;
    static constexpr uint32_t W = 11;
  };
  template <>
  struct FriField<koalabear_params> {
    static constexpr int INDEX = 1;
    static constexpr uint32_t W = 3;
  };

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

  // false: no domain on this device, or one smaller than 2^k
  template <class PR>
  static bool domain_for(uint32_t k, const uint32_t** tw, int* log_max)
  {
    return ntt_domain_table(FriField<PR>::INDEX, tw, log_max) && (int)k <= *log_max;
  }

  template <class PR, int WORDS>
  static icicle_error_t fold_run(const uint32_t* in, uint64_t n, const uint32_t* alpha, uint32_t* out, bool on_device, hipStream_t st)
  {
    if (!in || !alpha || !out) return ICICLE_INVALID_POINTER;
    if (n < 2 || !fri_is_pow2(n)) return ICICLE_INVALID_ARGUMENT;
    const uint32_t k = fri_log2(n);
    const uint32_t* tw = nullptr;
    int log_max = 0;
    if (!domain_for<PR>(k, &tw, &log_max)) return ICICLE_INVALID_ARGUMENT;
    ICICLE_TRY(bind_current_device());
    const size_t in_bytes = (size_t)n * WORDS * 4, out_bytes = in_bytes / 2;
    uint32_t a[4] = {0, 0, 0, 0};
    if (on_device) {
      HIP_TRY(hipMemcpyAsync(a, alpha, WORDS * 4, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
      HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
      return fold_launch<PR, WORDS>(in, out, k, a, tw, log_max, st);
    }
    std::memcpy(a, alpha, WORDS * 4);
    TempBuf d_in, d_out;
    HIP_TRY(d_in.alloc(in_bytes, st), ICICLE_ALLOCATION_FAILED);
    HIP_TRY(d_out.alloc(out_bytes, st), ICICLE_ALLOCATION_FAILED);
    HIP_TRY(hipMemcpyAsync(d_in.ptr(), in, in_bytes, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
    ICICLE_TRY((fold_launch<PR, WORDS>(d_in.as<uint32_t>(), d_out.as<uint32_t>(), k, a, tw, log_max, st)));
    HIP_TRY(hipMemcpyAsync(out, d_out.ptr(), out_bytes, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
    HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    return ICICLE_SUCCESS;
  }

  // ---- the proof object -----------------------------------------------------------------------------------------------------------
  // slots[q][r]: Merkle proofs owned by the FRI proof (handles of hash.hip's proof type, so icicle_merkle_proof_get_* read them)
  struct FriProofObj {
    std::vector<std::vector<icicle_merkle_proof_handle_t>> slots;
    std::vector<uint32_t> final_poly; // the elements' words back to back (1 or 4 per element)
    uint64_t nonce = 0;
    void clear()
    {
      for (auto& q : slots)
        for (auto p : q)
          if (p) (void)icicle_merkle_proof_delete(p);
      slots.clear();
      final_poly.clear();
      nonce = 0;
    }
    ~FriProofObj() { clear(); }
  };

  static icicle_merkle_proof_handle_t clone_merkle_proof(icicle_merkle_proof_handle_t src)
  {
    if (!src) return nullptr;
    size_t leaf_size = 0, root_size = 0, path_size = 0;
    uint64_t leaf_idx = 0;
    const uint8_t* leaf = icicle_merkle_proof_get_leaf(src, &leaf_size, &leaf_idx);
    const uint8_t* root = icicle_merkle_proof_get_root(src, &root_size);
    const uint8_t* path = icicle_merkle_proof_get_path(src, &path_size);
    return icicle_merkle_proof_create_with_data(icicle_merkle_proof_is_pruned(src), (int64_t)leaf_idx, leaf, leaf_size, root, root_size, path, path_size);
  }

  static FriProofObj* proof_from_arguments(icicle_merkle_proof_handle_t** query_proofs, size_t nof_queries, size_t nof_rounds, const uint32_t* final_poly,
                                           size_t final_poly_size, uint64_t pow_nonce, int words)
  {
    if ((nof_queries && nof_rounds && !query_proofs) || (final_poly_size && !final_poly)) return nullptr;
    std::unique_ptr<FriProofObj> p(new FriProofObj);
    p->slots.assign(nof_queries, std::vector<icicle_merkle_proof_handle_t>(nof_rounds, nullptr));
    for (size_t q = 0; q < nof_queries; q++)
      for (size_t r = 0; r < nof_rounds; r++) {
        if (!query_proofs[q] || !query_proofs[q][r]) return nullptr;
        if (!(p->slots[q][r] = clone_merkle_proof(query_proofs[q][r]))) return nullptr;
      }
    if (final_poly_size) p->final_poly.assign(final_poly, final_poly + final_poly_size * words);
    p->nonce = pow_nonce;
    return p.release();
  }

  // ---- the prover and the verifier ------------------------------------------------------------------------------------------------
  struct TreeHandle { // a tree of round r: the leaves hasher and `compress_layers` compress hashers
    icicle_merkle_tree_handle_t h = nullptr;
    TreeHandle() = default;
    TreeHandle(TreeHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
    TreeHandle(const TreeHandle&) = delete;
    TreeHandle& operator=(const TreeHandle&) = delete;
    ~TreeHandle()
    {
      if (h) (void)icicle_merkle_tree_delete(h);
    }
    bool create(icicle_hasher_handle_t leaves, icicle_hasher_handle_t compress, uint32_t layers, uint64_t element_bytes, uint64_t store_min)
    {
      std::vector<icicle_hasher_handle_t> hs(layers, compress);
      hs[0] = leaves;
      h = icicle_merkle_tree_create(hs.data(), hs.size(), element_bytes, store_min);
      return h != nullptr;
    }
  };

  static FriLabels labels_of(const icicle_fri_transcript_config_t* t)
  {
    return FriLabels{t->domain_separator_label,     t->round_challenge_label,     t->commit_phase_label,     t->nonce_label,     t->public_state,
                     t->domain_separator_label_len, t->round_challenge_label_len, t->commit_phase_label_len, t->nonce_label_len, t->public_state_len};
  }

  static icicle_error_t transcript_hash(icicle_hasher_handle_t hasher, const std::vector<uint8_t>& msg, hipStream_t st, std::vector<uint8_t>* digest)
  {
    if (msg.empty()) return ICICLE_INVALID_ARGUMENT;
    digest->assign(icicle_hasher_output_size(hasher), 0);
    icicle_hash_config_t hc{};
    hc.stream = (icicleStreamHandle)st, hc.batch = 1;
    return icicle_hasher_hash(hasher, msg.data(), msg.size(), &hc, digest->data());
  }

  // The checks of the configuration and the hashers that both entry points share; arguments only, the device is not touched.
  static icicle_error_t check_config(const icicle_fri_config_t* cfg, icicle_hasher_handle_t leaves, icicle_hasher_handle_t compress, int words)
  {
    if (fri_check_config(cfg->folding_factor, cfg->stopping_degree, cfg->nof_queries, hasher_default_chunk(compress), icicle_hasher_output_size(compress)))
      return ICICLE_INVALID_ARGUMENT;
    if (hasher_default_chunk(leaves) != 4ull * words) return ICICLE_INVALID_ARGUMENT; // one element per leaf
    if (cfg->pow_bits > 60) return ICICLE_INVALID_ARGUMENT;                          // proof_of_work's own range
    return ICICLE_SUCCESS;
  }
  // false: the size does not fit the configuration (fri_make_plan's rules of the size)
  static bool plan_of(const icicle_fri_config_t* cfg, uint64_t n, icicle_hasher_handle_t compress, FriPlan* plan)
  {
    return fri_make_plan(n, cfg->folding_factor, cfg->stopping_degree, cfg->nof_queries, hasher_default_chunk(compress), icicle_hasher_output_size(compress), plan) == 0;
  }

  template <class PR, int WORDS>
  static icicle_error_t fri_prove(const icicle_fri_config_t* cfg, const icicle_fri_transcript_config_t* tc, const uint32_t* input, size_t n, icicle_hasher_handle_t leaves,
                                  icicle_hasher_handle_t compress, uint64_t store_min, FriProofObj* proof)
  {
    if (!cfg || !tc || !tc->hasher || !tc->seed_rng || !input || !leaves || !compress || !proof) return ICICLE_INVALID_POINTER;
    FriPlan plan;
    ICICLE_TRY(check_config(cfg, leaves, compress, WORDS));
    if (!plan_of(cfg, n, compress, &plan)) return ICICLE_INVALID_ARGUMENT;
    const uint32_t* tw = nullptr;
    int log_max = 0;
    if (!domain_for<PR>(plan.log_n, &tw, &log_max)) return ICICLE_INVALID_ARGUMENT;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    constexpr size_t EB = 4 * WORDS; // bytes of one element

    // every layer in device memory: layer r at a 16-aligned offset of one buffer (a device input is layer 0 where it lies)
    std::vector<uint32_t*> layer(plan.rounds + 1, nullptr);
    std::vector<size_t> off(plan.rounds + 2, 0);
    for (uint32_t r = 0; r <= plan.rounds; r++) {
      const bool own = r > 0 || !cfg->are_inputs_on_device;
      off[r + 1] = off[r] + (own ? (plan.round_size(r) * EB + 15) & ~(size_t)15 : 0);
    }
    TempBuf d_layers;
    HIP_TRY(d_layers.alloc(off[plan.rounds + 1], st), ICICLE_ALLOCATION_FAILED);
    for (uint32_t r = 0; r <= plan.rounds; r++)
      layer[r] = reinterpret_cast<uint32_t*>(d_layers.as<uint8_t>() + off[r]);
    if (cfg->are_inputs_on_device)
      layer[0] = const_cast<uint32_t*>(input);
    else
      HIP_TRY(hipMemcpyAsync(layer[0], input, n * EB, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);

    // commit and fold
    const FriTranscriptBytes transcript(labels_of(tc), plan.log_n);
    icicle_merkle_tree_config_t mc{};
    mc.stream = (icicleStreamHandle)st, mc.is_leaves_on_device = true, mc.is_tree_on_device = true, mc.padding_policy = ICICLE_PADDING_NONE;
    std::vector<TreeHandle> trees(plan.rounds);
    std::vector<uint8_t> digest;
    uint32_t alpha[4] = {0, 0, 0, 0};
    for (uint32_t r = 0; r < plan.rounds; r++) {
      if (!trees[r].create(leaves, compress, plan.tree_layers(r), EB, store_min)) return ICICLE_INVALID_ARGUMENT;
      ICICLE_TRY(icicle_merkle_tree_build(trees[r].h, reinterpret_cast<const uint8_t*>(layer[r]), plan.round_size(r) * EB, &mc)); // returns with the root on the host
      size_t root_size = 0;
      const uint8_t* root = icicle_merkle_tree_get_root(trees[r].h, &root_size);
      if (!root || !root_size) return ICICLE_INVALID_ARGUMENT;
      const uint8_t* prev = reinterpret_cast<const uint8_t*>(r == 0 ? tc->seed_rng : alpha);
      ICICLE_TRY(transcript_hash(tc->hasher, transcript.round_input(prev, EB, root, root_size), st, &digest));
      fri_field_from_digest(digest.data(), digest.size(), PR::P, WORDS, alpha);
      ICICLE_TRY((fold_launch<PR, WORDS>(layer[r], layer[r + 1], plan.log_n - r, alpha, tw, log_max, st)));
    }
    std::vector<uint32_t> final_poly(plan.final_size * WORDS);
    HIP_TRY(hipMemcpyAsync(final_poly.data(), layer[plan.rounds], plan.final_size * EB, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
    HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);

    // proof of work over entry0 | alpha_last | nonce_label
    uint64_t nonce = 0;
    if (cfg->pow_bits != 0) {
      const std::vector<uint8_t> challenge = transcript.pow_challenge(reinterpret_cast<const uint8_t*>(alpha), EB);
      icicle_pow_config_t pc{};
      pc.stream = (icicleStreamHandle)st, pc.padding_size = 24;
      bool found = false;
      uint64_t mined = 0;
      ICICLE_TRY(proof_of_work(tc->hasher, challenge.data(), (uint32_t)challenge.size(), (uint8_t)cfg->pow_bits, &pc, &found, &nonce, &mined));
      if (!found) return ICICLE_INVALID_ARGUMENT;
    }

    // query phase
    ICICLE_TRY(transcript_hash(tc->hasher, transcript.query_input(cfg->pow_bits != 0, reinterpret_cast<const uint8_t*>(alpha), EB, nonce), st, &digest));
    const std::vector<uint64_t> queries = fri_draw_queries(digest.data(), cfg->nof_queries, plan.final_size, plan.n);
    FriProofObj fresh;
    fresh.slots.assign(2 * queries.size(), std::vector<icicle_merkle_proof_handle_t>(plan.rounds, nullptr));
    for (size_t j = 0; j < queries.size(); j++)
      for (uint32_t r = 0; r < plan.rounds; r++)
        for (int sym = 0; sym < 2; sym++) {
          icicle_merkle_proof_handle_t mp = icicle_merkle_proof_create();
          if (!mp) return ICICLE_ALLOCATION_FAILED;
          fresh.slots[2 * j + sym][r] = mp;
          ICICLE_TRY(icicle_merkle_tree_get_proof(trees[r].h, reinterpret_cast<const uint8_t*>(layer[r]), plan.round_size(r) * EB,
                                                  fri_leaf_index(queries[j], plan.round_size(r), sym != 0), false, &mc, mp));
        }
    HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    proof->clear();
    proof->slots.swap(fresh.slots);
    proof->final_poly.swap(final_poly);
    proof->nonce = nonce;
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

  template <class PR, int WORDS>
  static icicle_error_t fri_verify(const icicle_fri_config_t* cfg, const icicle_fri_transcript_config_t* tc, const FriProofObj* proof, icicle_hasher_handle_t leaves,
                                   icicle_hasher_handle_t compress, bool* valid)
  {
    using S = SmallField<PR>;
    if (!cfg || !tc || !tc->hasher || !tc->seed_rng || !proof || !leaves || !compress || !valid) return ICICLE_INVALID_POINTER;
    *valid = false;
    constexpr size_t EB = 4 * WORDS;
    ICICLE_TRY(check_config(cfg, leaves, compress, WORDS)); // the caller's arguments: errors
    // From here on everything is the proof's: whatever does not fit is a wrong proof, *valid = false with SUCCESS. The final
    // polynomial's length first (a longer one is a degree attack), then the proof's shape against the configuration.
    const uint64_t final_size = proof->final_poly.size() / WORDS;
    if (final_size != cfg->stopping_degree + 1) return ICICLE_SUCCESS;
    if (proof->slots.size() != 2 * cfg->nof_queries || proof->slots[0].empty()) return ICICLE_SUCCESS;
    const uint64_t rounds = proof->slots[0].size();
    FriPlan plan;
    if (rounds + fri_log2(final_size) > 31 || !plan_of(cfg, final_size << rounds, compress, &plan)) return ICICLE_SUCCESS;
    for (const auto& q : proof->slots) {
      if (q.size() != rounds) return ICICLE_SUCCESS;
      for (auto p : q)
        if (!p) return ICICLE_SUCCESS;
    }
    // one tree per round: every slot of a round carries the root the challenge is derived from (the reference compares each Merkle
    // proof only with the root that proof itself carries, so a forger could open each query against a tree of its own)
    for (uint32_t r = 0; r < rounds; r++) {
      size_t size0 = 0, size = 0;
      const uint8_t* root0 = icicle_merkle_proof_get_root(proof->slots[0][r], &size0);
      if (!root0 || !size0) return ICICLE_SUCCESS;
      for (const auto& q : proof->slots) {
        const uint8_t* root = icicle_merkle_proof_get_root(q[r], &size);
        if (!root || size != size0 || std::memcmp(root, root0, size0) != 0) return ICICLE_SUCCESS;
      }
    }
    for (uint32_t v : proof->final_poly)
      if (v >= PR::P) return ICICLE_SUCCESS;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;

    // alphas from the roots the proof carries
    const FriTranscriptBytes transcript(labels_of(tc), plan.log_n);
    std::vector<uint32_t> alphas(rounds * WORDS);
    std::vector<uint8_t> digest;
    const uint8_t* prev = reinterpret_cast<const uint8_t*>(tc->seed_rng);
    for (uint32_t r = 0; r < rounds; r++) {
      size_t root_size = 0;
      const uint8_t* root = icicle_merkle_proof_get_root(proof->slots[0][r], &root_size);
      if (!root || !root_size) return ICICLE_SUCCESS;
      ICICLE_TRY(transcript_hash(tc->hasher, transcript.round_input(prev, EB, root, root_size), st, &digest));
      fri_field_from_digest(digest.data(), digest.size(), PR::P, WORDS, &alphas[r * WORDS]);
      prev = reinterpret_cast<const uint8_t*>(&alphas[r * WORDS]);
    }
    if (cfg->pow_bits != 0) {
      const std::vector<uint8_t> challenge = transcript.pow_challenge(prev, EB);
      icicle_pow_config_t pc{};
      pc.stream = (icicleStreamHandle)st, pc.padding_size = 24;
      bool ok = false;
      uint64_t mined = 0;
      ICICLE_TRY(proof_of_work_verify(tc->hasher, challenge.data(), (uint32_t)challenge.size(), (uint8_t)cfg->pow_bits, &pc, proof->nonce, &ok, &mined));
      if (!ok) return ICICLE_SUCCESS;
    }
    ICICLE_TRY(transcript_hash(tc->hasher, transcript.query_input(cfg->pow_bits != 0, prev, EB, proof->nonce), st, &digest));
    const std::vector<uint64_t> queries = fri_draw_queries(digest.data(), cfg->nof_queries, plan.final_size, plan.n);

    // w_n^(-1) from the field's own root of unity, 1/2, both Montgomery
    uint32_t w = S::to_mont(PR::ROU);
    for (int i = 0; i < PR::TWO_ADICITY - (int)plan.log_n; i++)
      w = S::mul(w, w);
    const uint32_t w_inv = S::inv(w), half = S::to_mont((PR::P + 1) / 2);

    std::vector<TreeHandle> trees(rounds);
    for (uint32_t r = 0; r < rounds; r++)
      if (!trees[r].create(leaves, compress, plan.tree_layers(r), EB, 0)) return ICICLE_INVALID_ARGUMENT;
    for (size_t j = 0; j < queries.size(); j++)
      for (uint32_t r = 0; r < rounds; r++) {
        const uint64_t size = plan.round_size(r), idx = fri_leaf_index(queries[j], size, false), idx_sym = fri_leaf_index(queries[j], size, true);
        icicle_merkle_proof_handle_t mp[2] = {proof->slots[2 * j][r], proof->slots[2 * j + 1][r]};
        const uint8_t* leaf[2];
        uint64_t leaf_idx[2];
        for (int s = 0; s < 2; s++) {
          bool ok = false;
          const icicle_error_t e = icicle_merkle_tree_verify(trees[r].h, mp[s], &ok);
          if (e == ICICLE_INVALID_ARGUMENT) return ICICLE_SUCCESS; // a proof that does not fit the tree's shape
          ICICLE_TRY(e);
          if (!ok) return ICICLE_SUCCESS;
          size_t leaf_size = 0;
          leaf[s] = icicle_merkle_proof_get_leaf(mp[s], &leaf_size, &leaf_idx[s]);
          if (!leaf[s] || leaf_size != EB) return ICICLE_SUCCESS;
        }
        if (leaf_idx[0] != idx || leaf_idx[1] != idx_sym) return ICICLE_SUCCESS;
        // collinearity: (a + b)/2 + alpha * ((a - b)/2 * w_n^(-idx 2^r)) is the next round's leaf (or the final polynomial's value)
        uint32_t a[4], b[4], odd[4], folded[4];
        std::memcpy(a, leaf[0], EB), std::memcpy(b, leaf[1], EB);
        const uint32_t twh = S::mul(S::pow(w_inv, idx << r), half);
        for (int q = 0; q < WORDS; q++) {
          if (a[q] >= PR::P || b[q] >= PR::P) return ICICLE_SUCCESS;
          odd[q] = S::mul(S::sub(a[q], b[q]), twh);
        }
        field_mul<PR, WORDS>(odd, &alphas[r * WORDS], folded);
        for (int q = 0; q < WORDS; q++)
          folded[q] = S::add(folded[q], S::mul(S::add(a[q], b[q]), half));
        const uint8_t* expect;
        if (r + 1 == rounds) {
          expect = reinterpret_cast<const uint8_t*>(&proof->final_poly[(queries[j] % final_size) * WORDS]);
        } else {
          size_t next_size = 0;
          uint64_t next_idx = 0;
          expect = icicle_merkle_proof_get_leaf(proof->slots[2 * j][r + 1], &next_size, &next_idx);
          if (!expect || next_size != EB) return ICICLE_SUCCESS;
        }
        if (std::memcmp(expect, folded, EB) != 0) return ICICLE_SUCCESS;
      }
    *valid = true;
    return ICICLE_SUCCESS;
  }

} // namespace icicle_hip

using namespace icicle_hip;

static_assert(sizeof(icicle_fri_config_t) == 56 && offsetof(icicle_fri_config_t, folding_factor) == 8 && offsetof(icicle_fri_config_t, nof_queries) == 32 &&
                offsetof(icicle_fri_config_t, are_inputs_on_device) == 40 && offsetof(icicle_fri_config_t, is_async) == 41 && offsetof(icicle_fri_config_t, ext) == 48,
              "FriConfig layout (include/icicle/fri/fri_config.h)");
static_assert(sizeof(icicle_fri_transcript_config_t) == 96 && offsetof(icicle_fri_transcript_config_t, public_state) == 72 &&
                offsetof(icicle_fri_transcript_config_t, seed_rng) == 88,
              "FFIFriTranscriptConfig layout (src/fri/fri_c_api.cpp)");

#define FRI_GUARDED(expr)                                                                                              \
  try {                                                                                                                \
    return (expr);                                                                                                     \
  } catch (...) {                                                                                                      \
    return ICICLE_ALLOCATION_FAILED;                                                                                   \
  }

#define DEFINE_FRI(P, PR, WORDS)                                                                                       \
  extern "C" icicle_fri_proof_handle_t P##_icicle_initialize_fri_proof(void) { return (icicle_fri_proof_handle_t) new (std::nothrow) FriProofObj; } \
  extern "C" icicle_fri_proof_handle_t P##_icicle_create_with_arguments_fri_proof(icicle_merkle_proof_handle_t** query_proofs, size_t nof_queries, size_t nof_rounds, \
                                                                                  const uint32_t* final_poly, size_t final_poly_size, uint64_t pow_nonce) \
  {                                                                                                                    \
    try {                                                                                                              \
      return (icicle_fri_proof_handle_t)proof_from_arguments(query_proofs, nof_queries, nof_rounds, final_poly, final_poly_size, pow_nonce, WORDS); \
    } catch (...) {                                                                                                    \
      return nullptr;                                                                                                  \
    }                                                                                                                  \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_icicle_delete_fri_proof(icicle_fri_proof_handle_t proof)                               \
  {                                                                                                                    \
    if (!proof) return ICICLE_INVALID_POINTER;                                                                         \
    delete (FriProofObj*)proof;                                                                                        \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_nof_queries(icicle_fri_proof_handle_t proof, size_t* nof_queries)        \
  {                                                                                                                    \
    if (!proof || !nof_queries) return ICICLE_INVALID_POINTER;                                                         \
    *nof_queries = ((const FriProofObj*)proof)->slots.size();                                                          \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_nof_rounds(icicle_fri_proof_handle_t proof, size_t* nof_rounds)          \
  {                                                                                                                    \
    if (!proof || !nof_rounds) return ICICLE_INVALID_POINTER;                                                          \
    const FriProofObj* p = (const FriProofObj*)proof;                                                                  \
    *nof_rounds = p->slots.empty() ? 0 : p->slots[0].size();                                                           \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_round_proofs_for_query(icicle_fri_proof_handle_t proof, size_t query_idx, icicle_merkle_proof_handle_t* proofs) \
  {                                                                                                                    \
    if (!proof || !proofs) return ICICLE_INVALID_POINTER;                                                              \
    const FriProofObj* p = (const FriProofObj*)proof;                                                                  \
    if (query_idx >= p->slots.size()) return ICICLE_INVALID_ARGUMENT;                                                  \
    for (size_t r = 0; r < p->slots[query_idx].size(); r++)                                                            \
      proofs[r] = p->slots[query_idx][r];                                                                              \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_final_poly_size(icicle_fri_proof_handle_t proof, size_t* result)         \
  {                                                                                                                    \
    if (!proof || !result) return ICICLE_INVALID_POINTER;                                                              \
    *result = ((const FriProofObj*)proof)->final_poly.size() / WORDS;                                                  \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_final_poly(icicle_fri_proof_handle_t proof, uint32_t** final_poly)       \
  {                                                                                                                    \
    if (!proof || !final_poly) return ICICLE_INVALID_POINTER;                                                          \
    *final_poly = ((FriProofObj*)proof)->final_poly.data();                                                            \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_pow_nonce(icicle_fri_proof_handle_t proof, uint64_t* result)             \
  {                                                                                                                    \
    if (!proof || !result) return ICICLE_INVALID_POINTER;                                                              \
    *result = ((const FriProofObj*)proof)->nonce;                                                                      \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_merkle_tree_prove(const icicle_fri_config_t* fri_config, const icicle_fri_transcript_config_t* transcript_config,           \
                                                      const uint32_t* input_data, size_t input_size, icicle_hasher_handle_t merkle_tree_leaves_hash,            \
                                                      icicle_hasher_handle_t merkle_tree_compress_hash, uint64_t output_store_min_layer,                        \
                                                      icicle_fri_proof_handle_t fri_proof)                             \
  {                                                                                                                    \
    FRI_GUARDED((fri_prove<PR, WORDS>(fri_config, transcript_config, input_data, input_size, merkle_tree_leaves_hash, merkle_tree_compress_hash,               \
                                      output_store_min_layer, (FriProofObj*)fri_proof)))                               \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_merkle_tree_verify(const icicle_fri_config_t* fri_config, const icicle_fri_transcript_config_t* transcript_config,          \
                                                       icicle_fri_proof_handle_t fri_proof, icicle_hasher_handle_t merkle_tree_leaves_hash,                     \
                                                       icicle_hasher_handle_t merkle_tree_compress_hash, bool* valid)  \
  {                                                                                                                    \
    FRI_GUARDED((fri_verify<PR, WORDS>(fri_config, transcript_config, (const FriProofObj*)fri_proof, merkle_tree_leaves_hash, merkle_tree_compress_hash, valid))) \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_hip_fri_fold(const uint32_t* in, uint64_t n, const uint32_t* alpha, uint32_t* out, bool on_device, icicleStreamHandle stream)   \
  {                                                                                                                    \
    FRI_GUARDED((fold_run<PR, WORDS>(in, n, alpha, out, on_device, (hipStream_t)stream)))                              \
  }
DEFINE_FRI(babybear, babybear_params, 1)
DEFINE_FRI(babybear_extension, babybear_params, 4)
DEFINE_FRI(koalabear, koalabear_params, 1)
DEFINE_FRI(koalabear_extension, koalabear_params, 4)
