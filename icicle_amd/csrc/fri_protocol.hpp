// The FRI protocol over any field kind: the proof object, the prover and the verifier of the reference's C ABI
// (src/fri/fri_c_api.cpp), composed from what hash.hip and merkle.hip provide -- the query phase and the verifier on its batched openings and
// verification, one call per round --, and the macro that defines a prefix's entry points. Included by
// fri.hip (the 31-bit fields) and fri_wide.hip (Goldilocks, the 256-bit fields), which supply the field kind K:
//
//   K::WORDS                                      uint32 words of one element in memory (canonical, little-endian)
//   K::Domain, K::domain_for(k, &d)               the current device's twiddle table; false: none, or one smaller than 2^k
//   K::fold_launch(in, out, k, alpha, d, stream)  the fold kernel: 2^k elements -> 2^(k-1), both on the device, alpha canonical words
//   K::from_digest(digest, len, out)              F(digest) of the transcript
//   K::canonical(e)                               every coefficient of the element below p
//   K::Collinear(log_n).fold(a, b, alpha, e, out) the host's (a + b)/2 + alpha * ((a - b)/2 * w_n^(-e)), canonical words
//
// Reference semantics: backend/cpu/include/cpu_fri_backend.h:76-190 (commit-fold phase, proof of work, query phase),
// src/fri/fri.cpp:49-99,283-319 (verify), include/icicle/fri/fri_transcript.h (Fiat-Shamir). The host-only rules -- parameter
// checks, shapes, transcript bytes, sampler -- are in fri_plan.h.
#pragma once
#include "common.h"
#include "fri_plan.h"
#include <cstring>
#include <memory>
#include <new>

namespace icicle_hip {

  constexpr int FRI_MAX_WORDS = 8; // the widest element: a 256-bit scalar

  template <class K>
  static icicle_error_t fold_run(const uint32_t* in, uint64_t n, const uint32_t* alpha, uint32_t* out, bool on_device, hipStream_t st)
  {
    constexpr int WORDS = K::WORDS;
    if (!in || !alpha || !out) return ICICLE_INVALID_POINTER;
    if (n < 2 || !fri_is_pow2(n)) return ICICLE_INVALID_ARGUMENT;
    const uint32_t k = fri_log2(n);
    typename K::Domain dom;
    if (!K::domain_for(k, &dom)) return ICICLE_INVALID_ARGUMENT;
    ICICLE_TRY(bind_current_device());
    const size_t in_bytes = (size_t)n * WORDS * 4, out_bytes = in_bytes / 2;
    uint32_t a[FRI_MAX_WORDS] = {0};
    if (on_device) {
      HIP_TRY(hipMemcpyAsync(a, alpha, WORDS * 4, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
      HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
      return K::fold_launch(in, out, k, a, dom, st);
    }
    std::memcpy(a, alpha, WORDS * 4);
    TempBuf d_in, d_out;
    HIP_TRY(d_in.alloc(in_bytes, st), ICICLE_ALLOCATION_FAILED);
    HIP_TRY(d_out.alloc(out_bytes, st), ICICLE_ALLOCATION_FAILED);
    HIP_TRY(hipMemcpyAsync(d_in.ptr(), in, in_bytes, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
    ICICLE_TRY(K::fold_launch(d_in.as<uint32_t>(), d_out.as<uint32_t>(), k, a, dom, st));
    HIP_TRY(hipMemcpyAsync(out, d_out.ptr(), out_bytes, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
    HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    return ICICLE_SUCCESS;
  }

  // ---- the proof object -----------------------------------------------------------------------------------------------------------
  // slots[q][r]: Merkle proofs owned by the FRI proof (handles of merkle.hip's proof type, so icicle_merkle_proof_get_* read them)
  struct FriProofObj {
    std::vector<std::vector<icicle_merkle_proof_handle_t>> slots;
    std::vector<uint32_t> final_poly; // the elements' words back to back (K::WORDS per element)
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

  template <class K>
  static icicle_error_t fri_prove(const icicle_fri_config_t* cfg, const icicle_fri_transcript_config_t* tc, const uint32_t* input, size_t n, icicle_hasher_handle_t leaves,
                                  icicle_hasher_handle_t compress, uint64_t store_min, FriProofObj* proof)
  {
    constexpr int WORDS = K::WORDS;
    if (!cfg || !tc || !tc->hasher || !tc->seed_rng || !input || !leaves || !compress || !proof) return ICICLE_INVALID_POINTER;
    FriPlan plan;
    ICICLE_TRY(check_config(cfg, leaves, compress, WORDS));
    if (!plan_of(cfg, n, compress, &plan)) return ICICLE_INVALID_ARGUMENT;
    typename K::Domain dom;
    if (!K::domain_for(plan.log_n, &dom)) return ICICLE_INVALID_ARGUMENT;
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
    uint32_t alpha[FRI_MAX_WORDS] = {0};
    for (uint32_t r = 0; r < plan.rounds; r++) {
      if (!trees[r].create(leaves, compress, plan.tree_layers(r), EB, store_min)) return ICICLE_INVALID_ARGUMENT;
      ICICLE_TRY(icicle_merkle_tree_build(trees[r].h, reinterpret_cast<const uint8_t*>(layer[r]), plan.round_size(r) * EB, &mc)); // returns with the root on the host
      size_t root_size = 0;
      const uint8_t* root = icicle_merkle_tree_get_root(trees[r].h, &root_size);
      if (!root || !root_size) return ICICLE_INVALID_ARGUMENT;
      const uint8_t* prev = reinterpret_cast<const uint8_t*>(r == 0 ? tc->seed_rng : alpha);
      ICICLE_TRY(transcript_hash(tc->hasher, transcript.round_input(prev, EB, root, root_size), st, &digest));
      K::from_digest(digest.data(), digest.size(), alpha);
      ICICLE_TRY(K::fold_launch(layer[r], layer[r + 1], plan.log_n - r, alpha, dom, st));
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
    // one batch of openings per round: the round's 2 * nof_queries leaf indices in slot order (query, symmetric)
    FriProofObj fresh;
    fresh.slots.assign(2 * queries.size(), std::vector<icicle_merkle_proof_handle_t>(plan.rounds, nullptr));
    std::vector<uint64_t> indices(2 * queries.size());
    std::vector<icicle_merkle_proof_handle_t> opened(2 * queries.size());
    for (uint32_t r = 0; r < plan.rounds; r++) {
      for (size_t s = 0; s < opened.size(); s++) {
        if (!(opened[s] = fresh.slots[s][r] = icicle_merkle_proof_create())) return ICICLE_ALLOCATION_FAILED;
        indices[s] = fri_leaf_index(queries[s / 2], plan.round_size(r), (s & 1) != 0);
      }
      ICICLE_TRY(icicle_hip_merkle_tree_get_proofs(trees[r].h, reinterpret_cast<const uint8_t*>(layer[r]), plan.round_size(r) * EB, indices.data(), indices.size(), false,
                                                   &mc, opened.data()));
    }
    HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    proof->clear();
    proof->slots.swap(fresh.slots);
    proof->final_poly.swap(final_poly);
    proof->nonce = nonce;
    return ICICLE_SUCCESS;
  }

  template <class K>
  static icicle_error_t fri_verify(const icicle_fri_config_t* cfg, const icicle_fri_transcript_config_t* tc, const FriProofObj* proof, icicle_hasher_handle_t leaves,
                                   icicle_hasher_handle_t compress, bool* valid)
  {
    constexpr int WORDS = K::WORDS;
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
    for (uint64_t i = 0; i < final_size; i++)
      if (!K::canonical(&proof->final_poly[i * WORDS])) return ICICLE_SUCCESS;
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
      K::from_digest(digest.data(), digest.size(), &alphas[r * WORDS]);
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

    const typename K::Collinear line(plan.log_n); // w_n^(-1) from the field's own root of unity: no domain needed

    std::vector<TreeHandle> trees(rounds);
    for (uint32_t r = 0; r < rounds; r++)
      if (!trees[r].create(leaves, compress, plan.tree_layers(r), EB, 0)) return ICICLE_INVALID_ARGUMENT;
    // every Merkle proof of a round in one batch; a proof that does not fit the tree's shape (INVALID_ARGUMENT) is a wrong proof.
    // A batch shares one pruned flag, so a proof object that mixes pruned and full openings takes one batch per flag.
    std::vector<icicle_merkle_proof_handle_t> batch;
    std::vector<uint8_t> batch_ok; // bool, with an address
    for (uint32_t r = 0; r < rounds; r++)
      for (int flag = 0; flag < 2; flag++) {
        batch.clear();
        for (const auto& q : proof->slots)
          if (icicle_merkle_proof_is_pruned(q[r]) == (flag != 0)) batch.push_back(q[r]);
        if (batch.empty()) continue;
        batch_ok.assign(batch.size(), 0);
        const icicle_error_t e = icicle_hip_merkle_tree_verify_batch(trees[r].h, batch.data(), batch.size(), reinterpret_cast<bool*>(batch_ok.data()));
        if (e == ICICLE_INVALID_ARGUMENT) return ICICLE_SUCCESS;
        ICICLE_TRY(e);
        for (uint8_t ok : batch_ok)
          if (!ok) return ICICLE_SUCCESS;
      }
    for (size_t j = 0; j < queries.size(); j++)
      for (uint32_t r = 0; r < rounds; r++) {
        const uint64_t size = plan.round_size(r), idx = fri_leaf_index(queries[j], size, false), idx_sym = fri_leaf_index(queries[j], size, true);
        icicle_merkle_proof_handle_t mp[2] = {proof->slots[2 * j][r], proof->slots[2 * j + 1][r]};
        const uint8_t* leaf[2];
        uint64_t leaf_idx[2];
        for (int s = 0; s < 2; s++) {
          size_t leaf_size = 0;
          leaf[s] = icicle_merkle_proof_get_leaf(mp[s], &leaf_size, &leaf_idx[s]);
          if (!leaf[s] || leaf_size != EB) return ICICLE_SUCCESS;
        }
        if (leaf_idx[0] != idx || leaf_idx[1] != idx_sym) return ICICLE_SUCCESS;
        // collinearity: (a + b)/2 + alpha * ((a - b)/2 * w_n^(-idx 2^r)) is the next round's leaf (or the final polynomial's value)
        uint32_t a[FRI_MAX_WORDS], b[FRI_MAX_WORDS], folded[FRI_MAX_WORDS];
        std::memcpy(a, leaf[0], EB), std::memcpy(b, leaf[1], EB);
        if (!K::canonical(a) || !K::canonical(b)) return ICICLE_SUCCESS;
        line.fold(a, b, &alphas[r * WORDS], idx << r, folded);
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

// the entry points of prefix P over the field kind KIND (a type name without commas: an alias)
#define DEFINE_FRI(P, KIND)                                                                                            \
  extern "C" icicle_fri_proof_handle_t P##_icicle_initialize_fri_proof(void) { return (icicle_fri_proof_handle_t) new (std::nothrow) icicle_hip::FriProofObj; } \
  extern "C" icicle_fri_proof_handle_t P##_icicle_create_with_arguments_fri_proof(icicle_merkle_proof_handle_t** query_proofs, size_t nof_queries, size_t nof_rounds, \
                                                                                  const uint32_t* final_poly, size_t final_poly_size, uint64_t pow_nonce) \
  {                                                                                                                    \
    try {                                                                                                              \
      return (icicle_fri_proof_handle_t)icicle_hip::proof_from_arguments(query_proofs, nof_queries, nof_rounds, final_poly, final_poly_size, pow_nonce, KIND::WORDS); \
    } catch (...) {                                                                                                    \
      return nullptr;                                                                                                  \
    }                                                                                                                  \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_icicle_delete_fri_proof(icicle_fri_proof_handle_t proof)                               \
  {                                                                                                                    \
    if (!proof) return ICICLE_INVALID_POINTER;                                                                         \
    delete (icicle_hip::FriProofObj*)proof;                                                                            \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_nof_queries(icicle_fri_proof_handle_t proof, size_t* nof_queries)        \
  {                                                                                                                    \
    if (!proof || !nof_queries) return ICICLE_INVALID_POINTER;                                                         \
    *nof_queries = ((const icicle_hip::FriProofObj*)proof)->slots.size();                                              \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_nof_rounds(icicle_fri_proof_handle_t proof, size_t* nof_rounds)          \
  {                                                                                                                    \
    if (!proof || !nof_rounds) return ICICLE_INVALID_POINTER;                                                          \
    const icicle_hip::FriProofObj* p = (const icicle_hip::FriProofObj*)proof;                                          \
    *nof_rounds = p->slots.empty() ? 0 : p->slots[0].size();                                                           \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_round_proofs_for_query(icicle_fri_proof_handle_t proof, size_t query_idx, icicle_merkle_proof_handle_t* proofs) \
  {                                                                                                                    \
    if (!proof || !proofs) return ICICLE_INVALID_POINTER;                                                              \
    const icicle_hip::FriProofObj* p = (const icicle_hip::FriProofObj*)proof;                                          \
    if (query_idx >= p->slots.size()) return ICICLE_INVALID_ARGUMENT;                                                  \
    for (size_t r = 0; r < p->slots[query_idx].size(); r++)                                                            \
      proofs[r] = p->slots[query_idx][r];                                                                              \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_final_poly_size(icicle_fri_proof_handle_t proof, size_t* result)         \
  {                                                                                                                    \
    if (!proof || !result) return ICICLE_INVALID_POINTER;                                                              \
    *result = ((const icicle_hip::FriProofObj*)proof)->final_poly.size() / KIND::WORDS;                                \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_final_poly(icicle_fri_proof_handle_t proof, uint32_t** final_poly)       \
  {                                                                                                                    \
    if (!proof || !final_poly) return ICICLE_INVALID_POINTER;                                                          \
    *final_poly = ((icicle_hip::FriProofObj*)proof)->final_poly.data();                                                \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_proof_get_pow_nonce(icicle_fri_proof_handle_t proof, uint64_t* result)             \
  {                                                                                                                    \
    if (!proof || !result) return ICICLE_INVALID_POINTER;                                                              \
    *result = ((const icicle_hip::FriProofObj*)proof)->nonce;                                                          \
    return ICICLE_SUCCESS;                                                                                             \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_merkle_tree_prove(const icicle_fri_config_t* fri_config, const icicle_fri_transcript_config_t* transcript_config,           \
                                                      const uint32_t* input_data, size_t input_size, icicle_hasher_handle_t merkle_tree_leaves_hash,            \
                                                      icicle_hasher_handle_t merkle_tree_compress_hash, uint64_t output_store_min_layer,                        \
                                                      icicle_fri_proof_handle_t fri_proof)                             \
  {                                                                                                                    \
    FRI_GUARDED((icicle_hip::fri_prove<KIND>(fri_config, transcript_config, input_data, input_size, merkle_tree_leaves_hash, merkle_tree_compress_hash,        \
                                             output_store_min_layer, (icicle_hip::FriProofObj*)fri_proof)))            \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_fri_merkle_tree_verify(const icicle_fri_config_t* fri_config, const icicle_fri_transcript_config_t* transcript_config,          \
                                                       icicle_fri_proof_handle_t fri_proof, icicle_hasher_handle_t merkle_tree_leaves_hash,                     \
                                                       icicle_hasher_handle_t merkle_tree_compress_hash, bool* valid)  \
  {                                                                                                                    \
    FRI_GUARDED((icicle_hip::fri_verify<KIND>(fri_config, transcript_config, (const icicle_hip::FriProofObj*)fri_proof, merkle_tree_leaves_hash,               \
                                              merkle_tree_compress_hash, valid)))                                      \
  }                                                                                                                    \
  extern "C" icicle_error_t P##_hip_fri_fold(const uint32_t* in, uint64_t n, const uint32_t* alpha, uint32_t* out, bool on_device, icicleStreamHandle stream)   \
  {                                                                                                                    \
    FRI_GUARDED((icicle_hip::fold_run<KIND>(in, n, alpha, out, on_device, (hipStream_t)stream)))                       \
  }
