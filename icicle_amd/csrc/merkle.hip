// Merkle trees over the device hashers (hash.hip; Poseidon2 and Poseidon through the same hasher: poseidon2.hip, poseidon.hip): the
// build, openings and verification. There is one opening path and one verification path for any number of proofs
// (icicle_hip_merkle_tree_get_proofs, icicle_hip_merkle_tree_verify_batch: one gather launch for all openings, one hash launch per
// layer for all verifications; this backend's own); the reference's icicle_merkle_tree_get_proof and icicle_merkle_tree_verify are
// those two with count == 1. The tree's arithmetic is merkle_plan.h, the leaf-index arithmetic of an opening merkle_batch.h. What this
// file needs of the hashers -- struct Hasher, launch_batch, launch_leaves, the fused top's launcher -- is hash_merkle.h; every hash
// kernel, k_merkle_top included, is in hash.hip.
//
// C ABI of the reference: icicle/src/hash/merkle_c_api.cpp (icicle_merkle_tree_*, icicle_merkle_proof_*); config
// include/icicle/merkle/merkle_tree_config.h; tree / proof semantics backend/cpu/src/hash/cpu_merkle_tree.cpp:143-211,546-573 and
// include/icicle/merkle/merkle_tree.h:148-203.
#include "hash_merkle.h"
#include "merkle_batch.h"
#include <cstring>
#include <new>

namespace icicle_hip {

  // ---- Merkle tree --------------------------------------------------------------------------------------------------------------
  struct Proof {
    bool pruned = false;
    uint64_t leaf_idx = 0;
    std::vector<uint8_t> leaf, root, path;
  };

  struct Tree {
    MerklePlan plan;
    std::vector<Hasher> hashers;
    int store_min = 0;
    bool built = false;
    bool on_device = false;
    uint8_t* d_store = nullptr; // layers store_min .. L-1 (hipMalloc), when the tree stays on the device
    uint8_t* h_store = nullptr; // the same layers in pinned host memory otherwise
    uint8_t* h_root = nullptr;  // pinned, so that an asynchronous build can fill it in stream order
    uint64_t store_off(int i) const { return plan.layers[i].offset - plan.layers[store_min].offset; }
    uint64_t store_bytes() const { return plan.total_bytes - plan.layers[store_min].offset; }
    void release()
    {
      if (d_store) (void)hipFree(d_store);
      if (h_store) (void)hipHostFree(h_store);
      if (h_root) (void)hipHostFree(h_root);
      d_store = h_store = h_root = nullptr;
      built = false;
    }
  };

  static int top_max_of(const icicle_merkle_tree_config_t* cfg)
  {
    int v = MERKLE_TOP_MAX_HASHES;
    if (cfg->ext) v = reinterpret_cast<const ConfigExt*>(cfg->ext)->get_int("hip_merkle_top_max_hashes", v);
    return std::max(0, v);
  }

  // What layer 0 reads: `base` is addressed by byte offsets of the whole tree's leaves (only [.., valid) is ever read), `last`
  // the LastValue element or nullptr.
  struct LeafSource {
    const uint8_t* base;
    uint64_t valid;
    const uint8_t* last;
  };

  // Hashes layers [0, upto) of the (sub-)tree over layer-0 chunks [first, first + count): out[i] takes the digests of layer i in
  // order. Layer 0 goes through the hasher's batch kernel where the chunks lie inside the leaves and through its padded-leaf kernel
  // (k_keccak_leaves, k_blake_leaves, k_blake3_leaf_chunks) where they reach into the padding. From the first layer above it that
  // has at most top_max hashes one k_merkle_top launch does the rest, except that k_merkle_top hashes a Blake3 input as one chunk:
  // a Blake3 layer whose inputs exceed 1024 bytes takes its own launches (chunks, then one per tree level), and the fusion starts
  // above the highest such layer, or not at all.
  static icicle_error_t hash_layers(const Tree& t, const LeafSource& src, uint64_t first, uint64_t count, int upto, uint8_t* const* out, int top_max,
                                    hipStream_t st)
  {
    const MerklePlan& p = t.plan;
    const uint64_t c0 = p.layers[0].chunk, full_chunks = src.valid / c0;
    const uint64_t n_full = first >= full_chunks ? 0 : std::min(count, full_chunks - first);
    ICICLE_TRY(launch_batch(t.hashers[0], src.base + first * c0, c0, c0, n_full, out[0], st));
    ICICLE_TRY(launch_leaves(t.hashers[0], src.base, c0, first + n_full, count - n_full, src.valid, src.last, p.leaf_element_size,
                             out[0] + n_full * p.layers[0].out, st));
    int fuse_from = 1; // first layer with no multi-chunk Blake3 layer and no Poseidon2 or Poseidon layer (k_merkle_top has no case for them) at or above it
    for (int j = 1; j < upto; j++)
      if (t.hashers[j].multi_chunk(p.layers[j].chunk) || hash_kind_is_field(t.hashers[j].kind)) fuse_from = j + 1;
    uint64_t n = count;
    for (int i = 1; i < upto; i++) {
      n /= p.arity(i);
      if (i >= fuse_from && top_max > 0 && n <= (uint64_t)top_max) {
        MerkleTopArgs args;
        args.n = 0;
        uint64_t m = n;
        for (int j = i; j < upto; j++) {
          if (j > i) m /= p.arity(j);
          args.l[args.n++] = MerkleTopLayer{out[j - 1], out[j], (uint32_t)p.layers[j].chunk, (uint32_t)m, (uint32_t)t.hashers[j].rate_words, t.hashers[j].suffix,
                                            t.hashers[j].kind};
        }
        return launch_merkle_top(args, st);
      }
      ICICLE_TRY(launch_batch(t.hashers[i], out[i - 1], p.layers[i].chunk, p.layers[i].chunk, n, out[i], st));
    }
    return ICICLE_SUCCESS;
  }

  static icicle_error_t tree_build(Tree* t, const uint8_t* leaves, uint64_t leaves_size, const icicle_merkle_tree_config_t* cfg)
  {
    if (t->built) return ICICLE_INVALID_ARGUMENT;
    MerklePadding pad;
    if (merkle_padding(t->plan, leaves_size, cfg->padding_policy, &pad)) return ICICLE_INVALID_ARGUMENT;
    ICICLE_TRY(bind_current_device());
    t->release();
    hipStream_t st = (hipStream_t)cfg->stream;
    const MerklePlan& p = t->plan;
    const int L = p.L(), m = t->store_min;
    TempBuf d_leaves_tmp, d_low, d_top;
    const uint8_t* d_leaves = leaves;
    if (!cfg->is_leaves_on_device) {
      HIP_TRY(d_leaves_tmp.alloc(leaves_size, st), ICICLE_ALLOCATION_FAILED);
      HIP_TRY(hipMemcpyAsync(d_leaves_tmp.ptr(), leaves, leaves_size, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
      d_leaves = d_leaves_tmp.as<uint8_t>();
    }
    t->on_device = cfg->is_tree_on_device;
    HIP_TRY(hipHostMalloc((void**)&t->h_root, 64, hipHostMallocDefault), ICICLE_ALLOCATION_FAILED);
    uint8_t* store = nullptr; // device memory the stored layers are computed in
    if (t->on_device) {
      HIP_TRY(hipMalloc((void**)&t->d_store, t->store_bytes()), ICICLE_ALLOCATION_FAILED);
      store = t->d_store;
    } else {
      HIP_TRY(hipHostMalloc((void**)&t->h_store, t->store_bytes(), hipHostMallocDefault), ICICLE_ALLOCATION_FAILED);
      HIP_TRY(d_top.alloc(t->store_bytes(), st), ICICLE_ALLOCATION_FAILED);
      store = d_top.as<uint8_t>();
    }
    if (m > 0) HIP_TRY(d_low.alloc(p.layers[m].offset, st), ICICLE_ALLOCATION_FAILED);
    uint8_t* out[MERKLE_MAX_LAYERS];
    for (int i = 0; i < L; i++)
      out[i] = i < m ? d_low.as<uint8_t>() + p.layers[i].offset : store + t->store_off(i);
    const LeafSource src{d_leaves, leaves_size, cfg->padding_policy == MERKLE_PAD_LAST && pad.pad_bytes ? d_leaves + pad.last_off : nullptr};
    ICICLE_TRY(hash_layers(*t, src, 0, p.layers[0].count, L, out, top_max_of(cfg), st));
    HIP_TRY(hipMemcpyAsync(t->h_root, out[L - 1], p.layers[L - 1].out, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
    if (!t->on_device) HIP_TRY(hipMemcpyAsync(t->h_store, store, t->store_bytes(), hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
    if (!cfg->is_async) HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    t->built = true;
    return ICICLE_SUCCESS;
  }

  // ---- openings and verifications -----------------------------------------------------------------------------------------------
  // Pinned host memory for a call's one upload and one download. hipHostMalloc costs more than a whole batch, so the buffers
  // are kept between calls (and never given back: a handful of them, sized by the largest batch seen).
  class PinnedBuf
  {
  public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf()
    {
      if (!m_slot) return;
      std::lock_guard<std::mutex> lk(mtx());
      m_slot->busy = false;
    }
    hipError_t alloc(size_t bytes)
    {
      std::lock_guard<std::mutex> lk(mtx());
      Slot* pick = nullptr;
      for (Slot* s : pool())
        if (!s->busy && (!pick || s->cap > pick->cap)) pick = s;
      if (!pick) {
        pick = new Slot;
        pool().push_back(pick);
      }
      if (pick->cap < bytes) {
        size_t cap = 1 << 16;
        while (cap < bytes)
          cap *= 2;
        if (pick->p) (void)hipHostFree(pick->p);
        pick->p = nullptr, pick->cap = 0;
        const hipError_t e = hipHostMalloc((void**)&pick->p, cap, hipHostMallocPortable);
        if (e != hipSuccess) return e;
        pick->cap = cap;
      }
      pick->busy = true;
      m_slot = pick;
      return hipSuccess;
    }
    uint8_t* ptr() const { return m_slot->p; }

  private:
    struct Slot {
      uint8_t* p = nullptr;
      size_t cap = 0;
      bool busy = false;
    };
    static std::mutex& mtx()
    {
      static std::mutex m;
      return m;
    }
    static std::vector<Slot*>& pool()
    {
      static std::vector<Slot*>* v = new std::vector<Slot*>; // outlives every caller, the HIP runtime's shutdown included
      return *v;
    }
    Slot* m_slot = nullptr;
  };

  // 16 bytes or fewer from src to dst: one 128-bit access where both sides allow it, bytes otherwise
  __device__ __forceinline__ void copy_unit(uint8_t* dst, const uint8_t* src, uint32_t n)
  {
    if (n == 16 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
      *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    } else {
      for (uint32_t k = 0; k < n; k++)
        dst[k] = src[k];
    }
  }

  // The pieces of `count` proofs into count staging records (merkle_batch.h), one lane per 16 bytes of a record. A piece that is
  // not in device memory (layer[i] or leaves == nullptr) is left to the host.
  struct MerkleGatherArgs {
    MerkleBatchShape shape;
    const uint8_t* layer[MERKLE_MAX_LAYERS]; // layer i's digests: the stored layer, or for i < store_min the re-hashed sub-tree of slot 0
    uint64_t sub_stride;                     // from one slot's re-hashed sub-tree to the next
    const uint8_t* leaves;
    uint64_t leaves_size, last_off;
    uint32_t last_value;
    const uint64_t* idx;  // leaf indices, all inside the capacity
    const uint32_t* slot; // per proof: which re-hashed sub-tree it lies in (store_min > 0)
    uint64_t count;
    uint8_t* stage;
  };

  __global__ __launch_bounds__(256) void k_merkle_gather(const MerkleGatherArgs a)
  {
    const MerkleBatchShape& s = a.shape;
    const uint64_t units = s.stride / 16, total = a.count * units, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
      const uint64_t pr = t / units, off = (t % units) * 16;
      uint64_t q, len, chunk0;
      const int piece = merkle_batch_piece(s, off, &q, &len);
      if (piece < 0 || !merkle_batch_chunk0(s, a.idx[pr], &chunk0)) continue;
      uint64_t n = len - q < 16 ? len - q : 16;
      const uint8_t* src;
      if (piece < s.steps) {
        if (!a.layer[piece]) continue;
        MerkleBatchStep st;
        merkle_batch_step(s, chunk0, piece, &st);
        src = a.layer[piece] + (piece < s.store_min ? a.slot[pr] * a.sub_stride + st.sub_off : st.src_off) + q;
      } else if (!a.leaves) {
        continue;
      } else if (piece == s.steps) { // the part of the chunk that lies inside the leaves
        const uint64_t lo = chunk0 * s.c0 + q;
        if (lo >= a.leaves_size) continue;
        if (a.leaves_size - lo < n) n = a.leaves_size - lo;
        src = a.leaves + lo;
      } else {
        if (!a.last_value) continue;
        src = a.leaves + a.last_off + q;
      }
      copy_unit(a.stage + pr * s.stride + off, src, (uint32_t)n);
    }
  }

  // digest k of a layer (dig + k * o) into its hole in proof k's input of the next layer (in + k * stride + hole[k]); one lane per
  // 16 bytes of a digest
  __global__ __launch_bounds__(256) void k_merkle_scatter(const uint8_t* __restrict__ dig, uint32_t o, uint8_t* __restrict__ in, uint64_t stride,
                                                           const uint32_t* __restrict__ hole, uint64_t n)
  {
    const uint64_t units = (o + 15) / 16, total = n * units, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
      const uint64_t k = t / units;
      const uint32_t q = (uint32_t)(t % units) * 16;
      copy_unit(in + k * stride + hole[k] + q, dig + k * o + q, o - q < 16 ? o - q : 16);
    }
  }

  // `count` proofs of one tree (cpu_merkle_tree.cpp:546-573: the leaf's chunk, per layer the group of digests on the way to the
  // root, the root). Everything that lives on the device -- leaf chunks, the last element, groups of stored or re-hashed layers --
  // is gathered into one staging record per proof in one launch and comes back in one copy behind one synchronisation; host-
  // resident pieces are copied on the host, and a call with none on the device launches nothing. Everything that can be refused is
  // refused before the device is touched or a proof written.
  static icicle_error_t tree_proofs(const Tree* t, const uint8_t* leaves, uint64_t leaves_size, const uint64_t* idx, uint64_t count, bool pruned,
                                    const icicle_merkle_tree_config_t* cfg, Proof* const* proofs)
  {
    if (!t->built) return ICICLE_INVALID_ARGUMENT;
    const MerklePlan& p = t->plan;
    MerklePadding pad;
    if (merkle_padding(p, leaves_size, cfg->padding_policy, &pad)) return ICICLE_INVALID_ARGUMENT;
    const int L = p.L(), m = t->store_min;
    MerkleBatchShape sh;
    merkle_batch_shape(p, pruned, m, &sh);
    std::vector<uint64_t> chunk0(count);
    for (uint64_t i = 0; i < count; i++)
      if (!merkle_batch_chunk0(sh, idx[i], &chunk0[i])) return ICICLE_INVALID_ARGUMENT;
    if (count >= (1ull << 32) || count > (1ull << 40) / sh.stride) return ICICLE_INVALID_ARGUMENT; // a terabyte of staging
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const uint64_t c0 = p.layers[0].chunk, es = p.leaf_element_size;
    const bool dev_leaves = cfg->is_leaves_on_device, last_value = cfg->padding_policy == MERKLE_PAD_LAST && pad.pad_bytes > 0;
    const bool device_pieces = dev_leaves || (L > 1 && (m > 0 || t->on_device));

    // layers below store_min: the distinct sub-trees under layer store_min among the indices, each re-hashed once
    uint64_t sub_count = 1;
    std::vector<uint64_t> subs; // first layer-0 chunk of each, ascending
    std::vector<uint32_t> slot(count, 0);
    if (m > 0) {
      subs.resize(count);
      for (uint64_t i = 0; i < count; i++)
        merkle_batch_subtree(sh, chunk0[i], &subs[i], &sub_count);
      std::sort(subs.begin(), subs.end());
      subs.erase(std::unique(subs.begin(), subs.end()), subs.end());
      for (uint64_t i = 0; i < count; i++)
        slot[i] = (uint32_t)(std::lower_bound(subs.begin(), subs.end(), chunk0[i] / sub_count * sub_count) - subs.begin());
    }

    const uint64_t up_bytes = merkle_batch_pad16(12 * count), stage_bytes = count * sh.stride;
    PinnedBuf pinned;
    TempBuf d_buf, d_sub, d_low;
    const uint8_t* rec0 = nullptr; // the staging records on the host
    if (device_pieces) {
      HIP_TRY(pinned.alloc(up_bytes + stage_bytes), ICICLE_ALLOCATION_FAILED);
      HIP_TRY(d_buf.alloc(up_bytes + stage_bytes, st), ICICLE_ALLOCATION_FAILED);
      std::memcpy(pinned.ptr(), idx, 8 * count);
      std::memcpy(pinned.ptr() + 8 * count, slot.data(), 4 * count);
      HIP_TRY(hipMemcpyAsync(d_buf.ptr(), pinned.ptr(), up_bytes, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
      MerkleGatherArgs args{};
      args.shape = sh;
      for (int i = m; i + 1 < L; i++)
        args.layer[i] = t->on_device ? t->d_store + t->store_off(i) : nullptr;
      if (m > 0) {
        uint64_t low_off[MERKLE_MAX_LAYERS], sub_stride = 0;
        for (int i = 0; i < m; i++) {
          low_off[i] = sub_stride;
          sub_stride += merkle_batch_pad16(sub_count / (p.layers[0].count / p.layers[i].count) * p.layers[i].out);
        }
        HIP_TRY(d_low.alloc(sub_stride * subs.size(), st), ICICLE_ALLOCATION_FAILED);
        const uint64_t sub_leaves = merkle_batch_pad16(sub_count * c0); // host leaves: one region per sub-tree, then the last element
        if (!dev_leaves) HIP_TRY(d_sub.alloc(sub_leaves * subs.size() + es, st), ICICLE_ALLOCATION_FAILED);
        uint8_t* d_last = dev_leaves ? nullptr : d_sub.as<uint8_t>() + sub_leaves * subs.size();
        if (d_last && last_value) HIP_TRY(hipMemcpyAsync(d_last, leaves + pad.last_off, es, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
        const int top_max = top_max_of(cfg);
        for (size_t d = 0; d < subs.size(); d++) {
          LeafSource src{leaves, leaves_size, last_value ? leaves + pad.last_off : nullptr};
          if (!dev_leaves) {
            const uint64_t lo = subs[d] * c0, real = lo >= leaves_size ? 0 : std::min(sub_count * c0, leaves_size - lo);
            uint8_t* region = d_sub.as<uint8_t>() + sub_leaves * d;
            if (real) HIP_TRY(hipMemcpyAsync(region, leaves + lo, real, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
            src.base = reinterpret_cast<const uint8_t*>((uintptr_t)region - lo); // only offsets in [lo, lo + real) are read through it
            src.last = last_value ? d_last : nullptr;
          }
          uint8_t* sub_out[MERKLE_MAX_LAYERS];
          for (int i = 0; i < m; i++)
            sub_out[i] = d_low.as<uint8_t>() + sub_stride * d + low_off[i];
          ICICLE_TRY(hash_layers(*t, src, subs[d], sub_count, m, sub_out, top_max, st));
        }
        for (int i = 0; i < m && i + 1 < L; i++)
          args.layer[i] = d_low.as<uint8_t>() + low_off[i];
        args.sub_stride = sub_stride;
      }
      args.leaves = dev_leaves ? leaves : nullptr;
      args.leaves_size = leaves_size, args.last_off = pad.last_off, args.last_value = last_value ? 1 : 0;
      args.idx = d_buf.as<uint64_t>();
      args.slot = reinterpret_cast<const uint32_t*>(d_buf.as<uint8_t>() + 8 * count);
      args.count = count;
      args.stage = d_buf.as<uint8_t>() + up_bytes;
      k_merkle_gather<<<grid_for(stage_bytes / 16), 256, 0, st>>>(args);
      LAUNCH_CHECK("k_merkle_gather", st);
      HIP_TRY(hipMemcpyAsync(pinned.ptr() + up_bytes, args.stage, stage_bytes, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
      rec0 = pinned.ptr() + up_bytes;
    }
    // the one synchronisation: also orders this call behind an asynchronous build on the same stream (h_store, h_root)
    HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);

    const uint64_t path_size = merkle_batch_path_size(sh);
    for (uint64_t i = 0; i < count; i++) {
      Proof* proof = proofs[i];
      const uint8_t* rec = rec0 ? rec0 + i * sh.stride : nullptr;
      proof->pruned = pruned;
      proof->leaf_idx = idx[i];
      proof->path.assign(path_size, 0);
      for (int l = 0; l + 1 < L; l++) {
        MerkleBatchStep s;
        merkle_batch_step(sh, chunk0[i], l, &s);
        const uint64_t o = p.layers[l].out;
        const uint8_t* g = (l < m || t->on_device) ? rec + sh.stage_at[l] : t->h_store + t->store_off(l) + s.src_off;
        if (pruned) {
          std::memcpy(proof->path.data() + s.dst_off, g, s.skip_off);
          std::memcpy(proof->path.data() + s.dst_off + s.skip_off, g + s.skip_off + o, s.len - s.skip_off - o);
        } else {
          std::memcpy(proof->path.data() + s.dst_off, g, s.len);
        }
      }
      // the leaf chunk, padded per policy
      const uint64_t leaf_lo = chunk0[i] * c0, leaf_real = leaf_lo >= leaves_size ? 0 : std::min(c0, leaves_size - leaf_lo);
      proof->leaf.assign(c0, 0);
      if (leaf_real) std::memcpy(proof->leaf.data(), dev_leaves ? rec + sh.leaf_at : leaves + leaf_lo, leaf_real);
      if (last_value) {
        const uint8_t* last = dev_leaves ? rec + sh.last_at : leaves + pad.last_off;
        for (uint64_t q = leaf_real; q < c0; q++)
          proof->leaf[q] = last[(leaf_lo + q) % es];
      }
      proof->root.assign(t->h_root, t->h_root + p.layers[L - 1].out);
    }
    return ICICLE_SUCCESS;
  }

  // The reference's walk (merkle_tree.h:148-203) over `count` proofs: hash the leaf, then one hash per layer over the path's group
  // with the previous digest in its place. One host image of every proof's layer inputs goes up in one copy, every layer is hashed in
  // one launch over all proofs (layer 0: one launch per distinct leaf size, the proofs ordered by it), a pruned proof's digests are
  // scattered into their holes in the next layer's inputs (a single one is written there by the hash itself), and all digests come
  // back in one copy behind one synchronisation. Full path: the digests are compared with the path on the host.
  static icicle_error_t tree_verify_batch(const Tree* t, const Proof* const* prs, uint64_t count, bool* valid)
  {
    const MerklePlan& p = t->plan;
    const int L = p.L();
    for (uint64_t i = 0; i < count; i++)
      valid[i] = false;
    // the checks, proof by proof, the first failure in index order; a root of another size is no root of this tree, and no error
    const bool pruned = prs[0]->pruned;
    std::vector<uint64_t> live;
    for (uint64_t i = 0; i < count; i++) {
      const Proof* pr = prs[i];
      if (pr->pruned != pruned) return ICICLE_INVALID_ARGUMENT;
      if (pr->leaf.empty()) return ICICLE_INVALID_ARGUMENT;
      if (pr->path.size() != (pruned ? p.pruned_path : p.full_path)) return ICICLE_INVALID_ARGUMENT;
      if (pr->root.size() != p.layers[L - 1].out) continue;
      if (pr->leaf_idx > (~0ull) / p.leaf_element_size) return ICICLE_INVALID_ARGUMENT;
      live.push_back(i);
    }
    if (live.empty()) return ICICLE_SUCCESS;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = nullptr;
    std::stable_sort(live.begin(), live.end(), [&](uint64_t a, uint64_t b) { return prs[a]->leaf.size() < prs[b]->leaf.size(); });
    const uint64_t n = live.size();
    // image: [n inputs of layer 0 | n inputs of layer 1 | .. | the holes of layers 1 .. L-1, n each] go up; the digests of layer i,
    // n * o_i bytes, lie behind them and come back
    std::vector<uint64_t> in_at(L), in_stride(L), dig_at(L);
    uint64_t at = 0;
    for (int i = 0; i < L; i++) {
      in_stride[i] = merkle_batch_pad16(i == 0 ? prs[live[n - 1]]->leaf.size() : p.layers[i].chunk);
      in_at[i] = at;
      at += n * in_stride[i];
    }
    const uint64_t holes_at = at, up_bytes = merkle_batch_pad16(holes_at + 4 * n * (L - 1));
    at = up_bytes;
    for (int i = 0; i < L; i++) {
      dig_at[i] = at;
      at += merkle_batch_pad16(n * p.layers[i].out);
    }
    const uint64_t total = at;
    PinnedBuf pinned;
    HIP_TRY(pinned.alloc(total), ICICLE_ALLOCATION_FAILED);
    uint8_t* img = pinned.ptr();
    uint32_t* holes = reinterpret_cast<uint32_t*>(img + holes_at);
    std::vector<uint64_t> offs;
    for (uint64_t k = 0; k < n; k++) {
      const Proof* pr = prs[live[k]];
      merkle_verify_offsets(p, pr->leaf_idx, pr->leaf.size(), &offs);
      std::memcpy(img + in_at[0] + k * in_stride[0], pr->leaf.data(), pr->leaf.size());
      const uint8_t* path = pr->path.data();
      for (int i = 1; i < L; i++) {
        const uint64_t c = p.layers[i].chunk, o = p.layers[i - 1].out, off = offs[i - 1];
        uint8_t* in = img + in_at[i] + k * in_stride[i];
        holes[(uint64_t)(i - 1) * n + k] = (uint32_t)off;
        if (pruned) {
          std::memcpy(in, path, off);
          std::memcpy(in + off + o, path + off, c - o - off);
          path += c - o;
        } else {
          std::memcpy(in, path, c);
          path += c;
        }
      }
    }
    TempBuf d_buf;
    HIP_TRY(d_buf.alloc(total, st), ICICLE_ALLOCATION_FAILED);
    uint8_t* d = d_buf.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(d, img, up_bytes, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
    for (int i = 0; i < L; i++) {
      // one pruned proof: its digest goes straight into its hole in the next layer's input, and the scatter launch is saved (the
      // L - 1 launches cost a single verify a quarter of its time: profiles/merkle_batch_notes.md)
      const bool direct = pruned && n == 1 && i + 1 < L;
      uint8_t* dig = direct ? d + in_at[i + 1] + holes[i] : d + dig_at[i];
      if (i == 0) {
        for (uint64_t k0 = 0; k0 < n;) { // runs of one leaf size
          const uint64_t len = prs[live[k0]]->leaf.size();
          uint64_t k1 = k0 + 1;
          while (k1 < n && prs[live[k1]]->leaf.size() == len)
            k1++;
          ICICLE_TRY(launch_batch(t->hashers[0], d + in_at[0] + k0 * in_stride[0], len, in_stride[0], k1 - k0, dig + k0 * p.layers[0].out, st));
          k0 = k1;
        }
      } else {
        ICICLE_TRY(launch_batch(t->hashers[i], d + in_at[i], p.layers[i].chunk, in_stride[i], n, dig, st));
      }
      if (pruned && i + 1 < L && !direct) {
        const uint32_t o = (uint32_t)p.layers[i].out;
        k_merkle_scatter<<<grid_for(n * ((o + 15) / 16)), 256, 0, st>>>(d + dig_at[i], o, d + in_at[i + 1], in_stride[i + 1],
                                                                       reinterpret_cast<const uint32_t*>(d + holes_at) + (uint64_t)i * n, n);
        LAUNCH_CHECK("k_merkle_scatter", st);
      }
    }
    HIP_TRY(hipMemcpyAsync(img + up_bytes, d + up_bytes, total - up_bytes, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
    HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    for (uint64_t k = 0; k < n; k++) {
      const Proof* pr = prs[live[k]];
      bool ok = true;
      if (!pruned)
        for (int i = 1; i < L && ok; i++) {
          const uint64_t o = p.layers[i - 1].out;
          ok = std::memcmp(img + dig_at[i - 1] + k * o, img + in_at[i] + k * in_stride[i] + holes[(uint64_t)(i - 1) * n + k], o) == 0;
        }
      valid[live[k]] = ok && std::memcmp(img + dig_at[L - 1] + k * p.layers[L - 1].out, pr->root.data(), pr->root.size()) == 0;
    }
    return ICICLE_SUCCESS;
  }

} // namespace icicle_hip

using namespace icicle_hip;

static_assert(sizeof(icicle_merkle_tree_config_t) == 24 && offsetof(icicle_merkle_tree_config_t, is_leaves_on_device) == 8 &&
                offsetof(icicle_merkle_tree_config_t, is_tree_on_device) == 9 && offsetof(icicle_merkle_tree_config_t, is_async) == 10 &&
                offsetof(icicle_merkle_tree_config_t, padding_policy) == 12 && offsetof(icicle_merkle_tree_config_t, ext) == 16,
              "MerkleTreeConfig layout (include/icicle/merkle/merkle_tree_config.h)");

extern "C" {

icicle_merkle_tree_handle_t icicle_merkle_tree_create(const icicle_hasher_handle_t* layer_hashes, size_t layer_hashes_len, uint64_t leaf_element_size,
                                                      uint64_t output_store_min_layer)
{
  try {
    if (!layer_hashes || layer_hashes_len == 0 || layer_hashes_len > (size_t)MERKLE_MAX_LAYERS) return nullptr;
    std::vector<uint64_t> chunk(layer_hashes_len), out(layer_hashes_len);
    Tree* t = new Tree;
    for (size_t i = 0; i < layer_hashes_len; i++) {
      const Hasher* h = (const Hasher*)layer_hashes[i];
      if (!h) {
        delete t;
        return nullptr;
      }
      t->hashers.push_back(*h); // the tree keeps its own copy: the caller may delete the handles
      chunk[i] = h->chunk, out[i] = h->out_bytes();
    }
    if (!merkle_make_plan(chunk.data(), out.data(), (int)layer_hashes_len, leaf_element_size, &t->plan)) {
      delete t;
      return nullptr;
    }
    t->store_min = (int)std::min<uint64_t>(output_store_min_layer, layer_hashes_len - 1);
    return (icicle_merkle_tree_handle_t)t;
  } catch (...) {
    return nullptr;
  }
}

icicle_error_t icicle_merkle_tree_delete(icicle_merkle_tree_handle_t tree)
{
  if (!tree) return ICICLE_INVALID_POINTER;
  Tree* t = (Tree*)tree;
  t->release();
  delete t;
  return ICICLE_SUCCESS;
}

icicle_error_t icicle_merkle_tree_build(icicle_merkle_tree_handle_t tree, const uint8_t* leaves, uint64_t size, const icicle_merkle_tree_config_t* config)
{
  if (!tree || !leaves || !config) return ICICLE_INVALID_POINTER;
  HASH_GUARDED(tree_build((Tree*)tree, leaves, size, config), ICICLE_ALLOCATION_FAILED)
}

const uint8_t* icicle_merkle_tree_get_root(icicle_merkle_tree_handle_t tree, size_t* out_size)
{
  const Tree* t = (const Tree*)tree;
  if (!t || !out_size || !t->built) return nullptr;
  *out_size = (size_t)t->plan.layers.back().out;
  return t->h_root;
}

icicle_error_t icicle_merkle_tree_get_proof(icicle_merkle_tree_handle_t tree, const uint8_t* leaves, uint64_t leaves_size, uint64_t leaf_idx, bool is_pruned,
                                            const icicle_merkle_tree_config_t* config, icicle_merkle_proof_handle_t merkle_proof)
{
  if (!tree || !leaves || !config || !merkle_proof) return ICICLE_INVALID_POINTER;
  Proof* const proof = (Proof*)merkle_proof;
  HASH_GUARDED(tree_proofs((const Tree*)tree, leaves, leaves_size, &leaf_idx, 1, is_pruned, config, &proof), ICICLE_ALLOCATION_FAILED)
}

icicle_error_t icicle_merkle_tree_verify(icicle_merkle_tree_handle_t tree, icicle_merkle_proof_handle_t merkle_proof, bool* valid)
{
  if (!tree || !merkle_proof || !valid) return ICICLE_INVALID_POINTER;
  const Proof* const proof = (const Proof*)merkle_proof;
  HASH_GUARDED(tree_verify_batch((const Tree*)tree, &proof, 1, valid), ICICLE_ALLOCATION_FAILED)
}

icicle_error_t icicle_hip_merkle_tree_get_proofs(icicle_merkle_tree_handle_t tree, const uint8_t* leaves, uint64_t leaves_size, const uint64_t* leaf_indices, uint64_t count,
                                                 bool is_pruned, const icicle_merkle_tree_config_t* config, icicle_merkle_proof_handle_t* proofs)
{
  if (!tree || !config) return ICICLE_INVALID_POINTER;
  if (count == 0) return ICICLE_SUCCESS;
  if (!leaves || !leaf_indices || !proofs) return ICICLE_INVALID_POINTER;
  for (uint64_t i = 0; i < count; i++)
    if (!proofs[i]) return ICICLE_INVALID_POINTER;
  HASH_GUARDED(tree_proofs((const Tree*)tree, leaves, leaves_size, leaf_indices, count, is_pruned, config, (Proof* const*)proofs), ICICLE_ALLOCATION_FAILED)
}

icicle_error_t icicle_hip_merkle_tree_verify_batch(icicle_merkle_tree_handle_t tree, const icicle_merkle_proof_handle_t* proofs, uint64_t count, bool* valid)
{
  if (!tree) return ICICLE_INVALID_POINTER;
  if (count == 0) return ICICLE_SUCCESS;
  if (!proofs || !valid) return ICICLE_INVALID_POINTER;
  for (uint64_t i = 0; i < count; i++)
    if (!proofs[i]) return ICICLE_INVALID_POINTER;
  HASH_GUARDED(tree_verify_batch((const Tree*)tree, (const Proof* const*)proofs, count, valid), ICICLE_ALLOCATION_FAILED)
}

icicle_merkle_proof_handle_t icicle_merkle_proof_create(void) { return (icicle_merkle_proof_handle_t) new (std::nothrow) Proof; }

icicle_merkle_proof_handle_t icicle_merkle_proof_create_with_data(bool pruned_path, int64_t leaf_idx, const uint8_t* leaf, size_t leaf_size, const uint8_t* root,
                                                                  size_t root_size, const uint8_t* path, size_t path_size)
{
  try {
    if ((!leaf && leaf_size) || (!root && root_size) || (!path && path_size)) return nullptr;
    Proof* p = new Proof;
    p->pruned = pruned_path;
    p->leaf_idx = (uint64_t)leaf_idx;
    p->leaf.assign(leaf, leaf + leaf_size);
    p->root.assign(root, root + root_size);
    p->path.assign(path, path + path_size);
    return (icicle_merkle_proof_handle_t)p;
  } catch (...) {
    return nullptr;
  }
}

icicle_error_t icicle_merkle_proof_delete(icicle_merkle_proof_handle_t proof)
{
  if (!proof) return ICICLE_INVALID_POINTER;
  delete (Proof*)proof;
  return ICICLE_SUCCESS;
}

bool icicle_merkle_proof_is_pruned(icicle_merkle_proof_handle_t proof) { return proof ? ((const Proof*)proof)->pruned : false; }

const uint8_t* icicle_merkle_proof_get_path(icicle_merkle_proof_handle_t proof, size_t* out_size)
{
  if (!proof || !out_size) return nullptr;
  const Proof* p = (const Proof*)proof;
  *out_size = p->path.size();
  return p->path.data();
}

const uint8_t* icicle_merkle_proof_get_leaf(icicle_merkle_proof_handle_t proof, size_t* out_size, uint64_t* out_leaf_idx)
{
  if (!proof || !out_size || !out_leaf_idx) return nullptr;
  const Proof* p = (const Proof*)proof;
  *out_size = p->leaf.size();
  *out_leaf_idx = p->leaf_idx;
  return p->leaf.data();
}

const uint8_t* icicle_merkle_proof_get_root(icicle_merkle_proof_handle_t proof, size_t* out_size)
{
  if (!proof || !out_size) return nullptr;
  const Proof* p = (const Proof*)proof;
  *out_size = p->root.size();
  return p->root.data();
}

} // extern "C"
