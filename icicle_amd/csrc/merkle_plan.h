// Host-only arithmetic of the Merkle tree (merkle.hip): layer counts, padding extents and the offsets verify() walks. No HIP in
// here, so tests/merkle_plan_harness.cpp compiles it with g++ and compares it with the Python model (tests/merkle_model.py).
// The leaf-index arithmetic of an opening -- the byte offsets of a proof's path, the sub-tree a proof recomputes --, as one
// host-and-device function, is merkle_batch.h.
//
// Notation (reference: icicle/backend/cpu/src/hash/cpu_merkle_tree.cpp:18-51): layer i hashes n_i chunks of c_i bytes into
// digests of o_i bytes; c_{i+1} % o_i == 0 ("each layer output size must divide the next layer input size"), the arity of
// layer i + 1 is a_{i+1} = c_{i+1} / o_i, n_{L-1} = 1, n_{i-1} = n_i * a_i, and the tree takes n_0 * c_0 bytes of leaves.
#pragma once
#include <cstdint>
#include <vector>

namespace icicle_hip {

  constexpr int MERKLE_MAX_LAYERS = 64; // the fused top kernel takes its layer descriptors by value
  enum { MERKLE_PAD_NONE = 0, MERKLE_PAD_ZERO = 1, MERKLE_PAD_LAST = 2 };

  struct MerkleLayerPlan {
    uint64_t chunk = 0;  // c_i
    uint64_t out = 0;    // o_i
    uint64_t count = 0;  // n_i
    uint64_t offset = 0; // byte offset of the layer's digests in a buffer that holds every layer back to back, 16-aligned
  };

  struct MerklePlan {
    std::vector<MerkleLayerPlan> layers;
    uint64_t leaf_element_size = 0;
    uint64_t capacity = 0;    // n_0 * c_0
    uint64_t full_path = 0;   // sum_{i>=1} c_i
    uint64_t pruned_path = 0; // sum_{i>=1} (c_i - o_{i-1})
    uint64_t total_bytes = 0; // of all layers' digests at the offsets above
    int L() const { return (int)layers.size(); }
    uint64_t arity(int i) const { return layers[i].chunk / layers[i - 1].out; } // i >= 1
  };

  // false: not a tree (no layer, a zero size, c_{i+1} % o_i != 0, too many layers, or sizes beyond 2^56 bytes)
  inline bool merkle_make_plan(const uint64_t* chunk, const uint64_t* out, int L, uint64_t leaf_element_size, MerklePlan* p)
  {
    if (L < 1 || L > MERKLE_MAX_LAYERS || leaf_element_size == 0) return false;
    p->layers.assign(L, MerkleLayerPlan{});
    p->leaf_element_size = leaf_element_size;
    p->full_path = p->pruned_path = 0;
    constexpr uint64_t LIMIT = 1ull << 56;
    uint64_t n = 1;
    for (int i = L - 1; i >= 0; i--) {
      if (chunk[i] == 0 || out[i] == 0 || chunk[i] >= (1ull << 32) || out[i] > 64) return false;
      p->layers[i].chunk = chunk[i], p->layers[i].out = out[i], p->layers[i].count = n;
      if (n * chunk[i] >= LIMIT) return false;
      if (i > 0) {
        if (out[i - 1] == 0 || chunk[i] % out[i - 1] != 0) return false;
        n *= chunk[i] / out[i - 1];
        if (n >= LIMIT) return false;
        p->full_path += chunk[i];
        p->pruned_path += chunk[i] - out[i - 1];
      }
    }
    p->capacity = p->layers[0].count * p->layers[0].chunk;
    uint64_t off = 0;
    for (int i = 0; i < L; i++) {
      p->layers[i].offset = off;
      off += (p->layers[i].count * p->layers[i].out + 15) & ~15ull;
    }
    p->total_bytes = off;
    return true;
  }

  // What layer 0 reads for `leaves_size` bytes of leaves: chunks [0, full_chunks) come from the leaves alone, the rest of the n_0
  // chunks hold at least one padding byte. ZeroPadding appends zeros, LastValue repeats the bytes [last_off, leaves_size).
  struct MerklePadding {
    uint64_t full_chunks = 0;
    uint64_t pad_bytes = 0;
    uint64_t last_off = 0; // LastValue only
  };
  // 0 = fine, 1 = invalid argument (the rules of the header: empty leaves, leaves beyond the capacity, short leaves without a
  // padding policy, LastValue with leaves_size or c_0 no multiple of the element size, an unknown policy)
  inline int merkle_padding(const MerklePlan& p, uint64_t leaves_size, int policy, MerklePadding* out)
  {
    if (leaves_size == 0 || leaves_size > p.capacity) return 1;
    if (policy < MERKLE_PAD_NONE || policy > MERKLE_PAD_LAST) return 1;
    if (leaves_size < p.capacity) {
      if (policy == MERKLE_PAD_NONE) return 1;
      if (policy == MERKLE_PAD_LAST) {
        const uint64_t es = p.leaf_element_size;
        if (leaves_size % es != 0 || p.layers[0].chunk % es != 0 || leaves_size < es) return 1;
        out->last_off = leaves_size - es;
      }
    }
    out->full_chunks = leaves_size / p.layers[0].chunk;
    out->pad_bytes = p.capacity - leaves_size;
    return 0;
  }

  // The offsets verify() walks (include/icicle/merkle/merkle_tree.h:148-203): where the digest of layer i - 1 sits inside the
  // input of layer i, for i = 1 .. L-1, from the element's byte offset alone.
  inline void merkle_verify_offsets(const MerklePlan& p, uint64_t leaf_idx, uint64_t leaf_size, std::vector<uint64_t>* offs)
  {
    offs->clear();
    uint64_t start = leaf_idx * p.leaf_element_size, in_size = leaf_size, out_size = p.layers[0].out;
    for (int i = 1; i < p.L(); i++) {
      start = (start / in_size) * out_size;
      in_size = p.layers[i].chunk, out_size = p.layers[i].out;
      offs->push_back(start % in_size);
    }
  }

} // namespace icicle_hip
