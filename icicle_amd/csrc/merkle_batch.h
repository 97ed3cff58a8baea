// Index arithmetic of Merkle openings (icicle_merkle_tree_get_proof, icicle_hip_merkle_tree_get_proofs, merkle.hip), the only one in
// the product: leaf index -> per layer the on-path node, the group's offset in the layer, the on-path digest's offset in the group,
// the group's place in the path (pruned or not) and its offset inside a re-hashed sub-tree; and the layout of the staging record one
// proof's pieces are gathered into. Written once for the host and the device: the gather kernel, the host's unpacking and the CPU
// harnesses call this code. tests/merkle_batch_harness.cpp holds it against the plain loop form of the walk, which it carries as
// test-only reference code, for every index; tests/merkle_plan_harness.cpp hands it to the Python model (tests/merkle_model.py).
// No HIP in here beyond the function qualifier.
#pragma once
#include "merkle_plan.h"

// qualifier of code that runs in a kernel and, for the host and the CPU tests, on the host
#if defined(__HIPCC__)
#define MERKLE_HD __host__ __device__ __forceinline__
#else
#define MERKLE_HD inline
#endif

namespace icicle_hip {

  // A tree's shape as the kernel takes it (by value), and the staging record of one proof:
  //   [ group of layer 0 | .. | group of layer L-2 | leaf chunk | last element ], every piece at a 16-aligned offset, so that
  // groups of 32- and 64-byte digests move 16 bytes per lane. A group is staged whole; pruning happens when the host unpacks.
  struct MerkleBatchShape {
    int steps = 0;     // L - 1: the layers a path has a group of
    int store_min = 0; // layers below it are not kept (clamped to [0, L-1])
    uint32_t pruned = 0;
    uint64_t es = 0, c0 = 0, capacity = 0; // leaf element size, c_0, n_0 * c_0
    uint32_t out[MERKLE_MAX_LAYERS];       // o_i
    uint32_t len[MERKLE_MAX_LAYERS];       // c_{i+1}: the group of layer i
    uint64_t stage_at[MERKLE_MAX_LAYERS];  // the group of layer i in the staging record
    uint64_t leaf_at = 0, last_at = 0, stride = 0;
  };

  inline uint64_t merkle_batch_pad16(uint64_t v) { return (v + 15) & ~15ull; }

  inline void merkle_batch_shape(const MerklePlan& p, bool pruned, int store_min, MerkleBatchShape* s)
  {
    const int L = p.L();
    s->steps = L - 1;
    s->store_min = store_min < 0 ? 0 : store_min > L - 1 ? L - 1 : store_min;
    s->pruned = pruned ? 1 : 0;
    s->es = p.leaf_element_size, s->c0 = p.layers[0].chunk, s->capacity = p.capacity;
    uint64_t at = 0;
    for (int i = 0; i < MERKLE_MAX_LAYERS; i++) {
      const bool on = i + 1 < L;
      s->out[i] = on ? (uint32_t)p.layers[i].out : 0;
      s->len[i] = on ? (uint32_t)p.layers[i + 1].chunk : 0;
      s->stage_at[i] = at;
      at += merkle_batch_pad16(s->len[i]);
    }
    s->leaf_at = at;
    s->last_at = at + merkle_batch_pad16(s->c0);
    s->stride = s->last_at + merkle_batch_pad16(s->es);
  }

  // the layer-0 chunk that holds element leaf_idx (the proof's leaf is this whole chunk); false: leaf_idx * leaf_element_size lies
  // at or beyond the capacity
  MERKLE_HD bool merkle_batch_chunk0(const MerkleBatchShape& s, uint64_t leaf_idx, uint64_t* chunk0)
  {
    if (leaf_idx >= s.capacity / s.es + 1) return false;
    const uint64_t byte0 = leaf_idx * s.es;
    if (byte0 >= s.capacity) return false;
    *chunk0 = byte0 / s.c0;
    return true;
  }

  // One layer's share of a proof's path (cpu_merkle_tree.cpp:546-573): the a_{i+1} digests of layer i that form the one input of
  // layer i + 1 on the way from the leaf to the root. Pruned, the digest ON the way is left out (verify recomputes it).
  struct MerkleBatchStep {
    uint64_t node = 0;     // index of the on-path digest in layer i
    uint64_t src_off = 0;  // byte offset of the group in layer i's digests
    uint64_t len = 0;      // c_{i+1}
    uint64_t skip_off = 0; // byte offset of the on-path digest inside the group
    uint64_t dst_off = 0;  // where the group starts in the path
    // a layer below store_min: the group's offset among the nodes of this layer under the on-path node of layer store_min, which
    // is where it lies in the re-hashed sub-tree; src_off for the stored layers
    uint64_t sub_off = 0;
  };
  // layer in [0, steps)
  MERKLE_HD void merkle_batch_step(const MerkleBatchShape& s, uint64_t chunk0, int layer, MerkleBatchStep* st)
  {
    uint64_t node = chunk0, dst = 0;
    for (int i = 0; i < layer; i++) {
      dst += s.pruned ? s.len[i] - s.out[i] : s.len[i];
      node /= s.len[i] / s.out[i]; // a_{i+1}
    }
    const uint64_t o = s.out[layer], a = s.len[layer] / o;
    st->node = node;
    st->src_off = (node / a) * a * o;
    st->len = s.len[layer];
    st->skip_off = (node % a) * o;
    st->dst_off = dst;
    uint64_t per_sub = 1; // nodes of this layer under one node of layer store_min: a multiple of a, so a group never straddles two
    for (int j = layer; j < s.store_min; j++)
      per_sub *= s.len[j] / s.out[j];
    st->sub_off = layer < s.store_min ? st->src_off - (node / per_sub) * per_sub * o : st->src_off;
  }

  MERKLE_HD uint64_t merkle_batch_path_size(const MerkleBatchShape& s)
  {
    uint64_t size = 0;
    for (int i = 0; i < s.steps; i++)
      size += s.pruned ? s.len[i] - s.out[i] : s.len[i];
    return size;
  }

  // the sub-tree under the on-path node of layer store_min: layer-0 chunks [first, first + count)
  MERKLE_HD void merkle_batch_subtree(const MerkleBatchShape& s, uint64_t chunk0, uint64_t* first, uint64_t* count)
  {
    uint64_t c = 1;
    for (int j = 0; j < s.store_min; j++)
      c *= s.len[j] / s.out[j];
    *count = c;
    *first = (chunk0 / c) * c;
  }

  // Which piece of the staging record byte `off` lies in: 0 .. steps-1 the group of that layer, steps the leaf chunk, steps + 1
  // the last element; -1: padding between two pieces. *q = the offset inside the piece, *len = the piece's bytes.
  MERKLE_HD int merkle_batch_piece(const MerkleBatchShape& s, uint64_t off, uint64_t* q, uint64_t* len)
  {
    int piece;
    uint64_t at, n;
    if (off >= s.last_at) {
      piece = s.steps + 1, at = s.last_at, n = s.es;
    } else if (off >= s.leaf_at) {
      piece = s.steps, at = s.leaf_at, n = s.c0;
    } else {
      piece = 0;
      while (piece + 1 < s.steps && off >= s.stage_at[piece + 1])
        piece++;
      at = s.stage_at[piece], n = s.len[piece]; // steps == 0: leaf_at == 0, so this branch is not taken
    }
    *q = off - at, *len = n;
    return off - at < n ? piece : -1;
  }

} // namespace icicle_hip
