// What merkle.hip reads from hash.hip: the hasher a tree layer copies, the two host functions that hash a batch of messages and
// the padded layer-0 chunks of a tree with it, and the descriptors and the launcher of the fused top kernel. Every kernel stays in
// hash.hip (and poseidon2.hip, poseidon.hip behind the hasher's kind); no device code crosses a translation unit.
#pragma once
#include "common.h"
#include "merkle_plan.h"
#include "blake.hpp"
#include <algorithm>

namespace icicle_hip {

  // Poseidon2: kernels and state in poseidon2.hip (31-bit fields), poseidon2_gold.hip (Goldilocks) and poseidon2_wide.hip (256-bit
  // fields), Poseidon: poseidon.hip
  enum : int { HASH_KECCAK = 0, HASH_BLAKE2S = 1, HASH_BLAKE3 = 2, HASH_POSEIDON2 = 3, HASH_POSEIDON = 4, HASH_POSEIDON2_WIDE = 5, HASH_POSEIDON2_GOLD = 6 };
  inline bool hash_kind_is_field(int kind) { return kind == HASH_POSEIDON2 || kind == HASH_POSEIDON || kind == HASH_POSEIDON2_WIDE || kind == HASH_POSEIDON2_GOLD; }

  struct Hasher {
    int kind;       // HASH_KECCAK, HASH_BLAKE2S, HASH_BLAKE3, HASH_POSEIDON2, HASH_POSEIDON, HASH_POSEIDON2_WIDE, HASH_POSEIDON2_GOLD
    int rate_words; // Keccak only -- 17: 256-bit digest, 9: 512-bit digest
    int out_words;
    uint32_t suffix; // Keccak only -- 0x01 Keccak, 0x06 SHA3
    uint64_t chunk;  // default input size, 0 = none
    std::shared_ptr<Poseidon2Hasher> p2; // Poseidon2 only -- field, width, tag and constants, shared with the trees that copy this hasher
    std::shared_ptr<PoseidonHasher> p1;  // Poseidon only -- the same; `chunk` is the only message length it hashes
    std::shared_ptr<Poseidon2WideHasher> p2w; // Poseidon2 over a 256-bit field only -- as p2, with elements and a digest of 32 bytes
    std::shared_ptr<Poseidon2GoldHasher> p2g; // Poseidon2 over Goldilocks only -- as p2, with elements and a digest of 8 bytes
    uint64_t out_bytes() const { return kind == HASH_POSEIDON2 ? 4 : kind == HASH_POSEIDON2_GOLD ? 8 : kind == HASH_KECCAK ? 8ull * out_words : 32; }
    // Blake3 over more than one chunk: several launches and a buffer of chaining values; not for the fused top kernel
    bool multi_chunk(uint64_t len) const { return kind == HASH_BLAKE3 && len > BLAKE3_CHUNK; }
  };

  inline unsigned grid_for(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 22); }

  // n messages of `len` bytes at in + t * stride -> digests of h.out_bytes() bytes back to back at out; any alignment
  icicle_error_t launch_batch(const Hasher& h, const uint8_t* in, uint64_t len, uint64_t stride, uint64_t n, uint8_t* out, hipStream_t st);
  // layer-0 chunks [first, first + n) of a tree whose leaves end inside or in front of them (ReadPadded of hash_readers.hpp)
  icicle_error_t launch_leaves(const Hasher& h, const uint8_t* leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid, const uint8_t* last,
                               uint64_t es, uint8_t* out, hipStream_t st);

  // the layers k_merkle_top (hash.hip) walks in one launch
  struct MerkleTopLayer {
    const uint8_t* in; // count chunks of `chunk` bytes
    uint8_t* out;
    uint32_t chunk, count, rate_words, suffix;
    int kind; // HASH_KECCAK (rate_words, suffix), HASH_BLAKE2S, HASH_BLAKE3 (chunk <= 1024: one Blake3 chunk)
  };
  struct MerkleTopArgs {
    MerkleTopLayer l[MERKLE_MAX_LAYERS];
    int n;
  };
  constexpr int MERKLE_TOP_THREADS = 1024;
  // default switch point (MerkleTreeConfig.ext "hip_merkle_top_max_hashes" overrides it, 0 = never fuse): the largest layer the one
  // block hashes in a single pass, one message per thread (profiles/hash_merkle_notes.md)
  constexpr int MERKLE_TOP_MAX_HASHES = 1024;
  icicle_error_t launch_merkle_top(const MerkleTopArgs& args, hipStream_t st);

// an entry point's body: no exception crosses the C ABI
#define HASH_GUARDED(expr, on_throw)                                                                                   \
  try {                                                                                                                \
    return (expr);                                                                                                     \
  } catch (...) {                                                                                                      \
    return on_throw;                                                                                                   \
  }

} // namespace icicle_hip
