// Keccak / SHA3 / Blake2s / Blake3 batch hashing, Merkle trees and the proof-of-work search on the device. The Blake compression and
// absorb code is blake.hpp, the four message readers hash_readers.hpp (both also compile for the host); the kernels over them are below.
// Poseidon2 over BabyBear and KoalaBear hashes through the same hasher and tree paths; its kernels and its state are poseidon2.hip.
// Poseidon over the 256-bit scalar fields does the same through poseidon.hip.
// Batched openings and verification (icicle_hip_merkle_tree_get_proofs, icicle_hip_merkle_tree_verify_batch: one gather launch for all
// openings, one hash launch per layer for all verifications) are this backend's own; their index arithmetic is merkle_batch.h.
//
// C ABI of the reference: icicle/src/hash/hash_c_api.cpp (icicle_create_keccak_256 .. icicle_create_blake3, icicle_hasher_hash), src/hash/merkle_c_api.cpp
// (icicle_merkle_tree_*, icicle_merkle_proof_*), include/icicle/hash/pow.h (proof_of_work, proof_of_work_verify); configs
// include/icicle/hash/hash_config.h, include/icicle/merkle/merkle_tree_config.h, pow.h;
// tree / proof semantics backend/cpu/src/hash/cpu_merkle_tree.cpp:143-211,546-573 and include/icicle/merkle/merkle_tree.h:148-203.
//
// The permutation is written from FIPS 202:
//   * rotation offsets: (t + 1)(t + 2) / 2 mod 64 for t = 0 .. 23 along the walk (x, y) -> (y, 2x + 3y) from (1, 0); lane (0, 0) stays.
//       rot, (x, y) = [0] * 25, (1, 0)
//       for t in range(24): rot[x + 5 * y] = (t + 1) * (t + 2) // 2 % 64; x, y = y, (2 * x + 3 * y) % 5
//   * rho + pi: B[y][2x + 3y] = rotl(A[x][y], rot[x][y]), lane index x + 5 y (the 25 lines of KECCAK_RHO_PI are this, printed by
//       for x in range(5): for y in range(5): print(f"b[{y + 5 * ((2 * x + 3 * y) % 5)}] = rotl64<{rot[x + 5 * y]}>(a[{x + 5 * y}]);"))
//   * round constants: bit 2^j - 1 of RC[i] is rc(j + 7 i), rc(t) = bit 0 of x^t mod x^8 + x^6 + x^5 + x^4 + 1 over GF(2):
//       r = 1
//       for i in range(24):
//           c = 0
//           for j in range(7):
//               if r & 1: c |= 1 << ((1 << j) - 1)
//               r = ((r << 1) ^ (0x71 if r & 0x80 else 0)) & 0xFF
//           RC.append(c)
// (tests/merkle_model.py holds the same three derivations and is checked against hashlib's SHA3.)
//
// One lane hashes one message: the 25-lane state is 50 VGPRs, every index a compile-time constant, the 24 rounds a rolled loop.
// Keccak is 64-bit integer ALU work, far from the memory roof, so the lanes' strided loads do not matter.
#include "common.h"
#include "merkle_plan.h"
#include "merkle_batch.h"
#include "hash_readers.hpp"
#include "blake.hpp"
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>

namespace icicle_hip {

  __constant__ uint64_t KECCAK_RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

  // rotate left by a constant: the compiler's 64-bit shift pair. Two v_alignbit_b32 on the halves were tried and retired
  // (profiles/hash_merkle_notes.md has the instruction counts of both, profiles/retired_variants.md the commit that still builds them).
  template <int N>
  __device__ __forceinline__ uint64_t rotl64(uint64_t v)
  {
    if constexpr (N == 0) {
      return v;
    } else {
      return (v << N) | (v >> (64 - N));
    }
  }

#define KECCAK_RHO_PI                                                                                                  \
  b[0] = rotl64<0>(a[0]), b[16] = rotl64<36>(a[5]), b[7] = rotl64<3>(a[10]), b[23] = rotl64<41>(a[15]), b[14] = rotl64<18>(a[20]);    \
  b[10] = rotl64<1>(a[1]), b[1] = rotl64<44>(a[6]), b[17] = rotl64<10>(a[11]), b[8] = rotl64<45>(a[16]), b[24] = rotl64<2>(a[21]);    \
  b[20] = rotl64<62>(a[2]), b[11] = rotl64<6>(a[7]), b[2] = rotl64<43>(a[12]), b[18] = rotl64<15>(a[17]), b[9] = rotl64<61>(a[22]);   \
  b[5] = rotl64<28>(a[3]), b[21] = rotl64<55>(a[8]), b[12] = rotl64<25>(a[13]), b[3] = rotl64<21>(a[18]), b[19] = rotl64<56>(a[23]);  \
  b[15] = rotl64<27>(a[4]), b[6] = rotl64<20>(a[9]), b[22] = rotl64<39>(a[14]), b[13] = rotl64<8>(a[19]), b[4] = rotl64<14>(a[24]);
#define KECCAK_CHI_ROW(r)                                                                                              \
  a[r + 0] = b[r + 0] ^ (~b[r + 1] & b[r + 2]), a[r + 1] = b[r + 1] ^ (~b[r + 2] & b[r + 3]), a[r + 2] = b[r + 2] ^ (~b[r + 3] & b[r + 4]), \
        a[r + 3] = b[r + 3] ^ (~b[r + 4] & b[r + 0]), a[r + 4] = b[r + 4] ^ (~b[r + 0] & b[r + 1]);

  __device__ __forceinline__ void keccak_f1600(uint64_t (&a)[25])
  {
#pragma unroll 1
    for (int rnd = 0; rnd < 24; rnd++) {
      const uint64_t c0 = a[0] ^ a[5] ^ a[10] ^ a[15] ^ a[20], c1 = a[1] ^ a[6] ^ a[11] ^ a[16] ^ a[21], c2 = a[2] ^ a[7] ^ a[12] ^ a[17] ^ a[22],
                     c3 = a[3] ^ a[8] ^ a[13] ^ a[18] ^ a[23], c4 = a[4] ^ a[9] ^ a[14] ^ a[19] ^ a[24];
      const uint64_t d0 = c4 ^ rotl64<1>(c1), d1 = c0 ^ rotl64<1>(c2), d2 = c1 ^ rotl64<1>(c3), d3 = c2 ^ rotl64<1>(c4), d4 = c3 ^ rotl64<1>(c0);
#pragma unroll
      for (int y = 0; y < 25; y += 5)
        a[y] ^= d0, a[y + 1] ^= d1, a[y + 2] ^= d2, a[y + 3] ^= d3, a[y + 4] ^= d4;
      uint64_t b[25];
      KECCAK_RHO_PI
      KECCAK_CHI_ROW(0) KECCAK_CHI_ROW(5) KECCAK_CHI_ROW(10) KECCAK_CHI_ROW(15) KECCAK_CHI_ROW(20)
      a[0] ^= KECCAK_RC[rnd];
    }
  }

  // where a lane's message bytes come from: ReadAligned, ReadBytes, ReadPadded, ReadPow (hash_readers.hpp)

  // sponge over one message of `len` bytes: absorb whole blocks, then the last block with the domain suffix at byte len % rate and
  // 0x80 at the block's last byte (pad10*1). The digest is a[0 .. OUT_WORDS).
  template <int RATE_WORDS, class RD>
  __device__ __forceinline__ void keccak_msg(const RD& rd, uint64_t len, uint32_t suffix, uint64_t (&a)[25])
  {
    constexpr uint64_t RATE = 8ull * RATE_WORDS;
#pragma unroll
    for (int i = 0; i < 25; i++)
      a[i] = 0;
    uint64_t off = 0;
    for (;;) { // one call site of the permutation: whole blocks, then the padded last one
      const bool last_block = len - off < RATE;
      if (!last_block) {
#pragma unroll
        for (int i = 0; i + 1 < RATE_WORDS; i += 2) {
          uint64_t lo, hi;
          rd.pair(off + 8 * i, lo, hi);
          a[i] ^= lo, a[i + 1] ^= hi;
        }
        if constexpr (RATE_WORDS & 1) a[RATE_WORDS - 1] ^= rd.word(off + 8 * (RATE_WORDS - 1));
      } else {
        // words [0, wi) are whole, word wi holds the last rem % 8 message bytes and the suffix, the block's last byte takes 0x80
        const uint32_t rem = (uint32_t)(len - off), wi = rem >> 3, nb = rem & 7;
        uint64_t part = (uint64_t)suffix << (8 * nb);
        for (uint32_t k = 0; k < nb; k++)
          part |= (uint64_t)rd.byte(off + 8 * wi + k) << (8 * k);
#pragma unroll
        for (int i = 0; i < RATE_WORDS; i++) {
          uint64_t w = 0;
          if ((uint32_t)i < wi) w = rd.word(off + 8 * i);
          if ((uint32_t)i == wi) w = part;
          if (i == RATE_WORDS - 1) w ^= 0x80ull << 56;
          a[i] ^= w;
        }
      }
      keccak_f1600(a);
      if (last_block) break;
      off += RATE;
    }
  }

  template <int OUT_WORDS>
  __device__ __forceinline__ void store_digest(uint8_t* out, bool aligned, const uint64_t (&a)[25])
  {
    if (aligned) {
#pragma unroll
      for (int i = 0; i < OUT_WORDS; i++)
        reinterpret_cast<uint64_t*>(out)[i] = a[i];
    } else {
#pragma unroll
      for (int i = 0; i < OUT_WORDS; i++)
#pragma unroll
        for (int k = 0; k < 8; k++)
          out[8 * i + k] = (uint8_t)(a[i] >> (8 * k));
    }
  }

  enum : uint32_t { HASH_IN_ALIGNED16 = 2, HASH_OUT_ALIGNED8 = 4 };

  // n messages of `len` bytes at in + t * stride -> digests of 8 * OUT_WORDS bytes at out + t * 8 * OUT_WORDS. One lane per message.
  // ALIGNED: `in` and `stride` are multiples of 8 (64-bit loads, 128-bit ones with HASH_IN_ALIGNED16); otherwise byte loads. Two
  // kernels rather than a branch, so that the byte path's loads in flight do not set the aligned path's register count.
  template <int RATE_WORDS, int OUT_WORDS, bool ALIGNED>
  __global__ __launch_bounds__(256) void k_keccak_batch(const uint8_t* __restrict__ in, uint64_t len, uint64_t stride, uint64_t n, uint32_t suffix, uint32_t flags,
                                                         uint8_t* __restrict__ out)
  {
    static_assert(2 * OUT_WORDS + RATE_WORDS == 25, "capacity = twice the digest");
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += step) {
      uint64_t a[25];
      const uint8_t* p = in + t * stride;
      if constexpr (ALIGNED)
        keccak_msg<RATE_WORDS>(ReadAligned{p, (flags & HASH_IN_ALIGNED16) != 0}, len, suffix, a);
      else
        keccak_msg<RATE_WORDS>(ReadBytes{p}, len, suffix, a);
      store_digest<OUT_WORDS>(out + t * (8 * OUT_WORDS), (flags & HASH_OUT_ALIGNED8) != 0, a);
    }
  }

  // layer-0 chunks [first, first + n) of a tree whose leaves end inside or in front of them (ReadPadded); digest t goes to
  // out + t * 8 * OUT_WORDS, 8-aligned
  template <int RATE_WORDS, int OUT_WORDS>
  __global__ __launch_bounds__(256) void k_keccak_leaves(const uint8_t* __restrict__ leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid,
                                                          const uint8_t* __restrict__ last, uint64_t es, uint32_t suffix, uint8_t* __restrict__ out)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += step) {
      uint64_t a[25];
      keccak_msg<RATE_WORDS>(ReadPadded{leaves, (first + t) * chunk, valid, last, es}, chunk, suffix, a);
      store_digest<OUT_WORDS>(out + t * (8 * OUT_WORDS), true, a);
    }
  }

  // ---- Blake2s / Blake3 ---------------------------------------------------------------------------------------------------------
  enum : int { HASH_KECCAK = 0, HASH_BLAKE2S = 1, HASH_BLAKE3 = 2, HASH_POSEIDON2 = 3, HASH_POSEIDON = 4 }; // Poseidon2: kernels and state in poseidon2.hip, Poseidon: poseidon.hip

  __device__ __forceinline__ void store_digest32(uint8_t* out, bool aligned, const uint32_t (&h)[8])
  {
    if (aligned) {
#pragma unroll
      for (int i = 0; i < 4; i++)
        reinterpret_cast<uint64_t*>(out)[i] = h[2 * i] | (uint64_t)h[2 * i + 1] << 32;
    } else {
#pragma unroll
      for (int i = 0; i < 8; i++)
#pragma unroll
        for (int k = 0; k < 4; k++)
          out[4 * i + k] = (uint8_t)(h[i] >> (8 * k));
    }
  }

  // Blake2s of any length, Blake3 of at most one chunk (1024 bytes)
  template <int KIND, class RD>
  __device__ __forceinline__ void blake_msg(const RD& rd, uint64_t len, uint32_t (&h)[8])
  {
    if constexpr (KIND == HASH_BLAKE2S)
      blake2s_msg(rd, len, h);
    else
      blake3_chunk(rd, len, 0, true, h);
  }

  // the Blake twin of k_keccak_batch: n messages of `len` bytes at in + t * stride -> 32-byte digests at out + 32 t
  template <int KIND, bool ALIGNED>
  __global__ __launch_bounds__(256) void k_blake_batch(const uint8_t* __restrict__ in, uint64_t len, uint64_t stride, uint64_t n, uint32_t flags, uint8_t* __restrict__ out)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += step) {
      uint32_t h[8];
      const uint8_t* p = in + t * stride;
      if constexpr (ALIGNED)
        blake_msg<KIND>(ReadAligned{p, (flags & HASH_IN_ALIGNED16) != 0}, len, h);
      else
        blake_msg<KIND>(ReadBytes{p}, len, h);
      store_digest32(out + t * 32, (flags & HASH_OUT_ALIGNED8) != 0, h);
    }
  }

  // the Blake twin of k_keccak_leaves
  template <int KIND>
  __global__ __launch_bounds__(256) void k_blake_leaves(const uint8_t* __restrict__ leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid,
                                                         const uint8_t* __restrict__ last, uint64_t es, uint8_t* __restrict__ out)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += step) {
      uint32_t h[8];
      blake_msg<KIND>(ReadPadded{leaves, (first + t) * chunk, valid, last, es}, chunk, h);
      store_digest32(out + t * 32, true, h);
    }
  }

  // Blake3 messages of more than one chunk. A per-lane stack of chaining values would be indexed at run time and live in scratch,
  // so the tree is walked level by level instead: one lane per chunk over all messages writes chaining values, then one launch
  // per level with one lane per parent (blake.hpp: pairing adjacent nodes, an odd last node carried up, is Blake3's tree).
  // Chaining value c of message t goes to cv + 32 (t * k + c); k = chunks per message.
  template <bool ALIGNED>
  __global__ __launch_bounds__(256) void k_blake3_chunks(const uint8_t* __restrict__ in, uint64_t len, uint64_t stride, uint64_t n, uint64_t k, uint32_t flags,
                                                          uint8_t* __restrict__ cv)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x, total = n * k;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
      const uint64_t msg = t / k, c = t % k, at = c * BLAKE3_CHUNK, clen = len - at < BLAKE3_CHUNK ? len - at : BLAKE3_CHUNK;
      const uint8_t* p = in + msg * stride + at; // stride % 8 == 0 and at % 1024 == 0 keep the alignment of `in`
      uint32_t h[8];
      if constexpr (ALIGNED)
        blake3_chunk(ReadAligned{p, (flags & HASH_IN_ALIGNED16) != 0}, clen, c, false, h);
      else
        blake3_chunk(ReadBytes{p}, clen, c, false, h);
      store_digest32(cv + t * 32, true, h);
    }
  }

  // the same over layer-0 chunks [first, first + n) of a tree that reach into the padding
  __global__ __launch_bounds__(256) void k_blake3_leaf_chunks(const uint8_t* __restrict__ leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t k, uint64_t valid,
                                                               const uint8_t* __restrict__ last, uint64_t es, uint8_t* __restrict__ cv)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x, total = n * k;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
      const uint64_t msg = t / k, c = t % k, at = c * BLAKE3_CHUNK, clen = chunk - at < BLAKE3_CHUNK ? chunk - at : BLAKE3_CHUNK;
      uint32_t h[8];
      blake3_chunk(ReadPadded{leaves, (first + msg) * chunk + at, valid, last, es}, clen, c, false, h);
      store_digest32(cv + t * 32, true, h);
    }
  }

  // one level: the k_in nodes of each of n messages (in + 32 (t * k_in + j)) become (k_in + 1) / 2 nodes at out + t * out_stride
  // + 32 j. k_in == 2 is the root level: ROOT is set and `out` is the digests (out_stride 32, any alignment per flags).
  __global__ __launch_bounds__(256) void k_blake3_parents(const uint8_t* __restrict__ in, uint64_t k_in, uint64_t n, uint64_t out_stride, uint32_t flags,
                                                           uint8_t* __restrict__ out)
  {
    const uint64_t k_out = (k_in + 1) / 2, total = n * k_out, step = (uint64_t)gridDim.x * blockDim.x;
    const bool root = k_in == 2, out8 = !root || (flags & HASH_OUT_ALIGNED8) != 0;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
      const uint64_t msg = t / k_out, j = t % k_out;
      const uint4* l = reinterpret_cast<const uint4*>(in + 32 * (msg * k_in + 2 * j)); // the node buffers are 16-aligned
      uint32_t h[8];
      const uint4 a0 = l[0], a1 = l[1];
      const uint32_t left[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      if (2 * j + 1 < k_in) {
        const uint4 b0 = l[2], b1 = l[3];
        const uint32_t right[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        blake3_parent(left, right, root, h);
      } else {
#pragma unroll
        for (int i = 0; i < 8; i++)
          h[i] = left[i];
      }
      store_digest32(out + msg * out_stride + 32 * j, out8, h);
    }
  }

  // ---- the top of a tree in one launch ------------------------------------------------------------------------------------------
  // Once a layer has at most MERKLE_TOP_MAX_HASHES hashes every further layer is smaller still: one launch per layer would be a
  // chain of launches that cannot fill one CU. One block walks them all, a barrier between layers; each layer reads the digests
  // the layer below wrote to global memory (the stored layer buffers, all 8-aligned). The layers may use different hashers.
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

  __global__ __launch_bounds__(MERKLE_TOP_THREADS) void k_merkle_top(const MerkleTopArgs args)
  {
    for (int d = 0; d < args.n; d++) {
      const MerkleTopLayer& l = args.l[d];
      for (uint32_t j = threadIdx.x; j < l.count; j += MERKLE_TOP_THREADS) {
        const ReadAligned rd{l.in + (uint64_t)j * l.chunk, false};
        if (l.kind != HASH_KECCAK) {
          uint32_t h[8];
          if (l.kind == HASH_BLAKE2S)
            blake2s_msg(rd, l.chunk, h);
          else
            blake3_chunk(rd, l.chunk, 0, true, h);
          store_digest32(l.out + (uint64_t)j * 32, true, h);
          continue;
        }
        uint64_t a[25];
        if (l.rate_words == 17) {
          keccak_msg<17>(rd, l.chunk, l.suffix, a);
          store_digest<4>(l.out + (uint64_t)j * 32, true, a);
        } else {
          keccak_msg<9>(rd, l.chunk, l.suffix, a);
          store_digest<8>(l.out + (uint64_t)j * 64, true, a);
        }
      }
      __syncthreads(); // the next layer reads what other waves of this block just wrote
    }
  }

  // ---- proof of work ------------------------------------------------------------------------------------------------------------
  // backend/cpu/src/hash/cpu_pow.cpp: the message of nonce n is challenge | n (8 bytes, little-endian) | padding_size zero bytes, its
  // candidate the digest's first 8 bytes as a little-endian word; n solves when the candidate is below 2^(64 - solution_bits). The
  // messages are never stored: a lane absorbs its nonce's message through ReadPow, so the search touches memory for the challenge
  // (the same words for every lane) and for one result word.
  template <int KIND, int RATE_WORDS>
  __device__ __forceinline__ uint64_t pow_candidate(const ReadPow& rd, uint64_t len, uint32_t suffix)
  {
    if constexpr (KIND == HASH_KECCAK) {
      uint64_t a[25];
      keccak_msg<RATE_WORDS>(rd, len, suffix, a);
      return a[0];
    } else {
      uint32_t h[8];
      blake_msg<KIND>(rd, len, h);
      return h[0] | (uint64_t)h[1] << 32;
    }
  }

  // Nonces [base, base + span), one lane per nonce, grid-stride, so that the grid walks the span in ascending sweeps. *best is the
  // smallest solving nonce seen so far (~0: none; the host never searches that nonce): a solving lane lowers it with a 64-bit
  // atomicMin, so the span's result is its smallest solution whatever order the lanes ran in. A lane skips nonces above the best
  // it last read, and leaves once the first nonce of its block's sweep is above it -- every sweep after that is too. The value
  // read may be stale, which costs hashes and never a result. Nobody waits: a lane reads *best once per nonce of its own and
  // goes on; the read for the next nonce is issued in front of the hash so that it is in flight beside it.
  template <int KIND, int RATE_WORDS>
  __global__ __launch_bounds__(256) void k_pow_search(const uint64_t* __restrict__ challenge, uint32_t size, uint64_t len, uint32_t suffix, uint64_t base, uint64_t span,
                                                       uint64_t threshold, unsigned long long* best)
  {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    uint64_t cur = __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < span; i += step) {
      const uint64_t nonce = base + i; // base + span <= 2^64 - 1024: no wrap
      if (nonce - threadIdx.x > cur) break;
      const bool skip = nonce > cur;
      cur = __hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (skip) continue;
      if (pow_candidate<KIND, RATE_WORDS>(ReadPow{challenge, size, nonce}, len, suffix) < threshold) atomicMin(best, (unsigned long long)nonce);
    }
  }

  // the candidate of one nonce: proof_of_work_verify, and the solver's mined_hash (no two lanes of the search write it)
  template <int KIND, int RATE_WORDS>
  __global__ __launch_bounds__(64) void k_pow_eval(const uint64_t* __restrict__ challenge, uint32_t size, uint64_t len, uint32_t suffix, uint64_t nonce, uint64_t* out)
  {
    if (blockIdx.x == 0 && threadIdx.x == 0) *out = pow_candidate<KIND, RATE_WORDS>(ReadPow{challenge, size, nonce}, len, suffix);
  }

  // ---- host side ----------------------------------------------------------------------------------------------------------------
  struct Hasher {
    int kind;       // HASH_KECCAK, HASH_BLAKE2S, HASH_BLAKE3, HASH_POSEIDON2, HASH_POSEIDON
    int rate_words; // Keccak only -- 17: 256-bit digest, 9: 512-bit digest
    int out_words;
    uint32_t suffix; // Keccak only -- 0x01 Keccak, 0x06 SHA3
    uint64_t chunk;  // default input size, 0 = none
    std::shared_ptr<Poseidon2Hasher> p2; // Poseidon2 only -- field, width, tag and constants, shared with the trees that copy this hasher
    std::shared_ptr<PoseidonHasher> p1;  // Poseidon only -- the same; `chunk` is the only message length it hashes
    uint64_t out_bytes() const { return kind == HASH_POSEIDON2 ? 4 : kind == HASH_KECCAK ? 8ull * out_words : 32; }
    // Blake3 over more than one chunk: several launches and a buffer of chaining values; not for the fused top kernel
    bool multi_chunk(uint64_t len) const { return kind == HASH_BLAKE3 && len > BLAKE3_CHUNK; }
  };

  uint64_t hasher_default_chunk(icicle_hasher_handle_t h) { return h ? reinterpret_cast<const Hasher*>(h)->chunk : 0; } // for fri.hip (common.h)

  static unsigned grid_for(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 22); }

  // Levels above the chaining values of n Blake3 messages of k chunks each (cv, 32 n k bytes): ping-pong between cv and a second
  // buffer of half the size, the root level writes the digests to `out`. Both buffers are released in stream order.
  static icicle_error_t launch_blake3_levels(TempBuf& cv, uint64_t n, uint64_t k, uint32_t flags, uint8_t* out, hipStream_t st)
  {
    TempBuf half;
    if (k > 2) HIP_TRY(half.alloc(32 * n * ((k + 1) / 2), st), ICICLE_ALLOCATION_FAILED);
    uint8_t* buf[2] = {cv.as<uint8_t>(), half.as<uint8_t>()};
    for (int cur = 0; k > 1; k = (k + 1) / 2, cur ^= 1) {
      const uint64_t k_out = (k + 1) / 2;
      k_blake3_parents<<<grid_for(n * k_out), 256, 0, st>>>(buf[cur], k, n, k == 2 ? 32 : 32 * k_out, flags, k == 2 ? out : buf[cur ^ 1]);
      LAUNCH_CHECK("k_blake3_parents", st);
    }
    return ICICLE_SUCCESS;
  }

  static icicle_error_t launch_blake_batch(const Hasher& h, const uint8_t* in, uint64_t len, uint64_t stride, uint64_t n, bool a8, uint32_t flags, uint8_t* out,
                                           hipStream_t st)
  {
    if (h.multi_chunk(len)) {
      const uint64_t k = blake3_chunks_of(len);
      TempBuf cv;
      HIP_TRY(cv.alloc(32 * n * k, st), ICICLE_ALLOCATION_FAILED);
      if (a8)
        k_blake3_chunks<true><<<grid_for(n * k), 256, 0, st>>>(in, len, stride, n, k, flags, cv.as<uint8_t>());
      else
        k_blake3_chunks<false><<<grid_for(n * k), 256, 0, st>>>(in, len, stride, n, k, flags, cv.as<uint8_t>());
      LAUNCH_CHECK("k_blake3_chunks", st);
      return launch_blake3_levels(cv, n, k, flags, out, st);
    }
    if (h.kind == HASH_BLAKE2S && a8)
      k_blake_batch<HASH_BLAKE2S, true><<<grid_for(n), 256, 0, st>>>(in, len, stride, n, flags, out);
    else if (h.kind == HASH_BLAKE2S)
      k_blake_batch<HASH_BLAKE2S, false><<<grid_for(n), 256, 0, st>>>(in, len, stride, n, flags, out);
    else if (a8)
      k_blake_batch<HASH_BLAKE3, true><<<grid_for(n), 256, 0, st>>>(in, len, stride, n, flags, out);
    else
      k_blake_batch<HASH_BLAKE3, false><<<grid_for(n), 256, 0, st>>>(in, len, stride, n, flags, out);
    LAUNCH_CHECK("k_blake_batch", st);
    return ICICLE_SUCCESS;
  }

  static icicle_error_t launch_blake_leaves(const Hasher& h, const uint8_t* leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid, const uint8_t* last,
                                            uint64_t es, uint8_t* out, hipStream_t st)
  {
    if (h.multi_chunk(chunk)) {
      const uint64_t k = blake3_chunks_of(chunk);
      TempBuf cv;
      HIP_TRY(cv.alloc(32 * n * k, st), ICICLE_ALLOCATION_FAILED);
      k_blake3_leaf_chunks<<<grid_for(n * k), 256, 0, st>>>(leaves, chunk, first, n, k, valid, last, es, cv.as<uint8_t>());
      LAUNCH_CHECK("k_blake3_leaf_chunks", st);
      return launch_blake3_levels(cv, n, k, HASH_OUT_ALIGNED8, out, st);
    }
    if (h.kind == HASH_BLAKE2S)
      k_blake_leaves<HASH_BLAKE2S><<<grid_for(n), 256, 0, st>>>(leaves, chunk, first, n, valid, last, es, out);
    else
      k_blake_leaves<HASH_BLAKE3><<<grid_for(n), 256, 0, st>>>(leaves, chunk, first, n, valid, last, es, out);
    LAUNCH_CHECK("k_blake_leaves", st);
    return ICICLE_SUCCESS;
  }

  static icicle_error_t launch_batch(const Hasher& h, const uint8_t* in, uint64_t len, uint64_t stride, uint64_t n, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    uint32_t flags = 0;
    const bool a8 = ((uintptr_t)in & 7) == 0 && (stride & 7) == 0;
    if (((uintptr_t)in & 15) == 0 && (stride & 15) == 0) flags |= HASH_IN_ALIGNED16;
    if (((uintptr_t)out & 7) == 0) flags |= HASH_OUT_ALIGNED8;
    if (h.kind == HASH_POSEIDON2) return poseidon2_launch_batch(*h.p2, in, len, stride, n, out, st);
    if (h.kind == HASH_POSEIDON) return len == h.chunk ? poseidon_launch_batch(*h.p1, in, len, stride, n, out, st) : ICICLE_INVALID_ARGUMENT;
    if (h.kind != HASH_KECCAK) return launch_blake_batch(h, in, len, stride, n, a8, flags, out, st);
    if (h.rate_words == 17 && a8)
      k_keccak_batch<17, 4, true><<<grid_for(n), 256, 0, st>>>(in, len, stride, n, h.suffix, flags, out);
    else if (h.rate_words == 17)
      k_keccak_batch<17, 4, false><<<grid_for(n), 256, 0, st>>>(in, len, stride, n, h.suffix, flags, out);
    else if (a8)
      k_keccak_batch<9, 8, true><<<grid_for(n), 256, 0, st>>>(in, len, stride, n, h.suffix, flags, out);
    else
      k_keccak_batch<9, 8, false><<<grid_for(n), 256, 0, st>>>(in, len, stride, n, h.suffix, flags, out);
    LAUNCH_CHECK("k_keccak_batch", st);
    return ICICLE_SUCCESS;
  }

  static icicle_error_t launch_leaves(const Hasher& h, const uint8_t* leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid, const uint8_t* last,
                                      uint64_t es, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    if (h.kind == HASH_POSEIDON2) return poseidon2_launch_leaves(*h.p2, leaves, chunk, first, n, valid, last, es, out, st);
    if (h.kind == HASH_POSEIDON) return chunk == h.chunk ? poseidon_launch_leaves(*h.p1, leaves, chunk, first, n, valid, last, es, out, st) : ICICLE_INVALID_ARGUMENT;
    if (h.kind != HASH_KECCAK) return launch_blake_leaves(h, leaves, chunk, first, n, valid, last, es, out, st);
    if (h.rate_words == 17)
      k_keccak_leaves<17, 4><<<grid_for(n), 256, 0, st>>>(leaves, chunk, first, n, valid, last, es, h.suffix, out);
    else
      k_keccak_leaves<9, 8><<<grid_for(n), 256, 0, st>>>(leaves, chunk, first, n, valid, last, es, h.suffix, out);
    LAUNCH_CHECK("k_keccak_leaves", st);
    return ICICLE_SUCCESS;
  }

  static Hasher* make_hasher(int rate_words, uint32_t suffix, uint64_t chunk)
  {
    return new (std::nothrow) Hasher{HASH_KECCAK, rate_words, (25 - rate_words) / 2, suffix, chunk};
  }
  static Hasher* make_blake(int kind, uint64_t chunk) { return new (std::nothrow) Hasher{kind, 0, 4, 0, chunk}; }
  // <field>_create_poseidon2_hasher: input_size in elements, 0 = one permutation's worth (t, or t - 1 beside a domain tag)
  static Hasher* make_poseidon2(int field, unsigned t, const uint32_t* domain_tag, unsigned input_size)
  {
    std::shared_ptr<Poseidon2Hasher> p2 = poseidon2_make(field, t, domain_tag);
    if (!p2) return nullptr;
    const uint64_t elems = input_size ? input_size : (domain_tag ? t - 1 : t);
    return new (std::nothrow) Hasher{HASH_POSEIDON2, 0, 0, 0, 4 * elems, std::move(p2)};
  }

  // <field>_create_poseidon_hasher: one permutation per message, so input_size is 0 or the arity (t, or t - 1 beside a domain tag)
  static Hasher* make_poseidon(int field, unsigned t, const uint32_t* domain_tag, unsigned input_size)
  {
    std::shared_ptr<PoseidonHasher> p1 = poseidon_make(field, t, domain_tag);
    if (!p1) return nullptr;
    const unsigned arity = domain_tag ? t - 1 : t;
    if (input_size != 0 && input_size != arity) return nullptr;
    return new (std::nothrow) Hasher{HASH_POSEIDON, 0, 0, 0, 32ull * arity, nullptr, std::move(p1)};
  }

  static icicle_error_t hasher_hash(const Hasher* h, const uint8_t* input, uint64_t input_len, const icicle_hash_config_t* cfg, uint8_t* output)
  {
    if (!h || !cfg) return ICICLE_INVALID_POINTER;
    const uint64_t len = input_len ? input_len : h->chunk;
    if (len == 0) return ICICLE_INVALID_ARGUMENT;
    if (h->kind == HASH_POSEIDON2 && len % 4 != 0) return ICICLE_INVALID_ARGUMENT; // whole field elements
    if (h->kind == HASH_POSEIDON && len != h->chunk) return ICICLE_INVALID_ARGUMENT; // one permutation: exactly the arity
    const uint64_t batch = cfg->batch;
    if (batch == 0) return ICICLE_SUCCESS;
    if (!input || !output) return ICICLE_INVALID_POINTER;
    if (len >= (1ull << 56) / batch) return ICICLE_INVALID_ARGUMENT;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const size_t in_bytes = (size_t)(len * batch), out_bytes = (size_t)(h->out_bytes() * batch);
    TempBuf d_in_tmp, d_out_tmp;
    const uint8_t* d_in = input;
    uint8_t* d_out = output;
    if (!cfg->are_inputs_on_device) {
      HIP_TRY(d_in_tmp.alloc(in_bytes, st), ICICLE_ALLOCATION_FAILED);
      HIP_TRY(hipMemcpyAsync(d_in_tmp.ptr(), input, in_bytes, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
      d_in = d_in_tmp.as<uint8_t>();
    }
    if (!cfg->are_outputs_on_device) {
      HIP_TRY(d_out_tmp.alloc(out_bytes, st), ICICLE_ALLOCATION_FAILED);
      d_out = d_out_tmp.as<uint8_t>();
    }
    ICICLE_TRY(launch_batch(*h, d_in, len, len, batch, d_out, st));
    if (!cfg->are_outputs_on_device) {
      HIP_TRY(hipMemcpyAsync(output, d_out, out_bytes, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
      HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    } else if (!cfg->is_async) {
      HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    }
    return ICICLE_SUCCESS;
  }

  // ---- proof of work, host side --------------------------------------------------------------------------------------------------
  using PowSearchFn = void (*)(const uint64_t*, uint32_t, uint64_t, uint32_t, uint64_t, uint64_t, uint64_t, unsigned long long*);
  using PowEvalFn = void (*)(const uint64_t*, uint32_t, uint64_t, uint32_t, uint64_t, uint64_t*);
  static PowSearchFn pow_search_kernel(const Hasher& h)
  {
    if (h.kind == HASH_BLAKE2S) return k_pow_search<HASH_BLAKE2S, 0>;
    if (h.kind == HASH_BLAKE3) return k_pow_search<HASH_BLAKE3, 0>;
    return h.rate_words == 17 ? k_pow_search<HASH_KECCAK, 17> : k_pow_search<HASH_KECCAK, 9>;
  }
  static PowEvalFn pow_eval_kernel(const Hasher& h)
  {
    if (h.kind == HASH_BLAKE2S) return k_pow_eval<HASH_BLAKE2S, 0>;
    if (h.kind == HASH_BLAKE3) return k_pow_eval<HASH_BLAKE3, 0>;
    return h.rate_words == 17 ? k_pow_eval<HASH_KECCAK, 17> : k_pow_eval<HASH_KECCAK, 9>;
  }

  // The reference's loop hashes 1024 nonces per round and stops in front of the round that would pass 2^64: the nonces it ever
  // tries are [0, 2^64 - 1024). The same bound here keeps ~0 free as the "none yet" value of the result word.
  constexpr uint64_t POW_NONCE_END = 0ull - 1024;
  // Default nonces per launch for a message of one hash block, about half a millisecond of hashing: 2^22 for the Keccak sponges
  // (0.76 ms at 5.5 G hashes/s), 2^24 for Blake2s and Blake3 (0.49 and 0.35 ms). Measured against 2^20 .. 2^32
  // (profiles/hash_merkle_notes.md): a launch, the copy of the result word and the synchronisation cost some 20 us per span, which
  // argues for long spans, but the waves of a grid do not advance in step, so a solution early in a long span is reported late --
  // at 2^28 a 25-bit Keccak-256 solve took five times as long as at 2^22. Halved per doubling of the message's blocks.
  constexpr int POW_SPAN_LOG2_KECCAK = 22, POW_SPAN_LOG2_BLAKE = 24, POW_SPAN_LOG2_MIN = 16, POW_SPAN_LOG2_MAX = 32, POW_SPANS_PER_LOOK = 16;

  struct PowPlan {
    uint64_t len, threshold, start, end; // nonces [start, end)
    int span_log2;
  };

  // everything that can be refused without a device
  static icicle_error_t pow_plan(const Hasher* h, const uint8_t* challenge, uint32_t challenge_size, uint8_t solution_bits, const icicle_pow_config_t* cfg,
                                 PowPlan* p)
  {
    if (!h || !cfg || (!challenge && challenge_size)) return ICICLE_INVALID_POINTER;
    if (h->kind == HASH_POSEIDON2 || h->kind == HASH_POSEIDON) return ICICLE_INVALID_ARGUMENT; // a digest of one field element is no 64-bit candidate
    if (solution_bits < 1 || solution_bits > 60) return ICICLE_INVALID_ARGUMENT;
    p->len = (uint64_t)challenge_size + 8 + cfg->padding_size;
    if (h->kind == HASH_BLAKE3 && p->len > BLAKE3_CHUNK) return ICICLE_INVALID_ARGUMENT; // one chunk: no tree inside a lane
    p->threshold = 1ull << (64 - solution_bits);
    const uint64_t block = h->kind == HASH_KECCAK ? 8ull * h->rate_words : 64, blocks = h->kind == HASH_KECCAK ? p->len / block + 1 : (p->len + block - 1) / block;
    int span = h->kind == HASH_KECCAK ? POW_SPAN_LOG2_KECCAK : POW_SPAN_LOG2_BLAKE;
    for (uint64_t b = 1; b < blocks && span > POW_SPAN_LOG2_MIN; b *= 2)
      span--;
    int lo = 0, hi = 0, count = 64;
    if (cfg->ext) {
      const ConfigExt* e = reinterpret_cast<const ConfigExt*>(cfg->ext);
      span = e->get_int("hip_pow_span_log2", span);
      lo = e->get_int("hip_pow_start_lo", 0), hi = e->get_int("hip_pow_start_hi", 0);
      count = e->get_int("hip_pow_count_log2", 64);
    }
    if (span < 0 || span > POW_SPAN_LOG2_MAX || count < 0 || count > 64) return ICICLE_INVALID_ARGUMENT;
    p->span_log2 = span;
    p->start = (uint64_t)(uint32_t)hi << 32 | (uint32_t)lo;
    p->end = POW_NONCE_END;
    if (count < 64 && p->start + (1ull << count) >= p->start) p->end = std::min<uint64_t>(POW_NONCE_END, p->start + (1ull << count));
    return ICICLE_SUCCESS;
  }

  // device words of one call: [0] the result word of the search, [1] the candidate of k_pow_eval, [2 ..] the challenge as ReadPow
  // reads it. A challenge in device memory is copied there as well: it may lie at any address, and the copy is once per call.
  static icicle_error_t pow_stage_device(TempBuf& buf, const uint8_t* challenge, uint32_t size, bool on_device, std::vector<uint64_t>& host_words, hipStream_t st)
  {
    const uint64_t words = pow_staging_words(size);
    HIP_TRY(buf.alloc(8 * (2 + words), st), ICICLE_ALLOCATION_FAILED);
    uint64_t* d = buf.as<uint64_t>() + 2;
    if (on_device) {
      HIP_TRY(hipMemsetAsync(d, 0, 8 * words, st), ICICLE_COPY_FAILED);
      if (size) HIP_TRY(hipMemcpyAsync(d, challenge, size, hipMemcpyDeviceToDevice, st), ICICLE_COPY_FAILED);
    } else {
      host_words.resize(words);
      pow_stage(challenge, size, host_words.data());
      HIP_TRY(hipMemcpyAsync(d, host_words.data(), 8 * words, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
    }
    return ICICLE_SUCCESS;
  }

  static icicle_error_t pow_eval(const Hasher& h, const TempBuf& buf, uint32_t size, uint64_t len, uint64_t nonce, uint64_t* mined, hipStream_t st)
  {
    uint64_t* d = buf.as<uint64_t>();
    pow_eval_kernel(h)<<<1, 64, 0, st>>>(d + 2, size, len, h.suffix, nonce, d + 1);
    LAUNCH_CHECK("k_pow_eval", st);
    HIP_TRY(hipMemcpyAsync(mined, d + 1, 8, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
    HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    return ICICLE_SUCCESS;
  }

  // Spans in ascending order, one launch each, and a look at the result word after every few of them: the first look that finds a
  // nonce finds the smallest solution of the whole search, since atomicMin keeps the smallest of all spans launched so far. The outputs are host
  // scalars, so the call returns with config->stream drained, whatever is_async says.
  static icicle_error_t pow_solve(const Hasher* h, const uint8_t* challenge, uint32_t challenge_size, uint8_t solution_bits, const icicle_pow_config_t* cfg, bool* found,
                                  uint64_t* nonce, uint64_t* mined_hash)
  {
    PowPlan p;
    ICICLE_TRY(pow_plan(h, challenge, challenge_size, solution_bits, cfg, &p));
    if (!found || !nonce || !mined_hash) return ICICLE_INVALID_POINTER;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    TempBuf buf;
    std::vector<uint64_t> host_words;
    ICICLE_TRY(pow_stage_device(buf, challenge, challenge_size, cfg->is_challenge_on_device, host_words, st));
    uint64_t* d = buf.as<uint64_t>();
    HIP_TRY(hipMemsetAsync(d, 0xFF, 8, st), ICICLE_COPY_FAILED);
    // as many blocks as the device holds at once, so that a sweep of the grid is one stretch of consecutive nonces in flight
    const PowSearchFn kernel = pow_search_kernel(*h);
    int dev = 0, cus = 0, per_cu = 0;
    HIP_TRY(hipGetDevice(&dev), ICICLE_INVALID_DEVICE);
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev), ICICLE_INVALID_DEVICE);
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), 256, 0), ICICLE_INVALID_DEVICE);
    const uint64_t resident = (uint64_t)std::max(cus, 1) * std::max(per_cu, 1), span = 1ull << p.span_log2;
    // Spans launched between two looks at the result word: 1, 2, 4, .. POW_SPANS_PER_LOOK. The spans of a group run one after the
    // other in stream order; those behind a solution cost a launch each and no hashing, since their blocks leave at their first nonce.
    uint64_t best = ~0ull, base = p.start;
    for (int look = 0; base < p.end && best == ~0ull; look++) {
      for (int g = std::min(1 << std::min(look, 30), POW_SPANS_PER_LOOK); g > 0 && base < p.end; g--) {
        const uint64_t n = std::min<uint64_t>(span, p.end - base);
        kernel<<<(unsigned)std::min<uint64_t>((n + 255) / 256, resident), 256, 0, st>>>(d + 2, challenge_size, p.len, h->suffix, base, n, p.threshold,
                                                                                        reinterpret_cast<unsigned long long*>(d));
        LAUNCH_CHECK("k_pow_search", st);
        base += n;
      }
      HIP_TRY(hipMemcpyAsync(&best, d, 8, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
      HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    }
    if (best == ~0ull) {
      *found = false; // nonce and mined_hash stay as they were
      return ICICLE_SUCCESS;
    }
    uint64_t mined = 0;
    ICICLE_TRY(pow_eval(*h, buf, challenge_size, p.len, best, &mined, st));
    *found = true, *nonce = best, *mined_hash = mined;
    return ICICLE_SUCCESS;
  }

  static icicle_error_t pow_verify(const Hasher* h, const uint8_t* challenge, uint32_t challenge_size, uint8_t solution_bits, const icicle_pow_config_t* cfg,
                                   uint64_t nonce, bool* is_correct, uint64_t* mined_hash)
  {
    PowPlan p;
    ICICLE_TRY(pow_plan(h, challenge, challenge_size, solution_bits, cfg, &p));
    if (!is_correct || !mined_hash) return ICICLE_INVALID_POINTER;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    TempBuf buf;
    std::vector<uint64_t> host_words;
    ICICLE_TRY(pow_stage_device(buf, challenge, challenge_size, cfg->is_challenge_on_device, host_words, st));
    uint64_t mined = 0;
    ICICLE_TRY(pow_eval(*h, buf, challenge_size, p.len, nonce, &mined, st));
    *mined_hash = mined, *is_correct = mined < p.threshold;
    return ICICLE_SUCCESS;
  }

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
      if (t.hashers[j].multi_chunk(p.layers[j].chunk) || t.hashers[j].kind == HASH_POSEIDON2 || t.hashers[j].kind == HASH_POSEIDON) fuse_from = j + 1;
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
        k_merkle_top<<<1, MERKLE_TOP_THREADS, 0, st>>>(args);
        LAUNCH_CHECK("k_merkle_top", st);
        return ICICLE_SUCCESS;
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

  static icicle_error_t tree_proof(const Tree* t, const uint8_t* leaves, uint64_t leaves_size, uint64_t leaf_idx, bool pruned,
                                   const icicle_merkle_tree_config_t* cfg, Proof* proof)
  {
    if (!t->built) return ICICLE_INVALID_ARGUMENT;
    const MerklePlan& p = t->plan;
    MerklePadding pad;
    if (merkle_padding(p, leaves_size, cfg->padding_policy, &pad)) return ICICLE_INVALID_ARGUMENT;
    const int L = p.L(), m = t->store_min;
    MerkleProofPlan pp;
    if (merkle_proof_plan(p, leaf_idx, pruned, m, &pp)) return ICICLE_INVALID_ARGUMENT;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = (hipStream_t)cfg->stream;
    const uint64_t c0 = p.layers[0].chunk, es = p.leaf_element_size;
    const bool dev_leaves = cfg->is_leaves_on_device, last_value = cfg->padding_policy == MERKLE_PAD_LAST && pad.pad_bytes > 0;

    // everything that lives on the device is gathered into one staging buffer -- [leaf chunk | last element | path] -- and
    // comes back in one copy behind one synchronisation; host-resident pieces are copied on the host
    const uint64_t path_at = (c0 + es + 15) & ~15ull, stage_bytes = path_at + pp.path_size;
    TempBuf d_stage, d_sub, d_low;
    HIP_TRY(d_stage.alloc(stage_bytes, st), ICICLE_ALLOCATION_FAILED);
    uint8_t* stage = d_stage.as<uint8_t>();
    bool device_pieces = false;

    // the leaf: the part of chunk0 that lies inside the leaves
    const uint64_t leaf_lo = pp.chunk0 * c0, leaf_real = leaf_lo >= leaves_size ? 0 : std::min(c0, leaves_size - leaf_lo);
    if (dev_leaves) {
      if (leaf_real) HIP_TRY(hipMemcpyAsync(stage, leaves + leaf_lo, leaf_real, hipMemcpyDeviceToDevice, st), ICICLE_COPY_FAILED);
      if (last_value) HIP_TRY(hipMemcpyAsync(stage + c0, leaves + pad.last_off, es, hipMemcpyDeviceToDevice, st), ICICLE_COPY_FAILED);
      device_pieces = leaf_real || last_value;
    }

    // layers below store_min: re-hash the sub-tree under the on-path node of layer store_min
    uint8_t* sub_out[MERKLE_MAX_LAYERS];
    uint64_t sub_node0[MERKLE_MAX_LAYERS];
    if (m > 0) {
      LeafSource src{leaves, leaves_size, last_value ? leaves + pad.last_off : nullptr};
      if (!dev_leaves) {
        const uint64_t lo = pp.sub_first * c0, real = lo >= leaves_size ? 0 : std::min(pp.sub_count * c0, leaves_size - lo);
        const uint64_t last_at = (real + 15) & ~15ull;
        HIP_TRY(d_sub.alloc(last_at + es, st), ICICLE_ALLOCATION_FAILED);
        if (real) HIP_TRY(hipMemcpyAsync(d_sub.ptr(), leaves + lo, real, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
        if (last_value) HIP_TRY(hipMemcpyAsync(d_sub.as<uint8_t>() + last_at, leaves + pad.last_off, es, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
        // only offsets in [lo, lo + real) are read through this pointer
        src.base = reinterpret_cast<const uint8_t*>((uintptr_t)d_sub.ptr() - lo);
        src.last = last_value ? d_sub.as<uint8_t>() + last_at : nullptr;
      }
      uint64_t bytes = 0;
      for (int i = 0; i < m; i++) {
        const uint64_t ratio = p.layers[0].count / p.layers[i].count; // layer-0 chunks per node of layer i
        sub_node0[i] = pp.sub_first / ratio;
        bytes += (pp.sub_count / ratio * p.layers[i].out + 15) & ~15ull;
      }
      HIP_TRY(d_low.alloc(bytes, st), ICICLE_ALLOCATION_FAILED);
      bytes = 0;
      for (int i = 0; i < m; i++) {
        sub_out[i] = d_low.as<uint8_t>() + bytes;
        bytes += (pp.sub_count / (p.layers[0].count / p.layers[i].count) * p.layers[i].out + 15) & ~15ull;
      }
      ICICLE_TRY(hash_layers(*t, src, pp.sub_first, pp.sub_count, m, sub_out, top_max_of(cfg), st));
    }

    proof->pruned = pruned;
    proof->leaf_idx = leaf_idx;
    proof->path.assign(pp.path_size, 0);
    // the path, group by group; pruned: the two runs around the on-path digest
    for (int i = 0; i + 1 < L; i++) {
      const MerkleProofStep& s = pp.steps[i];
      const uint64_t o = p.layers[i].out;
      const uint64_t run_src[2] = {s.src_off, pruned ? s.src_off + s.skip_off + o : 0};
      const uint64_t run_len[2] = {pruned ? s.skip_off : s.len, pruned ? s.len - s.skip_off - o : 0};
      uint64_t dst = s.dst_off;
      for (int r = 0; r < 2; r++) {
        if (run_len[r] == 0) continue;
        if (i < m) {
          HIP_TRY(hipMemcpyAsync(stage + path_at + dst, sub_out[i] + (run_src[r] - sub_node0[i] * o), run_len[r], hipMemcpyDeviceToDevice, st), ICICLE_COPY_FAILED);
          device_pieces = true;
        } else if (t->on_device) {
          HIP_TRY(hipMemcpyAsync(stage + path_at + dst, t->d_store + t->store_off(i) + run_src[r], run_len[r], hipMemcpyDeviceToDevice, st), ICICLE_COPY_FAILED);
          device_pieces = true;
        }
        dst += run_len[r];
      }
    }
    std::vector<uint8_t> host_stage;
    if (device_pieces) {
      host_stage.resize(stage_bytes);
      HIP_TRY(hipMemcpyAsync(host_stage.data(), stage, stage_bytes, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
    }
    // the one synchronisation: also orders this call behind an asynchronous build on the same stream (h_store, h_root)
    HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    if (device_pieces) std::memcpy(proof->path.data(), host_stage.data() + path_at, pp.path_size);
    if (!t->on_device)
      for (int i = m; i + 1 < L; i++) {
        const MerkleProofStep& s = pp.steps[i];
        const uint64_t o = p.layers[i].out;
        const uint8_t* g = t->h_store + t->store_off(i) + s.src_off;
        if (pruned) {
          std::memcpy(proof->path.data() + s.dst_off, g, s.skip_off);
          std::memcpy(proof->path.data() + s.dst_off + s.skip_off, g + s.skip_off + o, s.len - s.skip_off - o);
        } else {
          std::memcpy(proof->path.data() + s.dst_off, g, s.len);
        }
      }
    // the leaf chunk, padded per policy
    proof->leaf.assign(c0, 0);
    const uint8_t* real_src = dev_leaves ? host_stage.data() : leaves + leaf_lo;
    if (leaf_real) std::memcpy(proof->leaf.data(), real_src, leaf_real);
    if (last_value) {
      const uint8_t* last = dev_leaves ? host_stage.data() + c0 : leaves + pad.last_off;
      for (uint64_t q = leaf_real; q < c0; q++)
        proof->leaf[q] = last[(leaf_lo + q) % es];
    }
    proof->root.assign(t->h_root, t->h_root + p.layers[L - 1].out);
    return ICICLE_SUCCESS;
  }

  // the reference's walk (merkle_tree.h:148-203): hash the leaf, then one hash per layer over the path's group with the previous
  // digest in its place. All hashes run on the device in one stream-ordered chain. Pruned: every digest is written straight
  // into its hole in the next layer's input. Full path: the digests come back and are compared with the path on the host.
  static icicle_error_t tree_verify(const Tree* t, const Proof* pr, bool* valid)
  {
    const MerklePlan& p = t->plan;
    const int L = p.L();
    *valid = false;
    if (pr->leaf.empty()) return ICICLE_INVALID_ARGUMENT;
    if (pr->path.size() != (pr->pruned ? p.pruned_path : p.full_path)) return ICICLE_INVALID_ARGUMENT;
    if (pr->root.size() != p.layers[L - 1].out) return ICICLE_SUCCESS; // cannot be this tree's root
    if (pr->leaf_idx > (~0ull) / p.leaf_element_size) return ICICLE_INVALID_ARGUMENT;
    ICICLE_TRY(bind_current_device());
    hipStream_t st = nullptr;
    std::vector<uint64_t> offs;
    merkle_verify_offsets(p, pr->leaf_idx, pr->leaf.size(), &offs);
    // host image of the device buffer: [leaf | input of layer 1 | .. | input of layer L-1 | L digests of 64 bytes], all 16-aligned
    std::vector<uint64_t> in_at(L, 0);
    uint64_t at = (pr->leaf.size() + 15) & ~15ull;
    for (int i = 1; i < L; i++) {
      in_at[i] = at;
      at += (p.layers[i].chunk + 15) & ~15ull;
    }
    const uint64_t dig_at = at, total = dig_at + 64ull * L;
    std::vector<uint8_t> img(total, 0);
    std::memcpy(img.data(), pr->leaf.data(), pr->leaf.size());
    const uint8_t* path = pr->path.data();
    for (int i = 1; i < L; i++) {
      const uint64_t c = p.layers[i].chunk, o = p.layers[i - 1].out, off = offs[i - 1];
      if (pr->pruned) {
        std::memcpy(img.data() + in_at[i], path, off);
        std::memcpy(img.data() + in_at[i] + off + o, path + off, c - o - off);
        path += c - o;
      } else {
        std::memcpy(img.data() + in_at[i], path, c);
        path += c;
      }
    }
    TempBuf d_buf;
    HIP_TRY(d_buf.alloc(total, st), ICICLE_ALLOCATION_FAILED);
    uint8_t* d = d_buf.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(d, img.data(), dig_at, hipMemcpyHostToDevice, st), ICICLE_COPY_FAILED);
    for (int i = 0; i < L; i++) {
      const uint64_t len = i == 0 ? pr->leaf.size() : p.layers[i].chunk;
      uint8_t* out = d + dig_at + 64ull * i;
      if (pr->pruned && i + 1 < L) out = d + in_at[i + 1] + offs[i];
      ICICLE_TRY(launch_batch(t->hashers[i], d + in_at[i], len, len, 1, out, st));
    }
    HIP_TRY(hipMemcpyAsync(img.data() + dig_at, d + dig_at, 64ull * L, hipMemcpyDeviceToHost, st), ICICLE_COPY_FAILED);
    HIP_TRY(hipStreamSynchronize(st), ICICLE_SYNCHRONIZATION_FAILED);
    bool ok = true;
    if (!pr->pruned)
      for (int i = 1; i < L && ok; i++)
        ok = std::memcmp(img.data() + dig_at + 64ull * (i - 1), img.data() + in_at[i] + offs[i - 1], p.layers[i - 1].out) == 0;
    *valid = ok && std::memcmp(img.data() + dig_at + 64ull * (L - 1), pr->root.data(), pr->root.size()) == 0;
    return ICICLE_SUCCESS;
  }

  // ---- many openings, many verifications ------------------------------------------------------------------------------------------
  // Pinned host memory for a batch call's one upload and one download. hipHostMalloc costs more than a whole batch, so the buffers
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

  // `count` proofs of one tree in one gather launch, one copy back and one synchronisation; proofs[i] comes out as tree_proof
  // leaves it for idx[i]. Everything that can be refused is refused before the device is touched or a proof written.
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

  // tree_verify over `count` proofs: one host image of every proof's layer inputs goes up in one copy, every layer is hashed in one
  // launch over all proofs (layer 0: one launch per distinct leaf size, the proofs ordered by it), a pruned proof's digests are
  // scattered into their holes in the next layer's inputs, and all digests come back in one copy behind one synchronisation.
  static icicle_error_t tree_verify_batch(const Tree* t, const Proof* const* prs, uint64_t count, bool* valid)
  {
    const MerklePlan& p = t->plan;
    const int L = p.L();
    for (uint64_t i = 0; i < count; i++)
      valid[i] = false;
    // the single call's checks, in its order, proof by proof; a root of another size is no root of this tree, and no error
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
      if (i == 0) {
        for (uint64_t k0 = 0; k0 < n;) { // runs of one leaf size
          const uint64_t len = prs[live[k0]]->leaf.size();
          uint64_t k1 = k0 + 1;
          while (k1 < n && prs[live[k1]]->leaf.size() == len)
            k1++;
          ICICLE_TRY(launch_batch(t->hashers[0], d + in_at[0] + k0 * in_stride[0], len, in_stride[0], k1 - k0, d + dig_at[0] + k0 * p.layers[0].out, st));
          k0 = k1;
        }
      } else {
        ICICLE_TRY(launch_batch(t->hashers[i], d + in_at[i], p.layers[i].chunk, in_stride[i], n, d + dig_at[i], st));
      }
      if (pruned && i + 1 < L) {
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

static_assert(sizeof(icicle_hash_config_t) == 32 && offsetof(icicle_hash_config_t, batch) == 8 && offsetof(icicle_hash_config_t, are_inputs_on_device) == 16 &&
                offsetof(icicle_hash_config_t, are_outputs_on_device) == 17 && offsetof(icicle_hash_config_t, is_async) == 18 && offsetof(icicle_hash_config_t, ext) == 24,
              "HashConfig layout (include/icicle/hash/hash_config.h)");
static_assert(sizeof(icicle_merkle_tree_config_t) == 24 && offsetof(icicle_merkle_tree_config_t, is_leaves_on_device) == 8 &&
                offsetof(icicle_merkle_tree_config_t, is_tree_on_device) == 9 && offsetof(icicle_merkle_tree_config_t, is_async) == 10 &&
                offsetof(icicle_merkle_tree_config_t, padding_policy) == 12 && offsetof(icicle_merkle_tree_config_t, ext) == 16,
              "MerkleTreeConfig layout (include/icicle/merkle/merkle_tree_config.h)");
static_assert(sizeof(icicle_pow_config_t) == 32 && offsetof(icicle_pow_config_t, is_challenge_on_device) == 8 && offsetof(icicle_pow_config_t, padding_size) == 12 &&
                offsetof(icicle_pow_config_t, is_async) == 16 && offsetof(icicle_pow_config_t, ext) == 24,
              "PowConfig layout (include/icicle/hash/pow.h)");

#define HASH_GUARDED(expr, on_throw)                                                                                   \
  try {                                                                                                                \
    return (expr);                                                                                                     \
  } catch (...) {                                                                                                      \
    return on_throw;                                                                                                   \
  }

extern "C" {

icicle_hasher_handle_t icicle_create_keccak_256(uint64_t input_chunk_size) { return (icicle_hasher_handle_t)make_hasher(17, 0x01, input_chunk_size); }
icicle_hasher_handle_t icicle_create_keccak_512(uint64_t input_chunk_size) { return (icicle_hasher_handle_t)make_hasher(9, 0x01, input_chunk_size); }
icicle_hasher_handle_t icicle_create_sha3_256(uint64_t input_chunk_size) { return (icicle_hasher_handle_t)make_hasher(17, 0x06, input_chunk_size); }
icicle_hasher_handle_t icicle_create_sha3_512(uint64_t input_chunk_size) { return (icicle_hasher_handle_t)make_hasher(9, 0x06, input_chunk_size); }
icicle_hasher_handle_t icicle_create_blake2s(uint64_t input_chunk_size) { return (icicle_hasher_handle_t)make_blake(HASH_BLAKE2S, input_chunk_size); }
icicle_hasher_handle_t icicle_create_blake3(uint64_t input_chunk_size) { return (icicle_hasher_handle_t)make_blake(HASH_BLAKE3, input_chunk_size); }

icicle_hasher_handle_t babybear_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon2(0, t, domain_tag, input_size), nullptr)
}
icicle_hasher_handle_t koalabear_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon2(1, t, domain_tag, input_size), nullptr)
}
icicle_hasher_handle_t bn254_create_poseidon_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon(0, t, domain_tag, input_size), nullptr)
}
icicle_hasher_handle_t bls12_381_create_poseidon_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon(1, t, domain_tag, input_size), nullptr)
}
icicle_hasher_handle_t bls12_377_create_poseidon_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon(2, t, domain_tag, input_size), nullptr)
}
icicle_hasher_handle_t grumpkin_create_poseidon_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon(3, t, domain_tag, input_size), nullptr)
}

icicle_error_t icicle_hasher_hash(icicle_hasher_handle_t h, const uint8_t* input, uint64_t input_len, const icicle_hash_config_t* config, uint8_t* output)
{
  HASH_GUARDED(hasher_hash((const Hasher*)h, input, input_len, config, output), ICICLE_ALLOCATION_FAILED)
}

uint64_t icicle_hasher_output_size(icicle_hasher_handle_t h) { return h ? ((const Hasher*)h)->out_bytes() : 0; }

icicle_error_t icicle_hasher_delete(icicle_hasher_handle_t h)
{
  if (!h) return ICICLE_INVALID_POINTER;
  delete (Hasher*)h;
  return ICICLE_SUCCESS;
}

icicle_error_t proof_of_work(icicle_hasher_handle_t hasher, const uint8_t* challenge, uint32_t challenge_size, uint8_t solution_bits, const icicle_pow_config_t* config,
                             bool* found, uint64_t* nonce, uint64_t* mined_hash)
{
  HASH_GUARDED(pow_solve((const Hasher*)hasher, challenge, challenge_size, solution_bits, config, found, nonce, mined_hash), ICICLE_ALLOCATION_FAILED)
}

icicle_error_t proof_of_work_verify(icicle_hasher_handle_t hasher, const uint8_t* challenge, uint32_t challenge_size, uint8_t solution_bits,
                                    const icicle_pow_config_t* config, uint64_t nonce, bool* is_correct, uint64_t* mined_hash)
{
  HASH_GUARDED(pow_verify((const Hasher*)hasher, challenge, challenge_size, solution_bits, config, nonce, is_correct, mined_hash), ICICLE_ALLOCATION_FAILED)
}

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
  HASH_GUARDED(tree_proof((const Tree*)tree, leaves, leaves_size, leaf_idx, is_pruned, config, (Proof*)merkle_proof), ICICLE_ALLOCATION_FAILED)
}

icicle_error_t icicle_merkle_tree_verify(icicle_merkle_tree_handle_t tree, icicle_merkle_proof_handle_t merkle_proof, bool* valid)
{
  if (!tree || !merkle_proof || !valid) return ICICLE_INVALID_POINTER;
  HASH_GUARDED(tree_verify((const Tree*)tree, (const Proof*)merkle_proof, valid), ICICLE_ALLOCATION_FAILED)
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
