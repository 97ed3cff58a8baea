// Keccak / SHA3 / Blake2s / Blake3 batch hashing and the proof-of-work search on the device, and every hash kernel a Merkle tree
// runs (the tree itself is merkle.hip, which reaches this file through hash_merkle.h). The Blake compression and
// absorb code is blake.hpp, the four message readers hash_readers.hpp (both also compile for the host); the kernels over them are below.
// Poseidon2 over BabyBear and KoalaBear hashes through the same hasher and tree paths; its kernels and its state are poseidon2.hip.
// Poseidon over the 256-bit scalar fields does the same through poseidon.hip, Poseidon2 over them through poseidon2_wide.hip,
// Poseidon2 over Goldilocks through poseidon2_gold.hip.
//
// C ABI of the reference: icicle/src/hash/hash_c_api.cpp (icicle_create_keccak_256 .. icicle_create_blake3, icicle_hasher_hash),
// include/icicle/hash/pow.h (proof_of_work, proof_of_work_verify); configs include/icicle/hash/hash_config.h, pow.h.
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
#include "hash_merkle.h"
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
  // the hasher kinds (HASH_KECCAK, HASH_BLAKE2S, HASH_BLAKE3, ..) are hash_merkle.h
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
  // MerkleTopLayer, MerkleTopArgs and the switch point MERKLE_TOP_MAX_HASHES are hash_merkle.h: merkle.hip fills them in.
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

  icicle_error_t launch_merkle_top(const MerkleTopArgs& args, hipStream_t st)
  {
    k_merkle_top<<<1, MERKLE_TOP_THREADS, 0, st>>>(args);
    LAUNCH_CHECK("k_merkle_top", st);
    return ICICLE_SUCCESS;
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
  // struct Hasher and grid_for are hash_merkle.h

  uint64_t hasher_default_chunk(icicle_hasher_handle_t h) { return h ? reinterpret_cast<const Hasher*>(h)->chunk : 0; } // for fri.hip (common.h)

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

  icicle_error_t launch_batch(const Hasher& h, const uint8_t* in, uint64_t len, uint64_t stride, uint64_t n, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    uint32_t flags = 0;
    const bool a8 = ((uintptr_t)in & 7) == 0 && (stride & 7) == 0;
    if (((uintptr_t)in & 15) == 0 && (stride & 15) == 0) flags |= HASH_IN_ALIGNED16;
    if (((uintptr_t)out & 7) == 0) flags |= HASH_OUT_ALIGNED8;
    if (h.kind == HASH_POSEIDON2) return poseidon2_launch_batch(*h.p2, in, len, stride, n, out, st);
    if (h.kind == HASH_POSEIDON2_WIDE) return poseidon2_wide_launch_batch(*h.p2w, in, len, stride, n, out, st);
    if (h.kind == HASH_POSEIDON2_GOLD) return poseidon2_gold_launch_batch(*h.p2g, in, len, stride, n, out, st);
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

  icicle_error_t launch_leaves(const Hasher& h, const uint8_t* leaves, uint64_t chunk, uint64_t first, uint64_t n, uint64_t valid, const uint8_t* last,
                               uint64_t es, uint8_t* out, hipStream_t st)
  {
    if (n == 0) return ICICLE_SUCCESS;
    if (h.kind == HASH_POSEIDON2) return poseidon2_launch_leaves(*h.p2, leaves, chunk, first, n, valid, last, es, out, st);
    if (h.kind == HASH_POSEIDON2_WIDE) return poseidon2_wide_launch_leaves(*h.p2w, leaves, chunk, first, n, valid, last, es, out, st);
    if (h.kind == HASH_POSEIDON2_GOLD) return poseidon2_gold_launch_leaves(*h.p2g, leaves, chunk, first, n, valid, last, es, out, st);
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

  // the same over a 256-bit field (poseidon2_wide.hip): elements of 32 bytes
  static Hasher* make_poseidon2_wide(int field, unsigned t, const uint32_t* domain_tag, unsigned input_size)
  {
    std::shared_ptr<Poseidon2WideHasher> p2w = poseidon2_wide_make(field, t, domain_tag);
    if (!p2w) return nullptr;
    const uint64_t elems = input_size ? input_size : (domain_tag ? t - 1 : t);
    return new (std::nothrow) Hasher{HASH_POSEIDON2_WIDE, 0, 0, 0, 32 * elems, nullptr, nullptr, std::move(p2w)};
  }

  // the same over Goldilocks (poseidon2_gold.hip): elements of 8 bytes, the tag one element of two little-endian words
  static Hasher* make_poseidon2_gold(unsigned t, const uint32_t* domain_tag, unsigned input_size)
  {
    std::shared_ptr<Poseidon2GoldHasher> p2g = poseidon2_gold_make(t, domain_tag);
    if (!p2g) return nullptr;
    const uint64_t elems = input_size ? input_size : (domain_tag ? t - 1 : t);
    return new (std::nothrow) Hasher{HASH_POSEIDON2_GOLD, 0, 0, 0, 8 * elems, nullptr, nullptr, nullptr, std::move(p2g)};
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
    if (h->kind == HASH_POSEIDON2_WIDE && len % 32 != 0) return ICICLE_INVALID_ARGUMENT;
    if (h->kind == HASH_POSEIDON2_GOLD && len % 8 != 0) return ICICLE_INVALID_ARGUMENT;
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
    if (hash_kind_is_field(h->kind)) return ICICLE_INVALID_ARGUMENT; // a digest of one field element is no 64-bit candidate
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

} // namespace icicle_hip

using namespace icicle_hip;

static_assert(sizeof(icicle_hash_config_t) == 32 && offsetof(icicle_hash_config_t, batch) == 8 && offsetof(icicle_hash_config_t, are_inputs_on_device) == 16 &&
                offsetof(icicle_hash_config_t, are_outputs_on_device) == 17 && offsetof(icicle_hash_config_t, is_async) == 18 && offsetof(icicle_hash_config_t, ext) == 24,
              "HashConfig layout (include/icicle/hash/hash_config.h)");
static_assert(sizeof(icicle_pow_config_t) == 32 && offsetof(icicle_pow_config_t, is_challenge_on_device) == 8 && offsetof(icicle_pow_config_t, padding_size) == 12 &&
                offsetof(icicle_pow_config_t, is_async) == 16 && offsetof(icicle_pow_config_t, ext) == 24,
              "PowConfig layout (include/icicle/hash/pow.h)");

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
icicle_hasher_handle_t goldilocks_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon2_gold(t, domain_tag, input_size), nullptr)
}
icicle_hasher_handle_t bn254_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon2_wide(0, t, domain_tag, input_size), nullptr)
}
icicle_hasher_handle_t bls12_381_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon2_wide(1, t, domain_tag, input_size), nullptr)
}
icicle_hasher_handle_t bls12_377_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon2_wide(2, t, domain_tag, input_size), nullptr)
}
icicle_hasher_handle_t grumpkin_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon2_wide(3, t, domain_tag, input_size), nullptr)
}
icicle_hasher_handle_t stark252_create_poseidon2_hasher(unsigned t, const uint32_t* domain_tag, unsigned input_size)
{
  HASH_GUARDED((icicle_hasher_handle_t)make_poseidon2_wide(4, t, domain_tag, input_size), nullptr)
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

} // extern "C"
