// Blake2s-256 and Blake3 (default hash mode, 32-byte output), one lane per message or per 1024-byte chunk. Included from hash.hip;
// host-compilable (no HIP runtime), so tests/blake_host_harness.cpp runs the same compression and absorb code on the CPU.
//
// Written from RFC 7693 (Blake2s) and the BLAKE3 specification ("BLAKE3: one function, fast everywhere", sections 2.1 - 2.6):
//   * IV (both hashes, RFC 7693 section 2.6 / BLAKE3 table 1): the first 32 bits of the fractional parts of the square roots of
//     the first eight primes,
//       [isqrt(p << 64) & 0xFFFFFFFF for p in (2, 3, 5, 7, 11, 13, 17, 19)]
//   * Blake2s message schedule: the ten rows SIGMA[0 .. 9] of RFC 7693 section 2.7; round r takes row r. Parameter block word 0 is
//     0x01010020: digest length 32, key length 0, fanout 1, depth 1 (section 2.5); rotations 16, 12, 8, 7 (section 2.1).
//   * Blake3 message schedule: round 0 takes the block's words in order, every further round the previous round's order under the
//     permutation of BLAKE3 table 2 (2 6 3 10 7 0 4 13 1 11 12 5 9 14 15 8): sched(r, i) = sched(r - 1, PERM[i]). Seven rounds,
//     the G function of Blake2s with the message words taken in pairs (section 2.2); flags of table 3.
// (tests/blake_model.py holds the same derivations; its Blake2s is checked against hashlib, its Blake3 against recorded digests.)
//
// Every index into h / m / v is a compile-time constant (the rounds are template instantiations), so the arrays live in registers
// and the Blake3 permutation renames registers instead of moving data.
#pragma once
#include "hash_readers.hpp"

namespace icicle_hip {

  constexpr uint32_t BLAKE_IV[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};

  constexpr int BLAKE2S_SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
  constexpr int BLAKE3_PERM[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
  constexpr int blake3_sched(int r, int i) { return r == 0 ? i : blake3_sched(r - 1, BLAKE3_PERM[i]); }
  // index of the message word that position I of round R takes, as a constant expression
  template <int R, int I>
  constexpr int BLAKE2S_S = BLAKE2S_SIGMA[R][I];
  template <int R, int I>
  constexpr int BLAKE3_S = blake3_sched(R, I);

  enum : uint32_t { BLAKE3_CHUNK_START = 1, BLAKE3_CHUNK_END = 2, BLAKE3_PARENT = 4, BLAKE3_ROOT = 8 };
  constexpr uint64_t BLAKE3_CHUNK = 1024;

  template <int N>
  ICICLE_HD uint32_t blake_rotr(uint32_t x)
  {
#if defined(__clang__)
    return __builtin_rotateright32(x, N); // one v_alignbit_b32
#else
    return (x >> N) | (x << (32 - N));
#endif
  }

  ICICLE_HD void blake_g(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t x, uint32_t y)
  {
    a = a + b + x, d = blake_rotr<16>(d ^ a), c = c + d, b = blake_rotr<12>(b ^ c);
    a = a + b + y, d = blake_rotr<8>(d ^ a), c = c + d, b = blake_rotr<7>(b ^ c);
  }

// columns, then diagonals; S(i) is the index of the i-th message word of the round
#define BLAKE_ROUND_BODY(S)                                                                                            \
  blake_g(v[0], v[4], v[8], v[12], m[S(0)], m[S(1)]), blake_g(v[1], v[5], v[9], v[13], m[S(2)], m[S(3)]);                             \
  blake_g(v[2], v[6], v[10], v[14], m[S(4)], m[S(5)]), blake_g(v[3], v[7], v[11], v[15], m[S(6)], m[S(7)]);                           \
  blake_g(v[0], v[5], v[10], v[15], m[S(8)], m[S(9)]), blake_g(v[1], v[6], v[11], v[12], m[S(10)], m[S(11)]);                         \
  blake_g(v[2], v[7], v[8], v[13], m[S(12)], m[S(13)]), blake_g(v[3], v[4], v[9], v[14], m[S(14)], m[S(15)]);

  template <int R>
  ICICLE_HD void blake2s_round(uint32_t (&v)[16], const uint32_t (&m)[16])
  {
#define BLAKE_S(i) BLAKE2S_S<R, i>
    BLAKE_ROUND_BODY(BLAKE_S)
#undef BLAKE_S
  }
  template <int R>
  ICICLE_HD void blake3_round(uint32_t (&v)[16], const uint32_t (&m)[16])
  {
#define BLAKE_S(i) BLAKE3_S<R, i>
    BLAKE_ROUND_BODY(BLAKE_S)
#undef BLAKE_S
  }
#undef BLAKE_ROUND_BODY

  // RFC 7693 section 3.2: t = bytes absorbed so far, this block included
  ICICLE_HD void blake2s_compress(uint32_t (&h)[8], const uint32_t (&m)[16], uint64_t t, bool last)
  {
    uint32_t v[16];
#pragma unroll
    for (int i = 0; i < 8; i++)
      v[i] = h[i], v[i + 8] = BLAKE_IV[i];
    v[12] ^= (uint32_t)t, v[13] ^= (uint32_t)(t >> 32);
    if (last) v[14] = ~v[14];
    blake2s_round<0>(v, m), blake2s_round<1>(v, m), blake2s_round<2>(v, m), blake2s_round<3>(v, m), blake2s_round<4>(v, m);
    blake2s_round<5>(v, m), blake2s_round<6>(v, m), blake2s_round<7>(v, m), blake2s_round<8>(v, m), blake2s_round<9>(v, m);
#pragma unroll
    for (int i = 0; i < 8; i++)
      h[i] ^= v[i] ^ v[i + 8];
  }

  // BLAKE3 section 2.2, truncated to the first eight output words: the new chaining value (or, with ROOT, the digest)
  ICICLE_HD void blake3_compress(uint32_t (&h)[8], const uint32_t (&m)[16], uint64_t counter, uint32_t block_len, uint32_t flags)
  {
    uint32_t v[16];
#pragma unroll
    for (int i = 0; i < 8; i++)
      v[i] = h[i];
    v[8] = BLAKE_IV[0], v[9] = BLAKE_IV[1], v[10] = BLAKE_IV[2], v[11] = BLAKE_IV[3];
    v[12] = (uint32_t)counter, v[13] = (uint32_t)(counter >> 32), v[14] = block_len, v[15] = flags;
    blake3_round<0>(v, m), blake3_round<1>(v, m), blake3_round<2>(v, m), blake3_round<3>(v, m);
    blake3_round<4>(v, m), blake3_round<5>(v, m), blake3_round<6>(v, m);
#pragma unroll
    for (int i = 0; i < 8; i++)
      h[i] = v[i] ^ v[i + 8];
  }

  // the block at `off`: 64 message bytes, or the last `rem` < 64 of them, zero-filled
  template <class RD>
  ICICLE_HD void blake_load_block(const RD& rd, uint64_t off, uint32_t rem, uint32_t (&m)[16])
  {
    if (rem >= 64) {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        uint64_t lo, hi;
        rd.pair(off + 16 * i, lo, hi);
        m[4 * i] = (uint32_t)lo, m[4 * i + 1] = (uint32_t)(lo >> 32), m[4 * i + 2] = (uint32_t)hi, m[4 * i + 3] = (uint32_t)(hi >> 32);
      }
    } else {
      // words [0, wi) are whole, word wi holds the last rem % 8 bytes
      const uint32_t wi = rem >> 3, nb = rem & 7;
      uint64_t part = 0;
      for (uint32_t k = 0; k < nb; k++)
        part |= (uint64_t)rd.byte(off + 8 * wi + k) << (8 * k);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        uint64_t w = 0;
        if ((uint32_t)i < wi) w = rd.word(off + 8 * i);
        if ((uint32_t)i == wi) w = part;
        m[2 * i] = (uint32_t)w, m[2 * i + 1] = (uint32_t)(w >> 32);
      }
    }
  }

  // Blake2s-256 of one message of `len` bytes: every block but the last is 64 bytes; the last one (the only one of an empty
  // message, a full one where len is a multiple of 64) carries the final flag
  template <class RD>
  ICICLE_HD void blake2s_msg(const RD& rd, uint64_t len, uint32_t (&h)[8])
  {
#pragma unroll
    for (int i = 0; i < 8; i++)
      h[i] = BLAKE_IV[i];
    h[0] ^= 0x01010020u;
    uint64_t off = 0;
    for (;;) { // one call site of the compression
      const bool last = len - off <= 64;
      const uint32_t n = last ? (uint32_t)(len - off) : 64;
      uint32_t m[16];
      blake_load_block(rd, off, n, m);
      blake2s_compress(h, m, off + n, last);
      if (last) break;
      off += 64;
    }
  }

  // One Blake3 chunk (len <= 1024 bytes, chunk index `counter`): h becomes its chaining value -- or, with root = true (the message
  // is this one chunk), the digest
  template <class RD>
  ICICLE_HD void blake3_chunk(const RD& rd, uint64_t len, uint64_t counter, bool root, uint32_t (&h)[8])
  {
#pragma unroll
    for (int i = 0; i < 8; i++)
      h[i] = BLAKE_IV[i];
    uint64_t off = 0;
    for (;;) {
      const bool last = len - off <= 64;
      const uint32_t n = last ? (uint32_t)(len - off) : 64;
      uint32_t m[16];
      blake_load_block(rd, off, n, m);
      blake3_compress(h, m, counter, n, (off == 0 ? BLAKE3_CHUNK_START : 0u) | (last ? BLAKE3_CHUNK_END | (root ? BLAKE3_ROOT : 0u) : 0u));
      if (last) break;
      off += 64;
    }
  }

  // parent node over two chaining values (section 2.5): key = IV, counter 0, block length 64
  ICICLE_HD void blake3_parent(const uint32_t (&left)[8], const uint32_t (&right)[8], bool root, uint32_t (&h)[8])
  {
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 8; i++)
      m[i] = left[i], m[i + 8] = right[i], h[i] = BLAKE_IV[i];
    blake3_compress(h, m, 0, 64, BLAKE3_PARENT | (root ? BLAKE3_ROOT : 0u));
  }

  // A message of more than one chunk is a binary tree over its chunks whose left subtree holds the largest power of two of
  // chunks below the total (section 2.1). Pairing adjacent nodes level by level and carrying an odd last node up unchanged
  // builds that same tree, so a level is data-parallel: nodes_in nodes become (nodes_in + 1) / 2.
  inline uint64_t blake3_chunks_of(uint64_t len) { return len <= BLAKE3_CHUNK ? 1 : (len + BLAKE3_CHUNK - 1) / BLAKE3_CHUNK; }

} // namespace icicle_hip
