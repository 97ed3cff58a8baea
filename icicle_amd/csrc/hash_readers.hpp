// Where a lane's message bytes come from: the four readers every hash of hash.hip absorbs through. No HIP runtime in here, so
// the host harnesses (tests/blake_host_harness.cpp, tests/pow_host_harness.cpp) compile the readers and the code over them with g++.
#pragma once
#include <cstdint>
#include <cstring>

// qualifier of code that runs in a kernel and, for the CPU tests, on the host
#if defined(__HIPCC__)
#define ICICLE_HD __host__ __device__ __forceinline__
#else
#define ICICLE_HD inline
#endif

namespace icicle_hip {

  // 8-aligned message: 64-bit loads, 128-bit ones where message and offset are 16-aligned
  struct ReadAligned {
    const uint8_t* p;
    bool a16;
    ICICLE_HD uint64_t word(uint64_t off) const
    {
#if defined(__HIPCC__)
      return *reinterpret_cast<const uint64_t*>(p + off);
#else // the host build reads byte buffers: no load through a pointer of another type (little-endian hosts only, as the device is)
      uint64_t w;
      std::memcpy(&w, p + off, 8);
      return w;
#endif
    }
    ICICLE_HD uint32_t byte(uint64_t off) const { return p[off]; }
    ICICLE_HD void pair(uint64_t off, uint64_t& lo, uint64_t& hi) const
    {
#if defined(__HIPCC__)
      if (a16 && (off & 15) == 0) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p + off);
        lo = v.x, hi = v.y;
        return;
      }
#endif
      lo = word(off), hi = word(off + 8);
    }
  };
  // any alignment
  struct ReadBytes {
    const uint8_t* p;
    ICICLE_HD uint32_t byte(uint64_t off) const { return p[off]; }
    ICICLE_HD uint64_t word(uint64_t off) const
    {
      uint64_t w = 0;
#pragma unroll
      for (int k = 0; k < 8; k++)
        w |= (uint64_t)p[off + k] << (8 * k);
      return w;
    }
    ICICLE_HD void pair(uint64_t off, uint64_t& lo, uint64_t& hi) const { lo = word(off), hi = word(off + 8); }
  };
  // a layer-0 chunk of a tree that reaches into the padding: byte q of the padded leaves is leaves[q] below `valid`, beyond it
  // 0 (ZeroPadding: last == nullptr) or byte q % es of the last element (LastValue; valid and the chunk size are multiples of es)
  struct ReadPadded {
    const uint8_t* base; // leaves, addressed by the byte offset in the whole tree's leaves
    uint64_t pos;        // offset of this chunk
    uint64_t valid;
    const uint8_t* last;
    uint64_t es;
    ICICLE_HD uint32_t byte(uint64_t off) const
    {
      const uint64_t q = pos + off;
      if (q < valid) return base[q];
      return last ? last[q % es] : 0;
    }
    ICICLE_HD uint64_t word(uint64_t off) const
    {
      uint64_t w = 0;
      for (int k = 0; k < 8; k++)
        w |= (uint64_t)byte(off + k) << (8 * k);
      return w;
    }
    ICICLE_HD void pair(uint64_t off, uint64_t& lo, uint64_t& hi) const { lo = word(off), hi = word(off + 8); }
  };
  // The message of a proof-of-work nonce (cpu_pow.cpp): challenge[0, size), the nonce as 8 little-endian bytes, zeros from there
  // on. Nothing is stored per nonce: every lane reads the one challenge, at addresses that do not depend on the lane, and shifts
  // its own nonce in. `c` is the challenge copied into pow_staging_words(size) 8-aligned words, zero behind byte `size`
  // (pow_stage), so that the word in which challenge and nonce meet is one load and two shifts.
  struct ReadPow {
    const uint64_t* c;
    uint32_t size;
    uint64_t nonce;
    ICICLE_HD uint64_t word8(uint64_t j) const // message bytes [8 j, 8 j + 8)
    {
      const uint64_t cw = size >> 3;
      const uint32_t sh = 8 * (size & 7);
      uint64_t w = j <= cw ? c[j] : 0; // c[cw]: the challenge's last size % 8 bytes, zero-filled
      if (j == cw) w |= nonce << sh;
      if (j == cw + 1 && sh) w |= nonce >> (64 - sh);
      return w;
    }
    ICICLE_HD uint64_t word(uint64_t off) const
    {
      const uint32_t sh = 8 * (uint32_t)(off & 7);
      const uint64_t lo = word8(off >> 3);
      return sh ? lo >> sh | word8((off >> 3) + 1) << (64 - sh) : lo;
    }
    ICICLE_HD uint32_t byte(uint64_t off) const { return (uint32_t)(word8(off >> 3) >> (8 * (off & 7))) & 0xFF; }
    ICICLE_HD void pair(uint64_t off, uint64_t& lo, uint64_t& hi) const { lo = word(off), hi = word(off + 8); }
  };
  inline uint64_t pow_staging_words(uint32_t size) { return (uint64_t)(size >> 3) + 1; }
  // fills the staging words of ReadPow from the challenge's bytes (host memory)
  inline void pow_stage(const uint8_t* challenge, uint32_t size, uint64_t* words)
  {
    std::memset(words, 0, 8 * pow_staging_words(size));
    if (size) std::memcpy(words, challenge, size);
  }

} // namespace icicle_hip
