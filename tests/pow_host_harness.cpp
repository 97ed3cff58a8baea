// Host check of the proof-of-work message reader (ReadPow, icicle_amd/csrc/hash_readers.hpp): the Blake absorb code of blake.hpp runs
// over it on the CPU, and the synthesised message is dumped through each of the reader's three accessors; tests/test_pow_cpu.py
// compares both with messages built in Python. With -DPOW_HARNESS_MAIN it is a stand-alone program over the same sizes that checks
// the reader against a message built here, the form to run under -fsanitize=address,undefined.
#include "../icicle_amd/csrc/blake.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace icicle_hip;

enum { KIND_BLAKE2S = 1, KIND_BLAKE3 = 2 };

// exactly the words the device gets: pow_staging_words(size) of them and not one more
static std::vector<uint64_t> staged(const uint8_t* challenge, uint32_t size)
{
  std::vector<uint64_t> w(pow_staging_words(size));
  pow_stage(challenge, size, w.data());
  return w;
}

// Blake2s (kind 1) or one Blake3 chunk (kind 2, len <= 1024) of challenge | nonce | zeros up to len
extern "C" int ph_hash(int kind, const uint8_t* challenge, uint32_t size, uint64_t nonce, uint64_t len, uint8_t* out)
{
  if (len < (uint64_t)size + 8 || (kind == KIND_BLAKE3 && len > BLAKE3_CHUNK)) return 1;
  const std::vector<uint64_t> w = staged(challenge, size);
  const ReadPow rd{w.data(), size, nonce};
  uint32_t h[8];
  if (kind == KIND_BLAKE2S)
    blake2s_msg(rd, len, h);
  else
    blake3_chunk(rd, len, 0, true, h);
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 4; k++)
      out[4 * i + k] = (uint8_t)(h[i] >> (8 * k));
  return 0;
}

// the first len message bytes as the reader serves them -- how 0: byte(), 1: word() at every offset from `shift` in steps of 8,
// 2: pair() in steps of 16
extern "C" int ph_message(const uint8_t* challenge, uint32_t size, uint64_t nonce, uint64_t len, int how, uint32_t shift, uint8_t* out)
{
  const std::vector<uint64_t> w = staged(challenge, size);
  const ReadPow rd{w.data(), size, nonce};
  std::vector<uint8_t> m(len + 32, 0);
  if (how == 0) {
    for (uint64_t i = 0; i < len; i++)
      m[i] = (uint8_t)rd.byte(i);
  } else {
    for (uint64_t off = 0; off < shift && off < len; off++)
      m[off] = (uint8_t)rd.byte(off);
    for (uint64_t off = shift; off < len; off += how == 1 ? 8 : 16) {
      uint64_t v[2] = {0, 0};
      if (how == 1)
        v[0] = rd.word(off);
      else
        rd.pair(off, v[0], v[1]);
      std::memcpy(m.data() + off, v, how == 1 ? 8 : 16);
    }
  }
  std::memcpy(out, m.data(), len);
  return 0;
}

#ifdef POW_HARNESS_MAIN
int main()
{
  int bad = 0, cases = 0;
  uint64_t checksum = 0;
  for (uint32_t size : {0, 1, 7, 8, 21, 31, 32, 33, 56, 60, 64, 120})
    for (uint32_t pad : {0, 3, 7, 24})
      for (uint64_t nonce : {0ull, 1ull, 0xFFFFFFFFull, 0x100000000ull, ~0ull, 0x0123456789ABCDEFull}) {
        std::vector<uint8_t> c(size); // exactly `size` bytes: a read past the challenge is the sanitizer's to find
        for (uint32_t i = 0; i < size; i++)
          c[i] = (uint8_t)(i * 37 + 11);
        const uint64_t len = (uint64_t)size + 8 + pad;
        std::vector<uint8_t> want(len, 0), got(len);
        if (size) std::memcpy(want.data(), c.data(), size);
        std::memcpy(want.data() + size, &nonce, 8);
        for (int how = 0; how < 3; how++)
          for (uint32_t shift = 0; shift < (how ? 8u : 1u); shift++) {
            ph_message(c.data(), size, nonce, len, how, shift, got.data());
            bad += got != want;
            cases++;
          }
        uint8_t d[32];
        for (int kind : {KIND_BLAKE2S, KIND_BLAKE3}) {
          bad += ph_hash(kind, c.data(), size, nonce, len, d);
          for (int i = 0; i < 32; i++)
            checksum = checksum * 131 + d[i];
        }
      }
  printf("%d reader cases, checksum %016llx, %d mismatches\n", cases, (unsigned long long)checksum, bad);
  return bad != 0;
}
#endif
