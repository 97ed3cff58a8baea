// Host check of the Blake2s / Blake3 device code (icicle_amd/csrc/blake.hpp over the readers of hash_readers.hpp): a flat C surface
// that tests/test_blake_cpu.py compares with the Python model (tests/blake_model.py). A Blake3 message of more than one chunk is
// walked the way hash.hip walks it: one chaining value per chunk, then level by level over adjacent pairs, an odd last node
// carried up. With -DBLAKE_HARNESS_MAIN it is a stand-alone program over the same lengths (known answers checked, a checksum
// printed), the form to run under -fsanitize=address,undefined.
#include "../icicle_amd/csrc/blake.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace icicle_hip;

enum { KIND_BLAKE2S = 1, KIND_BLAKE3 = 2 };

static void put(uint8_t* out, const uint32_t (&h)[8])
{
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 4; k++)
      out[4 * i + k] = (uint8_t)(h[i] >> (8 * k));
}

// reader_at(at) reads the message from byte `at` on
template <class F>
static void hash_any(int kind, uint64_t len, F reader_at, uint8_t* out)
{
  uint32_t h[8];
  if (kind == KIND_BLAKE2S) {
    blake2s_msg(reader_at(0), len, h);
    return put(out, h);
  }
  const uint64_t k = blake3_chunks_of(len);
  if (k == 1) {
    blake3_chunk(reader_at(0), len, 0, true, h);
    return put(out, h);
  }
  struct Cv {
    uint32_t w[8];
  };
  std::vector<Cv> nodes(k);
  for (uint64_t c = 0; c < k; c++) {
    const uint64_t at = c * BLAKE3_CHUNK;
    blake3_chunk(reader_at(at), len - at < BLAKE3_CHUNK ? len - at : BLAKE3_CHUNK, c, false, nodes[c].w);
  }
  for (uint64_t n = k; n > 1; n = (n + 1) / 2) {
    std::vector<Cv> up((n + 1) / 2);
    for (uint64_t j = 0; j < up.size(); j++) {
      if (2 * j + 1 < n)
        blake3_parent(nodes[2 * j].w, nodes[2 * j + 1].w, n == 2, up[j].w);
      else
        up[j] = nodes[2 * j];
    }
    nodes.swap(up);
  }
  put(out, nodes[0].w);
}

// reader 0: ReadAligned (p 8-aligned; 128-bit pairs where it is 16-aligned), 1: ReadBytes
extern "C" int bh_hash(int kind, int reader, const uint8_t* p, uint64_t len, uint8_t* out)
{
  if (reader == 0) {
    if ((uintptr_t)p & 7) return 1;
    const bool a16 = ((uintptr_t)p & 15) == 0;
    hash_any(kind, len, [&](uint64_t at) { return ReadAligned{p + at, a16}; }, out);
  } else {
    hash_any(kind, len, [&](uint64_t at) { return ReadBytes{p + at}; }, out);
  }
  return 0;
}

// the layer-0 chunk at byte `pos` of a tree's padded leaves: base[0, valid) are the leaves, `last` the LastValue element or NULL
extern "C" int bh_hash_padded(int kind, const uint8_t* base, uint64_t pos, uint64_t chunk, uint64_t valid, const uint8_t* last, uint64_t es, uint8_t* out)
{
  hash_any(kind, chunk, [&](uint64_t at) { return ReadPadded{base, pos + at, valid, last, es}; }, out);
  return 0;
}

#ifdef BLAKE_HARNESS_MAIN
static bool is_hex(const uint8_t* d, const char* hex)
{
  char buf[65];
  for (int i = 0; i < 32; i++)
    snprintf(buf + 2 * i, 3, "%02x", d[i]);
  return std::strcmp(buf, hex) == 0;
}

int main()
{
  std::vector<uint64_t> lens;
  for (uint64_t n = 0; n <= 300; n++)
    lens.push_back(n);
  for (uint64_t n : {1000, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073, 4096, 4097, 5120, 7168, 7169, 8192, 8193, 9216, 16384, 16385})
    lens.push_back(n);
  uint64_t checksum = 0;
  int bad = 0;
  uint8_t a[32], b[32], c[32];
  for (uint64_t n : lens) {
    std::vector<uint64_t> store(n / 8 + 4); // 8-aligned; the byte reader starts one byte in
    uint8_t* al = reinterpret_cast<uint8_t*>(store.data()) + 8;
    std::vector<uint8_t> odd(n + 1);
    for (uint64_t i = 0; i < n; i++)
      al[i] = odd[i + 1] = (uint8_t)(i % 251);
    for (int kind : {KIND_BLAKE2S, KIND_BLAKE3}) {
      bh_hash(kind, 0, al, n, a);
      bh_hash(kind, 1, odd.data() + 1, n, b);
      bad += std::memcmp(a, b, 32) != 0;
      if (n >= 40 && n % 20 == 0) {
        // a chunk of n bytes whose leaves end 40 bytes before its end: zeros, then copies of the last 20-byte element
        std::vector<uint8_t> zero(al, al + n), lastv(al, al + n);
        for (uint64_t i = n - 40; i < n; i++)
          zero[i] = 0, lastv[i] = n >= 60 ? al[n - 60 + i % 20] : 0;
        const uint64_t pos = 3 * n; // the chunk is the fourth of its tree: `base` is addressed from the tree's first byte
        std::vector<uint8_t> tree(pos + n);
        std::memcpy(tree.data() + pos, al, n);
        bh_hash_padded(kind, tree.data(), pos, n, pos + n - 40, nullptr, 20, a);
        bh_hash(kind, 1, zero.data(), n, c);
        bad += std::memcmp(a, c, 32) != 0;
        if (n >= 60) {
          bh_hash_padded(kind, tree.data(), pos, n, pos + n - 40, tree.data() + pos + n - 60, 20, a);
          bh_hash(kind, 1, lastv.data(), n, c);
          bad += std::memcmp(a, c, 32) != 0;
        }
      }
      for (int i = 0; i < 32; i++)
        checksum = checksum * 131 + b[i];
      if (n == 0 && kind == KIND_BLAKE3) bad += !is_hex(b, "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262");
      if (n == 0 && kind == KIND_BLAKE2S) bad += !is_hex(b, "69217a3079908094e11121d042354a7c1f55b6482ca1a51e1b250dfd1ed0eef9");
    }
  }
  const char* kat = "Hello world I am blake2s";
  bh_hash(KIND_BLAKE2S, 1, reinterpret_cast<const uint8_t*>(kat), std::strlen(kat), a);
  bad += !is_hex(a, "291c4b3648438cc57d1e965ee52e5572e8dc4938bc960e22d6ebe3a280aea759");
  printf("%zu lengths, checksum %016llx, %d mismatches\n", lens.size(), (unsigned long long)checksum, bad);
  return bad != 0;
}
#endif
