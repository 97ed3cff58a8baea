// Host-only part of FRI (fri.hip): the parameter checks, the round and tree shapes, the bytes the transcript hashes, the map from
// a digest to a field element, and the query sampler. No HIP in here, so tests/fri_host_harness.cpp and
// tests/fri_wide_host_harness.cpp compile it with g++ and compare it with the Python models (tests/fri_model.py, fri_model_wide.py).
//
// Reference: icicle/src/fri/fri.cpp:329-431 (shapes, check_if_valid), include/icicle/fri/fri_transcript.h (entry_0, the round,
// proof-of-work and query-phase inputs), include/icicle/utils/rand_gen.h (std::mt19937 + std::uniform_int_distribution<size_t>).
// The distribution is not specified by the C++ standard; what the reference's build computes is written out below, so that a proof
// does not depend on the C++ library this project is built against.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace icicle_hip {

  struct FriPlan {
    uint32_t log_n = 0;      // log2 of the input size
    uint32_t rounds = 0;     // log_n - log2(stopping_degree + 1)
    uint64_t n = 0;          // input size in elements
    uint64_t final_size = 0; // stopping_degree + 1
    uint64_t round_size(uint32_t r) const { return n >> r; }       // elements of layer r, r = 0 .. rounds (the last: final poly)
    uint32_t tree_layers(uint32_t r) const { return log_n - r + 1; } // the leaves hasher + log2(round_size) compress layers
  };

  inline bool fri_is_pow2(uint64_t v) { return v != 0 && (v & (v - 1)) == 0; }
  inline uint32_t fri_log2(uint64_t v)
  {
    uint32_t l = 0;
    while (v > 1)
      v >>= 1, l++;
    return l;
  }

  // 0 = fine, 1 = invalid argument: the rules that do not depend on the input size. The reference's (fri.cpp:405-431): folding
  // factor 2, queries > 0, compress arity 2. Ours on top, where the reference leaves its final polynomial zero: stopping_degree + 1
  // a power of two.
  inline int fri_check_config(uint64_t folding_factor, uint64_t stopping_degree, uint64_t nof_queries, uint64_t compress_chunk, uint64_t compress_out)
  {
    if (folding_factor != 2 || nof_queries == 0) return 1;
    if (compress_out == 0 || compress_chunk % compress_out != 0 || compress_chunk / compress_out != 2) return 1;
    return fri_is_pow2(stopping_degree + 1) ? 0 : 1;
  }

  // 0 = fine, 1 = invalid argument: fri_check_config and the rules of the size -- a power of two (the reference's), queries <= n / 2
  // (the reference's), and at least one round (ours: stopping_degree + 1 < n).
  inline int fri_make_plan(uint64_t n, uint64_t folding_factor, uint64_t stopping_degree, uint64_t nof_queries, uint64_t compress_chunk, uint64_t compress_out,
                           FriPlan* p)
  {
    if (fri_check_config(folding_factor, stopping_degree, nof_queries, compress_chunk, compress_out)) return 1;
    if (!fri_is_pow2(n) || n >= (1ull << 32)) return 1; // the sampler draws from n - final_size + 1 < 2^32 values
    const uint64_t fs = stopping_degree + 1;
    if (nof_queries > n / 2 || fs >= n) return 1;
    p->n = n, p->final_size = fs, p->log_n = fri_log2(n), p->rounds = p->log_n - fri_log2(fs);
    return 0;
  }

  // ---- transcript bytes ----------------------------------------------------------------------------------------------------------
  struct FriLabels {
    const uint8_t *domain_separator, *round_challenge, *commit_phase, *nonce, *public_state;
    size_t domain_separator_len, round_challenge_len, commit_phase_len, nonce_len, public_state_len;
  };

  class FriTranscriptBytes
  {
  public:
    FriTranscriptBytes(const FriLabels& l, uint32_t log_n) : m_l(l)
    {
      put(m_entry0, l.domain_separator, l.domain_separator_len);
      put_le32(m_entry0, log_n);
      put(m_entry0, l.public_state, l.public_state_len);
    }
    const std::vector<uint8_t>& entry0() const { return m_entry0; }
    // entry0 | prev | round_challenge_label | commit_phase_label | root; prev: the seed (round 0) or the previous alpha
    std::vector<uint8_t> round_input(const uint8_t* prev, size_t prev_len, const uint8_t* root, size_t root_len) const
    {
      std::vector<uint8_t> v = m_entry0;
      put(v, prev, prev_len);
      put(v, m_l.round_challenge, m_l.round_challenge_len);
      put(v, m_l.commit_phase, m_l.commit_phase_len);
      put(v, root, root_len);
      return v;
    }
    // entry0 | alpha_last | nonce_label: the challenge the proof of work appends its nonce to
    std::vector<uint8_t> pow_challenge(const uint8_t* alpha, size_t alpha_len) const
    {
      std::vector<uint8_t> v = m_entry0;
      put(v, alpha, alpha_len);
      put(v, m_l.nonce, m_l.nonce_len);
      return v;
    }
    // with a proof of work: entry0 | nonce_label | LE32(nonce) -- only the low 32 bits of the nonce; without: entry0 | alpha_last
    std::vector<uint8_t> query_input(bool with_pow, const uint8_t* alpha, size_t alpha_len, uint64_t nonce) const
    {
      std::vector<uint8_t> v = m_entry0;
      if (with_pow) {
        put(v, m_l.nonce, m_l.nonce_len);
        put_le32(v, (uint32_t)nonce);
      } else {
        put(v, alpha, alpha_len);
      }
      return v;
    }

  private:
    static void put(std::vector<uint8_t>& v, const uint8_t* p, size_t n)
    {
      if (p && n) v.insert(v.end(), p, p + n);
    }
    static void put_le32(std::vector<uint8_t>& v, uint32_t x)
    {
      for (int i = 0; i < 4; i++)
        v.push_back((uint8_t)(x >> (8 * i)));
    }
    FriLabels m_l;
    std::vector<uint8_t> m_entry0;
  };

  // F(digest). One word: the whole digest as one little-endian integer mod p. Four words (quartic extension): coefficient k is the
  // little-endian u32 at bytes 4k .. 4k+3 mod p, so only the first 16 bytes count.
  inline void fri_field_from_digest(const uint8_t* digest, size_t len, uint32_t p, int words, uint32_t* out)
  {
    if (words == 1) {
      uint64_t r = 0;
      for (size_t i = len; i-- > 0;)
        r = ((r << 8) | digest[i]) % p;
      out[0] = (uint32_t)r;
      return;
    }
    for (int k = 0; k < words; k++) {
      uint32_t w = 0;
      for (int b = 0; b < 4; b++)
        if ((size_t)(4 * k + b) < len) w |= (uint32_t)digest[4 * k + b] << (8 * b);
      out[k] = w % p;
    }
  }

  // F(digest) of the fields wider than 32 bits (the reference's from(bytes, size): math/modular_arithmetic.h, goldilocks.h). A scalar
  // of `nw` words: the whole digest as one little-endian integer mod p, 32- and 64-byte digests alike -- bit by bit from the top,
  // r = 2r + bit with one conditional subtraction, so no wide division is needed. p: nw words, nw <= 8.
  inline void fri_wide_from_digest(const uint8_t* digest, size_t len, const uint32_t* p, int nw, uint32_t* out)
  {
    uint32_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t bit = 8 * len; bit-- > 0;) {
      uint32_t carry = (digest[bit >> 3] >> (bit & 7)) & 1u;
      for (int i = 0; i < nw; i++) {
        const uint32_t top = r[i] >> 31;
        r[i] = (r[i] << 1) | carry;
        carry = top;
      }
      bool ge = carry != 0; // 2r + bit reached 2^(32 nw) > p
      if (!ge) {
        ge = true; // equal to p
        for (int i = nw - 1; i >= 0; i--)
          if (r[i] != p[i]) {
            ge = r[i] > p[i];
            break;
          }
      }
      if (ge) {
        uint64_t borrow = 0;
        for (int i = 0; i < nw; i++) {
          const uint64_t d = (uint64_t)r[i] - p[i] - borrow;
          r[i] = (uint32_t)d;
          borrow = (d >> 63) & 1;
        }
      }
    }
    for (int i = 0; i < nw; i++)
      out[i] = r[i];
  }
  // Goldilocks' quadratic extension (complex_extension.h): coefficient k is the little-endian u64 at bytes 8k .. 8k+7 mod p, so only
  // the first 16 bytes count; a digest shorter than that gives zero, as the reference does. p: two words, out: four.
  inline void fri_gold_ext_from_digest(const uint8_t* digest, size_t len, const uint32_t* p, uint32_t* out)
  {
    for (int k = 0; k < 2; k++) {
      if (len < 16)
        out[2 * k] = out[2 * k + 1] = 0;
      else
        fri_wide_from_digest(digest + 8 * k, 8, p, 2, out + 2 * k);
    }
  }

  // ---- query sampler ---------------------------------------------------------------------------------------------------------------
  // MT19937 (Matsumoto, Nishimura 1998) with the init_genrand seeding of the 2002 version -- what std::mt19937 is defined to be.
  class FriMt19937
  {
  public:
    explicit FriMt19937(uint32_t seed)
    {
      m_s[0] = seed;
      for (int i = 1; i < 624; i++)
        m_s[i] = 1812433253u * (m_s[i - 1] ^ (m_s[i - 1] >> 30)) + (uint32_t)i;
      m_i = 624;
    }
    uint32_t next()
    {
      if (m_i >= 624) twist();
      uint32_t y = m_s[m_i++];
      y ^= y >> 11;
      y ^= (y << 7) & 0x9d2c5680u;
      y ^= (y << 15) & 0xefc60000u;
      y ^= y >> 18;
      return y;
    }

  private:
    void twist()
    {
      for (int i = 0; i < 624; i++) {
        const uint32_t y = (m_s[i] & 0x80000000u) | (m_s[(i + 1) % 624] & 0x7fffffffu);
        m_s[i] = m_s[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1) ? 0x9908b0dfu : 0u);
      }
      m_i = 0;
    }
    uint32_t m_s[624];
    int m_i;
  };

  inline uint32_t fri_query_seed(const uint8_t* digest) // the low 32 bits of the digest's first 8 bytes as a little-endian word
  {
    return (uint32_t)digest[0] | (uint32_t)digest[1] << 8 | (uint32_t)digest[2] << 16 | (uint32_t)digest[3] << 24;
  }

  // One query from the INCLUSIVE range [final_size, n] (so q may equal n; positions are taken mod the round size): the 32-bit
  // multiply-and-reject draw over R = n - final_size + 1 values. R < 2^32 is required.
  inline uint64_t fri_draw_query(FriMt19937& mt, uint64_t final_size, uint64_t n)
  {
    const uint32_t R = (uint32_t)(n - final_size + 1);
    uint64_t m = (uint64_t)mt.next() * R;
    if ((uint32_t)m < R) {
      const uint32_t threshold = (0u - R) % R; // (2^32 - R) % R
      while ((uint32_t)m < threshold)
        m = (uint64_t)mt.next() * R;
    }
    return final_size + (m >> 32);
  }

  inline std::vector<uint64_t> fri_draw_queries(const uint8_t* digest, uint64_t nof_queries, uint64_t final_size, uint64_t n)
  {
    FriMt19937 mt(fri_query_seed(digest));
    std::vector<uint64_t> q(nof_queries);
    for (auto& v : q)
      v = fri_draw_query(mt, final_size, n);
    return q;
  }

  // slot 2j of round r proves leaf q % size, slot 2j + 1 its symmetric position (q + size / 2) % size
  inline uint64_t fri_leaf_index(uint64_t q, uint64_t round_size, bool symmetric) { return (q + (symmetric ? round_size / 2 : 0)) % round_size; }

} // namespace icicle_hip
