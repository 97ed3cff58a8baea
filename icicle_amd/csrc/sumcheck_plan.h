// Host-only part of sumcheck (sumcheck.hip): the bytes the transcript hashes, the map from a digest to a field element for one-word
// and eight-word fields, plain host arithmetic over those fields, the evaluation of a compiled program, the Lagrange evaluation and the
// verifier. No HIP in here, so tests/sumcheck_host_harness.cpp compiles it with g++ and compares it with the Python model
// (tests/sumcheck_model.py).
//
// Reference: include/icicle/sumcheck/sumcheck_transcript.h (round 0 and round i inputs), sumcheck.h:123-193 (verify, Lagrange),
// include/icicle/math/modular_arithmetic.h:458 (from(bytes): the digest as one little-endian integer mod p).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <vector>
#include "program_plan.h"

namespace icicle_hip {

  inline bool sumcheck_is_pow2(uint64_t v) { return v != 0 && (v & (v - 1)) == 0; }
  inline uint32_t sumcheck_log2(uint64_t v)
  {
    uint32_t l = 0;
    while (v > 1)
      v >>= 1, l++;
    return l;
  }

  // ---- arithmetic mod p on canonical little-endian words; p < 2^(32 words - 1). Cold paths only: the verifier and the tests. ----
  struct HostField {
    int words = 1;
    uint32_t p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HostField() = default;
    HostField(const uint32_t* modulus, int nof_words) : words(nof_words) { std::memcpy(p, modulus, 4 * nof_words); }

    bool geq_p(const uint32_t* a) const
    {
      for (int i = words; i-- > 0;)
        if (a[i] != p[i]) return a[i] > p[i];
      return true;
    }
    bool is_canonical(const uint32_t* a) const { return !geq_p(a); }
    bool eq(const uint32_t* a, const uint32_t* b) const { return std::memcmp(a, b, 4 * words) == 0; }
    void sub_p(uint32_t* a) const
    {
      uint64_t borrow = 0;
      for (int i = 0; i < words; i++) {
        const uint64_t d = (uint64_t)a[i] - p[i] - borrow;
        a[i] = (uint32_t)d, borrow = (d >> 32) & 1;
      }
    }
    void add(const uint32_t* a, const uint32_t* b, uint32_t* out) const
    {
      uint32_t r[8];
      uint64_t c = 0;
      for (int i = 0; i < words; i++) {
        c += (uint64_t)a[i] + b[i];
        r[i] = (uint32_t)c, c >>= 32;
      }
      if (geq_p(r)) sub_p(r); // no carry out: 2p < 2^(32 words)
      std::memcpy(out, r, 4 * words);
    }
    void sub(const uint32_t* a, const uint32_t* b, uint32_t* out) const
    {
      uint32_t r[8];
      uint64_t borrow = 0;
      for (int i = 0; i < words; i++) {
        const uint64_t d = (uint64_t)a[i] - b[i] - borrow;
        r[i] = (uint32_t)d, borrow = (d >> 32) & 1;
      }
      if (borrow) {
        uint64_t c = 0;
        for (int i = 0; i < words; i++) {
          c += (uint64_t)r[i] + p[i];
          r[i] = (uint32_t)c, c >>= 32;
        }
      }
      std::memcpy(out, r, 4 * words);
    }
    // `nof_words` little-endian words as one integer, mod p
    void reduce(const uint32_t* wide, int nof_words, uint32_t* out) const
    {
      uint32_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int bit = 32 * nof_words; bit-- > 0;) {
        uint32_t c = (wide[bit / 32] >> (bit % 32)) & 1;
        for (int i = 0; i < words; i++) { // r = 2 r + bit < 2p
          const uint32_t top = r[i] >> 31;
          r[i] = (r[i] << 1) | c, c = top;
        }
        if (geq_p(r)) sub_p(r);
      }
      std::memcpy(out, r, 4 * words);
    }
    void mul(const uint32_t* a, const uint32_t* b, uint32_t* out) const
    {
      uint32_t wide[16] = {0};
      for (int i = 0; i < words; i++) {
        uint64_t c = 0;
        for (int j = 0; j < words; j++) {
          c += (uint64_t)a[i] * b[j] + wide[i + j];
          wide[i + j] = (uint32_t)c, c >>= 32;
        }
        wide[i + words] = (uint32_t)c;
      }
      reduce(wide, 2 * words, out);
    }
    void from_u32(uint32_t v, uint32_t* out) const
    {
      uint32_t w[8] = {v, 0, 0, 0, 0, 0, 0, 0};
      reduce(w, words, out);
    }
    // F(digest): the whole digest as one little-endian integer, mod p
    void from_digest(const uint8_t* digest, size_t len, uint32_t* out) const
    {
      std::vector<uint32_t> w((len + 3) / 4 + 1, 0);
      for (size_t i = 0; i < len; i++)
        w[i / 4] |= (uint32_t)digest[i] << (8 * (i % 4));
      reduce(w.data(), (int)((len + 3) / 4), out);
    }
    void inv(const uint32_t* a, uint32_t* out) const // a^(p - 2); 0 gives 0
    {
      uint32_t e[8], r[8], base[8];
      std::memcpy(e, p, 4 * words), std::memcpy(base, a, 4 * words);
      uint64_t borrow = 2;
      for (int i = 0; i < words; i++) {
        const uint64_t d = (uint64_t)e[i] - borrow;
        e[i] = (uint32_t)d, borrow = (d >> 32) & 1;
      }
      from_u32(1, r);
      for (int bit = 0; bit < 32 * words; bit++) {
        if ((e[bit / 32] >> (bit % 32)) & 1) mul(r, base, r);
        mul(base, base, base);
      }
      std::memcpy(out, r, 4 * words);
    }
  };

  // the value of a compiled program at `inputs` (nof_inputs elements back to back); false: an inverse, or a variable out of range
  inline bool program_eval(const HostField& f, const CompiledProgram& p, const uint32_t* inputs, uint32_t* out)
  {
    const int w = f.words;
    if (p.predefined >= 0) {
      uint32_t t[8];
      f.mul(inputs, inputs + w, t);
      f.sub(t, inputs + 2 * w, t);
      if (p.predefined == PROG_EQ_X_AB_MINUS_C) f.mul(inputs + 3 * w, t, t);
      std::memcpy(out, t, 4 * w);
      return true;
    }
    std::vector<uint32_t> v((size_t)p.nof_vars() * w, 0);
    std::memcpy(v.data(), inputs, (size_t)4 * w * p.nof_inputs());
    for (int k = 0; k < p.nof_constants; k++)
      std::memcpy(&v[(size_t)(p.nof_parameters + k) * w], p.constants[k].data(), 4 * w);
    for (const ProgInstr& i : p.ins) {
      if (i.a >= p.nof_vars() || i.b >= p.nof_vars() || i.dst >= p.nof_vars()) return false;
      const uint32_t *a = &v[(size_t)i.a * w], *b = &v[(size_t)i.b * w];
      uint32_t* d = &v[(size_t)i.dst * w];
      switch (i.op) {
      case PROG_COPY: std::memmove(d, a, 4 * w); break;
      case PROG_ADD: f.add(a, b, d); break;
      case PROG_SUB: f.sub(a, b, d); break;
      case PROG_MUL: f.mul(a, b, d); break;
      default: return false;
      }
    }
    std::memcpy(out, &v[(size_t)p.nof_inputs() * w], 4 * w);
    return true;
  }

  // ---- transcript bytes ----------------------------------------------------------------------------------------------------------
  struct SumcheckLabels {
    const uint8_t *domain_separator, *round_poly, *round_challenge;
    size_t domain_separator_len, round_poly_len, round_challenge_len;
  };

  // Every u32 little-endian, a field element its canonical bytes. entry0 = round_poly_label | u32(d + 1) | u32(0).
  class SumcheckTranscriptBytes
  {
  public:
    SumcheckTranscriptBytes(const SumcheckLabels& l, uint32_t nof_rounds, uint32_t degree, const uint8_t* claimed_sum, const uint8_t* seed, size_t element_bytes)
        : m_l(l), m_degree(degree), m_eb(element_bytes)
    {
      put(m_head, l.domain_separator, l.domain_separator_len);
      put_le32(m_head, nof_rounds); // the reference's argument is named mle_polynomial_size; prover and verifier pass the number of rounds
      put_le32(m_head, degree);
      put(m_head, claimed_sum, element_bytes);
      put(m_head, seed, element_bytes);
      put(m_head, l.round_challenge, l.round_challenge_len);
      put(m_entry0, l.round_poly, l.round_poly_len);
      put_le32(m_entry0, degree + 1);
      put_le32(m_entry0, 0);
    }
    const std::vector<uint8_t>& entry0() const { return m_entry0; }
    // round 0: domain_separator | u32(rounds) | u32(d) | claimed_sum | seed | round_challenge_label | R_0 | entry0 -- R_0 before entry0
    // round i: entry0 | alpha_i | round_challenge_label | round_poly_label | u32(d + 1) | u32(i) | R_i
    std::vector<uint8_t> round_input(uint32_t round, const uint8_t* prev_alpha, const uint8_t* round_poly) const
    {
      std::vector<uint8_t> v;
      if (round == 0) {
        v = m_head;
        put(v, round_poly, (m_degree + 1) * m_eb);
        put(v, m_entry0.data(), m_entry0.size());
        return v;
      }
      v = m_entry0;
      put(v, prev_alpha, m_eb);
      put(v, m_l.round_challenge, m_l.round_challenge_len);
      put(v, m_l.round_poly, m_l.round_poly_len);
      put_le32(v, m_degree + 1);
      put_le32(v, round);
      put(v, round_poly, (m_degree + 1) * m_eb);
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
    SumcheckLabels m_l;
    uint32_t m_degree;
    size_t m_eb;
    std::vector<uint8_t> m_head, m_entry0;
  };

  // ---- the verifier ----------------------------------------------------------------------------------------------------------------
  // The polynomial through (i, evals[i]), i < count <= 7, at x: sum_i evals[i] prod_{j != i} (x - j) / (i - j). The denominators are
  // inverted together (one inversion).
  inline void sumcheck_lagrange_eval(const HostField& f, const uint32_t* evals, int count, const uint32_t* x, uint32_t* out)
  {
    const int w = f.words;
    uint32_t num[7][8], den[7][8], pre[7][8], t[8], u[8], acc[8];
    for (int i = 0; i < count; i++) {
      std::memcpy(num[i], evals + (size_t)i * w, 4 * w);
      f.from_u32(1, den[i]);
      for (int j = 0; j < count; j++) {
        if (j == i) continue;
        f.from_u32((uint32_t)j, t);
        f.sub(x, t, u);
        f.mul(num[i], u, num[i]);
        f.from_u32((uint32_t)i, u);
        f.sub(u, t, u);
        f.mul(den[i], u, den[i]);
      }
    }
    f.from_u32(1, acc);
    for (int i = 0; i < count; i++) { // pre[i] = den[0] .. den[i - 1]
      std::memcpy(pre[i], acc, 4 * w);
      f.mul(acc, den[i], acc);
    }
    f.inv(acc, acc);
    uint32_t result[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = count; i-- > 0;) { // acc = 1 / (den[0] .. den[i])
      f.mul(acc, pre[i], t);        // 1 / den[i]
      f.mul(acc, den[i], acc);
      f.mul(num[i], t, t);
      f.add(result, t, result);
    }
    std::memcpy(out, result, 4 * w);
  }

  // hash(message, digest) -> false on failure
  using SumcheckHashFn = std::function<bool(const std::vector<uint8_t>&, std::vector<uint8_t>*)>;

  // 0 = ran (*valid says how it ended), 1 = the hash failed. polys: `rounds` round polynomials of `size` elements back to back.
  // R_0[0] + R_0[1] = claimed_sum; for r < rounds - 1, alpha = F(H(msg_r)) and R_r(alpha) = R_{r+1}[0] + R_{r+1}[1]; the last round
  // polynomial is not checked against anything. A shape no prover makes (no rounds, fewer than 2 or more than 7 evaluations, a word at
  // or above p) is a wrong proof, not an error.
  inline int sumcheck_verify_host(const HostField& f, const uint32_t* polys, uint64_t rounds, uint64_t size, const uint32_t* claimed_sum, const uint32_t* seed,
                                  const SumcheckLabels& labels, const SumcheckHashFn& hash, bool* valid)
  {
    *valid = false;
    const int w = f.words;
    if (rounds == 0 || rounds > 63 || size < 2 || size > (uint64_t)PROG_MAX_DEGREE + 1) return 0;
    for (uint64_t i = 0; i < rounds * size; i++)
      if (!f.is_canonical(polys + i * w)) return 0;
    uint32_t t[8], alpha[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    f.add(polys, polys + w, t);
    if (!f.eq(t, claimed_sum)) return 0;
    const SumcheckTranscriptBytes transcript(labels, (uint32_t)rounds, (uint32_t)size - 1, reinterpret_cast<const uint8_t*>(claimed_sum),
                                             reinterpret_cast<const uint8_t*>(seed), 4 * (size_t)w);
    std::vector<uint8_t> digest;
    for (uint64_t r = 0; r + 1 < rounds; r++) {
      const uint32_t *cur = polys + r * size * w, *next = cur + size * w;
      if (!hash(transcript.round_input((uint32_t)r, reinterpret_cast<const uint8_t*>(alpha), reinterpret_cast<const uint8_t*>(cur)), &digest)) return 1;
      f.from_digest(digest.data(), digest.size(), alpha);
      sumcheck_lagrange_eval(f, cur, (int)size, alpha, t);
      uint32_t want[8];
      f.add(next, next + w, want);
      if (!f.eq(t, want)) return 0;
    }
    *valid = true;
    return 0;
  }

} // namespace icicle_hip
