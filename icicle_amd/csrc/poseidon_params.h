// Poseidon parameters over a 256-bit scalar field for a width t in {3, 5, 9, 12}, derived from the specification when a hasher is
// created. Host only, no HIP: the CPU tests compile it with g++ (tests/poseidon_host_harness.cpp). Nothing here is a table: every
// number below follows from p and t.
//
// Sources: Poseidon (USENIX Security 2021, eprint 2019/458: S-box x^5, Grain LFSR, Cauchy MDS matrix, the equivalent form of the
// partial rounds in its appendix B) and the Filecoin specification of the optimized schedule (the same factorisation, with names).
//   rounds       R_F = 8 (4 + 4), R_P = 56, 56, 57, 57 for t = 3, 5, 9, 12
//   M            M[i][j] = 1 / (i + j + t); the state is a row vector, new[j] = sum_i s[i] M[i][j]
//   constants    Grain: 80-bit state, seed = field 1 (2 bits) | sbox 1 (4) | n = bits of p (12) | t (12) | R_F (10) | R_P (10) | thirty 1s,
//                feedback s62 ^ s51 ^ s38 ^ s23 ^ s13 ^ s0, 160 bits discarded, then self-shrinking: of every pair of bits the
//                second is output when the first is 1. n bits MSB first make a value, values >= p are rejected. t (R_F + R_P)
//                values: t per round, c_r the vector of round r. n is the bit length of p, except for Grumpkin's scalar field
//                (BN254's base field, 254 bits), whose constants the reference generated with n = 255: its digests pin that.
// The textbook round is s <- sbox(s + c_r) M. The optimized schedule computes the same permutation as
//   s += c_0
//   3 x          s <- (sbox(s) + c_r M^-1) M                                                    r = 1, 2, 3
//                s <- (sbox(s) + a M^-1) P
//   R_P x        s_0 <- sbox(s_0) + k_i;  s <- s S_i                                            S_i sparse
//   3 x          s <- (sbox(s) + c_r M^-1) M                                                    r = 4 + R_P + 1, ..
//                s <- sbox(s) M
// where a constant added in front of an S-box is moved behind the preceding matrix (c M^-1), and in the partial rounds only its
// first entry stays (k_i) while the rest travels back round by round into a. The matrices come from M = M' M'' with
// M' = [[1, 0], [0, M^]] (M^ the lower right block) and M'' = [[M_00, v], [w^, I]], w^ = M^^-1 w (w the first column, v the first
// row, both without M_00): M'' is sparse, M' commutes with the partial S-box and is multiplied into the matrix of the round in
// front. Walking back from the last partial round gives S_(R_P - 1), .., S_0 and at last P. S_i is stored as its first column
// (M_00, w^) followed by v: new_0 = sum_i s_i col_i, new_j = s_0 v_j + s_j.
// tests/test_poseidon_cpu.py holds the same derivation written independently in Python integers; tests/poseidon_model.py the
// textbook permutation; tests/golden/poseidon_vectors.json digests of the reference, which prove all three.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>
#include "bigfield.hpp"

namespace icicle_hip {
  namespace poseidon {

    constexpr int FULL_ROUNDS = 8;
    inline int partial_rounds(unsigned t) { return t == 3 || t == 5 ? 56 : t == 9 || t == 12 ? 57 : 0; }
    inline bool width_supported(unsigned t) { return partial_rounds(t) != 0; }
    // the field size that seeds the LFSR and the number of bits it draws per constant
    template <class PR>
    constexpr int grain_bits()
    {
      return std::is_same<PR, bn254_fq_params>::value ? 255 : PR::NBITS;
    }

    // the bit stream behind the round constants
    class Grain
    {
    public:
      Grain(int n, int t, int r_f, int r_p)
      {
        int at = 0;
        auto put = [&](uint32_t v, int bits) {
          for (int b = bits - 1; b >= 0; b--)
            m_s[at++] = (v >> b) & 1;
        };
        put(1, 2), put(1, 4), put((uint32_t)n, 12), put((uint32_t)t, 12), put((uint32_t)r_f, 10), put((uint32_t)r_p, 10);
        while (at < 80)
          m_s[at++] = 1;
        for (int i = 0; i < 160; i++)
          step();
      }
      uint32_t bit()
      {
        while (!step())
          step();
        return step();
      }

    private:
      uint8_t m_s[80];
      int m_head = 0; // s_i is m_s[(m_head + i) % 80]
      uint8_t at(int i) const { return m_s[(m_head + i) % 80]; }
      uint8_t step()
      {
        const uint8_t b = at(62) ^ at(51) ^ at(38) ^ at(23) ^ at(13) ^ at(0);
        m_s[m_head] = b; // s_0 leaves, the new bit becomes s_79
        m_head = (m_head + 1) % 80;
        return b;
      }
    };

    // F_p on the host through bigfield.hpp: Montgomery form, every result reduced to [0, p)
    template <class PR>
    struct HostField {
      using F = FieldOps<PR>;
      using fe = Fe<PR>;
      static fe mul(const fe& a, const fe& b) { return F::reduce(F::mul(a, b)); }
      static fe add(const fe& a, const fe& b) { return F::reduce(F::add(a, b)); }
      static fe sub(const fe& a, const fe& b) { return F::reduce(F::template sub<1>(a, b)); }
      static fe inv(const fe& a) { return F::reduce(F::inv(a)); }
      static bool is_zero(const fe& a) { return F::is_zero_limbs(a); }
      static fe from_small(uint32_t v)
      {
        uint32_t w[PR::NL32] = {v};
        return F::reduce(F::from_canonical(w));
      }
      // canonical words, little-endian; false when >= p
      static bool below_p(const uint32_t* w)
      {
        for (int i = PR::NL32 - 1; i >= 0; i--)
          if (w[i] != PR::P32[i]) return w[i] < PR::P32[i];
        return false;
      }
    };

    template <class PR>
    using Vec = std::vector<Fe<PR>>; // a vector of t, or a t x t matrix row-major

    template <class PR>
    Vec<PR> mat_mul(const Vec<PR>& a, const Vec<PR>& b, size_t n)
    {
      using H = HostField<PR>;
      Vec<PR> c(n * n, FieldOps<PR>::zero());
      for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++)
          for (size_t k = 0; k < n; k++)
            c[i * n + j] = H::add(c[i * n + j], H::mul(a[i * n + k], b[k * n + j]));
      return c;
    }
    // v A for a row vector v
    template <class PR>
    Vec<PR> row_times(const Vec<PR>& v, const Vec<PR>& a, size_t n)
    {
      using H = HostField<PR>;
      Vec<PR> r(n, FieldOps<PR>::zero());
      for (size_t j = 0; j < n; j++)
        for (size_t i = 0; i < n; i++)
          r[j] = H::add(r[j], H::mul(v[i], a[i * n + j]));
      return r;
    }
    // Gauss-Jordan; false for a singular matrix (none of the matrices here is)
    template <class PR>
    bool mat_inv(const Vec<PR>& a, size_t n, Vec<PR>* out)
    {
      using H = HostField<PR>;
      using F = FieldOps<PR>;
      const size_t w = 2 * n;
      Vec<PR> m(n * w, F::zero());
      for (size_t i = 0; i < n; i++) {
        for (size_t j = 0; j < n; j++)
          m[i * w + j] = a[i * n + j];
        m[i * w + n + i] = F::reduce(F::one());
      }
      for (size_t c = 0; c < n; c++) {
        size_t piv = c;
        while (piv < n && H::is_zero(m[piv * w + c]))
          piv++;
        if (piv == n) return false;
        for (size_t j = 0; j < w; j++)
          std::swap(m[piv * w + j], m[c * w + j]);
        const Fe<PR> iv = H::inv(m[c * w + c]);
        for (size_t j = 0; j < w; j++)
          m[c * w + j] = H::mul(m[c * w + j], iv);
        for (size_t r = 0; r < n; r++) {
          if (r == c || H::is_zero(m[r * w + c])) continue;
          const Fe<PR> f = m[r * w + c];
          for (size_t j = 0; j < w; j++)
            m[r * w + j] = H::sub(m[r * w + j], H::mul(f, m[c * w + j]));
        }
      }
      out->assign(n * n, F::zero());
      for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++)
          (*out)[i * n + j] = m[i * w + n + j];
      return true;
    }

    // Everything in Montgomery form, reduced to [0, p).
    template <class PR>
    struct Params {
      int t = 0, r_f = 0, r_p = 0;
      Vec<PR> grain;  // t (r_f + r_p): the round constants as the LFSR gives them
      Vec<PR> mds;    // t x t, row-major
      Vec<PR> rc;     // t r_f + r_p: c_0 | 3 x c M^-1 | a M^-1 | k_0 .. k_(r_p - 1) | 3 x c M^-1
      Vec<PR> pre;    // t x t, row-major: P
      Vec<PR> sparse; // r_p x (2 t - 1): S_0 .. S_(r_p - 1)
    };

    template <class PR>
    Params<PR> derive(int t)
    {
      using H = HostField<PR>;
      using F = FieldOps<PR>;
      using fe = Fe<PR>;
      const size_t T = (size_t)t;
      Params<PR> P;
      P.t = t, P.r_f = FULL_ROUNDS, P.r_p = partial_rounds((unsigned)t);
      const int half = P.r_f / 2, rounds = P.r_f + P.r_p;

      constexpr int NB = grain_bits<PR>();
      static_assert(NB <= 32 * PR::NL32, "a constant fits the words");
      Grain g(NB, t, P.r_f, P.r_p);
      while (P.grain.size() < T * rounds) {
        uint32_t w[PR::NL32] = {0};
        for (int b = NB - 1; b >= 0; b--)
          w[b / 32] |= g.bit() << (b % 32);
        if (H::below_p(w)) P.grain.push_back(F::reduce(F::from_canonical(w)));
      }
      auto round_key = [&](int r) { return Vec<PR>(P.grain.begin() + T * r, P.grain.begin() + T * (r + 1)); };

      P.mds.resize(T * T);
      for (size_t i = 0; i < T; i++)
        for (size_t j = 0; j < T; j++)
          P.mds[i * T + j] = H::inv(H::from_small((uint32_t)(i + j + T)));
      Vec<PR> mds_inv;
      mat_inv<PR>(P.mds, T, &mds_inv);

      auto append = [&](const Vec<PR>& v) { P.rc.insert(P.rc.end(), v.begin(), v.end()); };
      append(round_key(0));
      for (int r = 1; r < half; r++)
        append(row_times<PR>(round_key(r), mds_inv, T));
      // back through the partial rounds: what cannot stay in front of the partial S-box moves one round up
      Vec<PR> acc = round_key(half + P.r_p);
      std::vector<fe> partial((size_t)P.r_p);
      for (int i = 0; i < P.r_p; i++) {
        Vec<PR> moved = row_times<PR>(acc, mds_inv, T);
        partial[(size_t)(P.r_p - 1 - i)] = moved[0];
        moved[0] = F::zero();
        const Vec<PR> prev = round_key(half + P.r_p - 1 - i);
        for (size_t j = 0; j < T; j++)
          acc[j] = H::add(prev[j], moved[j]);
      }
      append(row_times<PR>(acc, mds_inv, T));
      append(partial);
      for (int r = 1; r < half; r++)
        append(row_times<PR>(round_key(half + P.r_p + r), mds_inv, T));

      // M = M' M'', from the last partial round to the first
      Vec<PR> m = P.mds;
      std::vector<Vec<PR>> sparse_rev;
      for (int i = 0; i < P.r_p; i++) {
        const size_t S = T - 1;
        Vec<PR> hat(S * S), hat_inv;
        for (size_t a = 0; a < S; a++)
          for (size_t b = 0; b < S; b++)
            hat[a * S + b] = m[(a + 1) * T + b + 1];
        mat_inv<PR>(hat, S, &hat_inv);
        Vec<PR> s;
        s.push_back(m[0]);
        for (size_t a = 0; a < S; a++) { // w^ = M^^-1 w
          fe x = F::zero();
          for (size_t b = 0; b < S; b++)
            x = H::add(x, H::mul(hat_inv[a * S + b], m[(b + 1) * T]));
          s.push_back(x);
        }
        for (size_t b = 1; b < T; b++)
          s.push_back(m[b]);
        sparse_rev.push_back(s);
        Vec<PR> prime(T * T, F::zero());
        prime[0] = F::reduce(F::one());
        for (size_t a = 0; a < S; a++)
          for (size_t b = 0; b < S; b++)
            prime[(a + 1) * T + b + 1] = hat[a * S + b];
        m = mat_mul<PR>(P.mds, prime, T);
      }
      P.pre = m;
      for (int i = P.r_p - 1; i >= 0; i--)
        P.sparse.insert(P.sparse.end(), sparse_rev[(size_t)i].begin(), sparse_rev[(size_t)i].end());
      return P;
    }

    // canonical words of a reduced Montgomery element
    template <class PR>
    void to_words(const Fe<PR>& a, uint32_t* w)
    {
      FieldOps<PR>::to_canonical(w, a);
    }

    // the parameters of (PR, t), derived once per process; nullptr for a width outside the four
    template <class PR>
    std::shared_ptr<const Params<PR>> params(unsigned t)
    {
      if (!width_supported(t)) return nullptr;
      static std::mutex mtx;
      static std::map<unsigned, std::shared_ptr<const Params<PR>>> cache;
      std::lock_guard<std::mutex> lk(mtx);
      auto& slot = cache[t];
      if (!slot) slot = std::make_shared<const Params<PR>>(derive<PR>((int)t));
      return slot;
    }

  } // namespace poseidon
} // namespace icicle_hip
