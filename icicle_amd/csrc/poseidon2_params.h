// Poseidon2 parameters for a 31-bit prime p and a width t in {2, 3, 4, 8, 12, 16, 20, 24}, derived from the specification when a
// hasher is created. Host only, no HIP: the CPU tests compile it with g++ (tests/poseidon2_host_harness.cpp). Nothing here is a
// table: every number below follows from p, t and the security level.
//
// Sources: Poseidon (USENIX Security 2021, eprint 2019/458: S-box exponent, round numbers, Grain LFSR), Poseidon2 (eprint 2023/323:
// the two matrices and the condition on the partial-round matrix), eprint 2023/537 (the binomial bound on the round numbers).
//   alpha        smallest a >= 3 with gcd(a, p - 1) = 1 (7 for BabyBear, 3 for KoalaBear)
//   R_F, R_P     the cheapest pair -- t R_F + R_P S-boxes, ties to the smaller R_F -- among R_P in 1 .. 499, even R_F in 4 .. 98 that
//                meets the statistical, interpolation, Groebner (three forms) and binomial bounds at M = 128 bits; then the margin
//                R_F += 2, R_P = ceil(1.075 R_P)
//   constants    Grain: 80-bit state, seed = field 1 (2 bits) | sbox 0 (4) | n = bits of p (12) | t (12) | R_F (10) | R_P (10) | thirty 1s,
//                feedback s62 ^ s51 ^ s38 ^ s23 ^ s13 ^ s0, 160 bits discarded, then self-shrinking: of every pair of bits the
//                second is output when the first is 1. n bits MSB first make a value, values >= p are rejected. R_F t + R_P values
//                in round order: t per full round, one per partial round.
//   M_I          ones off the diagonal; the diagonal is (2, 3), (2, 2, 3), or t values from the same stream behind the constants,
//                each reduced mod p (no rejection), all t redrawn until the characteristic polynomial of M_I^i is irreducible of
//                degree t for i = 1 .. 2t. poseidon2.hpp applies it as s + (d_i - 1) x_i with s the sum of the state.
//   M_E          circ(2, 1), circ(2, 1, 1), M4, or blocks of M4 with 2 M4 on the diagonal: never stored, poseidon2.hpp applies it by
//                M4's addition chain.
// The characteristic polynomial of A is found as the minimal polynomial of the vector e_0: if e_0, A e_0, .., A^(t-1) e_0 are
// dependent that polynomial has a degree below t and divides the characteristic one, which then is reducible; otherwise the two are
// equal. Irreducibility is Rabin's test: x^(p^t) = x mod f and gcd(x^(p^(t/q)) - x, f) = 1 for every prime q | t, the powers of the
// Frobenius map taken with its matrix on the basis 1, x, .., x^(t-1).
// tests/poseidon2_model.py holds the same derivation written independently; tests/golden/poseidon2_vectors.json holds digests of
// the reference, which prove both.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

namespace icicle_hip {
  namespace poseidon2 {

    constexpr int SECURITY_BITS = 128;

    struct Params {
      uint32_t p = 0;
      int t = 0, alpha = 0, r_f = 0, r_p = 0;
      std::vector<uint32_t> rc;   // r_f t + r_p canonical residues, round order
      std::vector<uint32_t> diag; // t canonical residues: the diagonal of M_I
    };

    inline bool width_supported(unsigned t) { return t == 2 || t == 3 || t == 4 || (t % 4 == 0 && t >= 8 && t <= 24); }

    // ---- round numbers --------------------------------------------------------------------------------------------------------------
    inline uint64_t gcd_u64(uint64_t a, uint64_t b)
    {
      while (b) {
        const uint64_t r = a % b;
        a = b, b = r;
      }
      return a;
    }
    inline int alpha_of(uint32_t p)
    {
      int a = 3;
      while (gcd_u64((uint64_t)a, (uint64_t)p - 1) != 1)
        a++;
      return a;
    }
    inline int bit_length(uint32_t p)
    {
      int n = 0;
      while (p >> n)
        n++;
      return n;
    }
    // binom(n, k)^2 > 2^(M - 1), i.e. ceil(2 log2 binom(n, k)) >= M, exactly: the running binomials binom(n - k + i, i) only grow, so
    // the product may stop at the first one that reaches 2^64
    inline bool binomial_squared_exceeds(uint64_t n, uint64_t k, int m_minus_1)
    {
      if (k > n) return false;
      if (k > n - k) k = n - k;
      unsigned __int128 c = 1;
      for (uint64_t i = 1; i <= k; i++) {
        c = c * (n - k + i) / i; // c < 2^64 and n < 2^32 before the product
        if (c >> 64) return true; // c^2 >= 2^128
      }
      return c * c > ((unsigned __int128)1 << m_minus_1);
    }
    // p enters only as n, its bit length, and lg = log2 p: poseidon2_wide_params.h calls this for the 256-bit primes
    inline bool rounds_suffice(int n, double lg, int t, int alpha, int r_f, int r_p)
    {
      const int M = SECURITY_BITS;
      const double log_a_2 = std::log(2.0) / std::log((double)alpha);
      int ceil_log_a_t = 0; // smallest k with alpha^k >= t
      for (int v = 1; v < t; v *= alpha)
        ceil_log_a_t++;
      // statistical attacks: 6 full rounds while (floor(log2 p - C))(t + 1) >= M, else 10; C = (alpha - 1) / 2 as the parameter script
      // of the Poseidon2 authors has it, with which the published instances were generated
      int need = M <= (int)std::floor(lg - (alpha - 1) / 2.0) * (t + 1) ? 6 : 10;
      // interpolation attack
      need = std::max(need, 1 + (int)std::ceil(log_a_2 * std::min(M, n)) + ceil_log_a_t - r_p);
      // Groebner basis attacks
      need = std::max(need, (int)std::ceil(log_a_2 * std::min((double)M, lg) - r_p));
      need = std::max(need, (int)std::ceil(t - 1 + log_a_2 * std::min(M / (double)(t + 1), lg / 2) - r_p));
      need = std::max(need, (int)std::ceil((t - 2 + M / (2 * std::log2((double)alpha)) - r_p) / (double)(t - 1)));
      if (r_f < need) return false;
      // eprint 2023/537: r_f is even, so every argument is an integer
      const uint64_t r = (uint64_t)t / 3, under = r * (r_f / 2) + r_p + alpha, over = (uint64_t)(r_f - 1) * t + r_p + r + under;
      return binomial_squared_exceeds(over, under, M - 1);
    }
    inline void round_numbers(int n, double lg, int t, int alpha, int* r_f_out, int* r_p_out)
    {
      long best_cost = -1;
      int best_f = 0, best_p = 0;
      for (int r_p = 1; r_p < 500; r_p++)
        for (int r_f = 4; r_f < 100; r_f += 2) {
          if (!rounds_suffice(n, lg, t, alpha, r_f, r_p)) continue;
          const int f = r_f + 2, q = (int)std::ceil(1.075 * r_p);
          const long cost = (long)t * f + q;
          if (best_cost < 0 || cost < best_cost || (cost == best_cost && f < best_f)) best_cost = cost, best_f = f, best_p = q;
          break; // more full rounds beside the same partial rounds only cost more
        }
      *r_f_out = best_f, *r_p_out = best_p;
    }
    inline void round_numbers(uint32_t p, int t, int alpha, int* r_f_out, int* r_p_out)
    {
      round_numbers(bit_length(p), std::log2((double)p), t, alpha, r_f_out, r_p_out);
    }

    // ---- Grain ------------------------------------------------------------------------------------------------------------------------
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
        put(1, 2), put(0, 4), put((uint32_t)n, 12), put((uint32_t)t, 12), put((uint32_t)r_f, 10), put((uint32_t)r_p, 10);
        while (at < 80)
          m_s[at++] = 1;
        for (int i = 0; i < 160; i++)
          step();
      }
      uint32_t bits(int n)
      {
        uint32_t v = 0;
        for (int i = 0; i < n; i++)
          v = v << 1 | bit();
        return v;
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
      uint32_t bit()
      {
        while (!step())
          step();
        return step();
      }
    };

    // ---- F_p, polynomials (coefficients low first) and matrices (row-major) -------------------------------------------------------------------
    inline uint32_t mulmod(uint32_t a, uint32_t b, uint32_t p) { return (uint32_t)((uint64_t)a * b % p); }
    inline uint32_t submod(uint32_t a, uint32_t b, uint32_t p) { return a >= b ? a - b : a + p - b; }
    inline uint32_t powmod(uint32_t a, uint64_t e, uint32_t p)
    {
      uint32_t r = 1;
      for (; e; e >>= 1, a = mulmod(a, a, p))
        if (e & 1) r = mulmod(r, a, p);
      return r;
    }
    inline uint32_t invmod(uint32_t a, uint32_t p) { return powmod(a, (uint64_t)p - 2, p); }
    using Poly = std::vector<uint32_t>;

    // a b mod f, f monic of degree t, a and b of degree < t
    inline Poly poly_mulmod(const Poly& a, const Poly& b, const Poly& f, uint32_t p)
    {
      const size_t t = f.size() - 1;
      std::vector<uint64_t> acc(2 * t - 1, 0);
      for (size_t i = 0; i < t; i++)
        for (size_t j = 0; j < t; j++)
          acc[i + j] += (uint64_t)a[i] * b[j] % p; // at most t terms below 2^31 each
      Poly c(2 * t - 1);
      for (size_t i = 0; i < c.size(); i++)
        c[i] = (uint32_t)(acc[i] % p);
      for (size_t k = 2 * t - 2; k >= t; k--) { // x^k = -(f_0 + .. + f_(t-1) x^(t-1)) x^(k-t)
        const uint32_t top = c[k];
        if (top)
          for (size_t i = 0; i < t; i++)
            c[k - t + i] = submod(c[k - t + i], mulmod(top, f[i], p), p);
      }
      c.resize(t);
      return c;
    }
    inline void poly_trim(Poly& a)
    {
      while (!a.empty() && a.back() == 0)
        a.pop_back();
    }
    inline Poly poly_rem(Poly a, const Poly& b, uint32_t p) // b trimmed, not zero
    {
      const uint32_t inv = invmod(b.back(), p);
      while (a.size() >= b.size()) {
        const uint32_t q = mulmod(a.back(), inv, p);
        const size_t off = a.size() - b.size();
        if (q)
          for (size_t i = 0; i < b.size(); i++)
            a[off + i] = submod(a[off + i], mulmod(q, b[i], p), p);
        a.pop_back();
      }
      poly_trim(a);
      return a;
    }
    inline bool poly_coprime(Poly a, Poly b, uint32_t p)
    {
      poly_trim(a), poly_trim(b);
      while (!b.empty()) {
        Poly r = poly_rem(a, b, p);
        a = std::move(b), b = std::move(r);
      }
      return a.size() == 1;
    }
    // Rabin's test for a monic f of degree t >= 2
    inline bool is_irreducible(const Poly& f, uint32_t p)
    {
      const size_t t = f.size() - 1;
      Poly x(t, 0), h(t, 0);
      x[1] = 1;
      // h = x^p mod f
      h[0] = 1;
      for (int b = 31; b >= 0; b--) {
        h = poly_mulmod(h, h, f, p);
        if (p >> b & 1) h = poly_mulmod(h, x, f, p);
      }
      // the Frobenius map g -> g^p is linear: row i of its matrix is x^(i p) = h^i
      std::vector<Poly> frob(t);
      frob[0].assign(t, 0), frob[0][0] = 1;
      for (size_t i = 1; i < t; i++)
        frob[i] = poly_mulmod(frob[i - 1], h, f, p);
      Poly cur = x; // x^(p^k)
      for (size_t k = 1; k <= t; k++) {
        std::vector<uint64_t> acc(t, 0);
        for (size_t i = 0; i < t; i++)
          if (cur[i])
            for (size_t j = 0; j < t; j++)
              acc[j] += (uint64_t)cur[i] * frob[i][j] % p;
        for (size_t j = 0; j < t; j++)
          cur[j] = (uint32_t)(acc[j] % p);
        bool wanted = false; // k = t / q for a prime q | t
        if (k < t && t % k == 0) {
          const size_t q = t / k;
          wanted = true;
          for (size_t d = 2; d * d <= q; d++)
            if (q % d == 0) wanted = false;
        }
        if (wanted) {
          Poly diff(t);
          for (size_t j = 0; j < t; j++)
            diff[j] = submod(cur[j], x[j], p);
          Poly g = diff;
          poly_trim(g);
          if (g.empty() || !poly_coprime(f, diff, p)) return false;
        }
      }
      return cur == x;
    }

    using Matrix = std::vector<uint32_t>; // t x t
    inline Matrix mat_mul(const Matrix& a, const Matrix& b, size_t t, uint32_t p)
    {
      Matrix c(t * t);
      for (size_t i = 0; i < t; i++)
        for (size_t j = 0; j < t; j++) {
          uint64_t s = 0;
          for (size_t k = 0; k < t; k++)
            s += (uint64_t)a[i * t + k] * b[k * t + j] % p;
          c[i * t + j] = (uint32_t)(s % p);
        }
      return c;
    }
    // the characteristic polynomial of a, if it can be irreducible: false when e_0, a e_0, .., a^(t-1) e_0 are dependent
    inline bool char_poly_if_cyclic(const Matrix& a, size_t t, uint32_t p, Poly* f)
    {
      // columns k < t: a^k e_0; column t: a^t e_0. Solve K c = a^t e_0.
      std::vector<Poly> rows(t, Poly(t + 1, 0));
      Poly v(t, 0), w(t);
      v[0] = 1;
      for (size_t k = 0; k <= t; k++) {
        for (size_t i = 0; i < t; i++)
          rows[i][k] = v[i];
        for (size_t i = 0; i < t; i++) {
          uint64_t s = 0;
          for (size_t j = 0; j < t; j++)
            s += (uint64_t)a[i * t + j] * v[j] % p;
          w[i] = (uint32_t)(s % p);
        }
        v = w;
      }
      for (size_t col = 0; col < t; col++) {
        size_t piv = col;
        while (piv < t && rows[piv][col] == 0)
          piv++;
        if (piv == t) return false;
        std::swap(rows[piv], rows[col]);
        const uint32_t inv = invmod(rows[col][col], p);
        for (size_t j = col; j <= t; j++)
          rows[col][j] = mulmod(rows[col][j], inv, p);
        for (size_t i = 0; i < t; i++) {
          const uint32_t m = rows[i][col];
          if (i == col || m == 0) continue;
          for (size_t j = col; j <= t; j++)
            rows[i][j] = submod(rows[i][j], mulmod(m, rows[col][j], p), p);
        }
      }
      f->assign(t + 1, 0); // x^t - sum c_k x^k
      for (size_t k = 0; k < t; k++)
        (*f)[k] = submod(0, rows[k][t], p);
      (*f)[t] = 1;
      return true;
    }
    inline bool diagonal_is_good(const std::vector<uint32_t>& diag, uint32_t p)
    {
      const size_t t = diag.size();
      Matrix m(t * t, 1);
      for (size_t i = 0; i < t; i++)
        m[i * t + i] = diag[i];
      Matrix cur = m;
      Poly f;
      for (size_t i = 1; i <= 2 * t; i++) {
        if (!char_poly_if_cyclic(cur, t, p, &f) || !is_irreducible(f, p)) return false;
        if (i < 2 * t) cur = mat_mul(m, cur, t, p);
      }
      return true;
    }

    inline Params derive(uint32_t p, int t)
    {
      Params P;
      P.p = p, P.t = t, P.alpha = alpha_of(p);
      round_numbers(p, t, P.alpha, &P.r_f, &P.r_p);
      const int n = bit_length(p);
      Grain g(n, t, P.r_f, P.r_p);
      const size_t count = (size_t)P.r_f * t + P.r_p;
      while (P.rc.size() < count) {
        const uint32_t v = g.bits(n);
        if (v < p) P.rc.push_back(v);
      }
      if (t == 2) {
        P.diag = {2, 3};
      } else if (t == 3) {
        P.diag = {2, 2, 3};
      } else {
        P.diag.resize(t);
        do {
          for (int i = 0; i < t; i++)
            P.diag[i] = g.bits(n) % p;
        } while (!diagonal_is_good(P.diag, p));
      }
      return P;
    }

    // the parameters of (p, t), derived once per process; nullptr for a width outside the eight
    inline std::shared_ptr<const Params> params(uint32_t p, unsigned t)
    {
      if (!width_supported(t) || bit_length(p) != 31) return nullptr;
      static std::mutex mtx;
      static std::map<std::pair<uint32_t, unsigned>, std::shared_ptr<const Params>> cache;
      std::lock_guard<std::mutex> lk(mtx);
      auto& slot = cache[{p, t}];
      if (!slot) slot = std::make_shared<const Params>(derive(p, (int)t));
      return slot;
    }

  } // namespace poseidon2
} // namespace icicle_hip
