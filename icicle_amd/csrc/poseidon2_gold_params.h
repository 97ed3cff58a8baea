// Poseidon2 parameters over Goldilocks, p = 2^64 - 2^32 + 1, for a width t in {2, 3, 4, 8, 12, 16, 20, 24}, derived from the
// specification when the first hasher of a width is created. Host only, no HIP: the CPU tests compile it with g++
// (tests/poseidon2_gold_host_harness.cpp). Nothing here is a table: every number below follows from p, t and the security level.
//
// The derivation is that of poseidon2_params.h, which states it and its sources. What depends on p only through its bit length,
// log2 p and alpha -- the round-number search and the Grain LFSR -- is that header's code, called from here with n = 64. What
// computes in F_p -- the rejection sampling of 64-bit values, the diagonal of M_I and the irreducibility test of the
// characteristic polynomials of M_I^i -- is written here over canonical uint64_t values, every product an unsigned __int128 reduced
// by the shape of p (FieldOps<goldilocks_params>::mul of goldfield.hpp, host side).
//   alpha        7: p - 1 = 2^32 * 3 * 5 * 17 * 257 * 65537
//   R_F, R_P     (8, 27), (8, 23), (8, 21) for t = 2, 3, 4 and (8, 22) for t = 8 .. 24
//   constants    Grain seeded with n = 64: 64 bits MSB first per value (two draws of 32), values >= p rejected
//   M_I          diagonal (2, 3), (2, 2, 3), or t draws of 64 bits reduced mod p (one subtraction: 2^64 < 2 p), all t redrawn until
//                the characteristic polynomial of M_I^i is irreducible of degree t for i = 1 .. 2t
// tests/poseidon2_model_gold.py holds the same derivation written independently in Python integers;
// tests/golden/poseidon2_vectors_gold.json holds digests of the reference, which prove both.
#pragma once
#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>
#include "goldfield.hpp"
#include "poseidon2_params.h"

namespace icicle_hip {
  namespace poseidon2_gold {

    constexpr uint64_t P = goldilocks_params::P;

    inline bool width_supported(unsigned t) { return poseidon2::width_supported(t); }

    // ---- F_p on canonical values -----------------------------------------------------------------------------------------------------
    inline uint64_t addmod(uint64_t a, uint64_t b) { return FieldOps<goldilocks_params>::add({a}, {b}).v; }
    inline uint64_t submod(uint64_t a, uint64_t b) { return FieldOps<goldilocks_params>::sub<1>({a}, {b}).v; }
    inline uint64_t mulmod(uint64_t a, uint64_t b) { return FieldOps<goldilocks_params>::mul({a}, {b}).v; }
    inline uint64_t invmod(uint64_t a) { return FieldOps<goldilocks_params>::inv({a}).v; }

    // 64 bits of the stream, MSB first
    inline uint64_t draw(poseidon2::Grain& g)
    {
      const uint64_t hi = g.bits(32);
      return hi << 32 | g.bits(32);
    }

    // ---- polynomials over F_p (coefficients low first) and matrices (row-major) ----------------------------------------------------------
    using Poly = std::vector<uint64_t>;

    // a b mod f, f monic of degree t, a and b of degree < t
    inline Poly poly_mulmod(const Poly& a, const Poly& b, const Poly& f)
    {
      const size_t t = f.size() - 1;
      Poly c(2 * t - 1, 0);
      for (size_t i = 0; i < t; i++)
        if (a[i])
          for (size_t j = 0; j < t; j++)
            c[i + j] = addmod(c[i + j], mulmod(a[i], b[j]));
      for (size_t k = 2 * t - 2; k >= t; k--) { // x^k = -(f_0 + .. + f_(t-1) x^(t-1)) x^(k-t)
        const uint64_t top = c[k];
        if (top)
          for (size_t i = 0; i < t; i++)
            c[k - t + i] = submod(c[k - t + i], mulmod(top, f[i]));
      }
      c.resize(t);
      return c;
    }
    inline void poly_trim(Poly& a)
    {
      while (!a.empty() && a.back() == 0)
        a.pop_back();
    }
    inline Poly poly_rem(Poly a, const Poly& b) // b trimmed, not zero
    {
      const uint64_t inv = invmod(b.back());
      while (a.size() >= b.size()) {
        const uint64_t q = mulmod(a.back(), inv);
        const size_t off = a.size() - b.size();
        if (q)
          for (size_t i = 0; i < b.size(); i++)
            a[off + i] = submod(a[off + i], mulmod(q, b[i]));
        a.pop_back();
      }
      poly_trim(a);
      return a;
    }
    inline bool poly_coprime(Poly a, Poly b)
    {
      poly_trim(a), poly_trim(b);
      while (!b.empty()) {
        Poly r = poly_rem(a, b);
        a = std::move(b), b = std::move(r);
      }
      return a.size() == 1;
    }
    // Rabin's test for a monic f of degree t >= 2
    inline bool is_irreducible(const Poly& f)
    {
      const size_t t = f.size() - 1;
      Poly x(t, 0), h(t, 0);
      x[1] = 1;
      // h = x^p mod f
      h[0] = 1;
      for (int b = 63; b >= 0; b--) {
        h = poly_mulmod(h, h, f);
        if (P >> b & 1) h = poly_mulmod(h, x, f);
      }
      // the Frobenius map g -> g^p is linear: row i of its matrix is x^(i p) = h^i
      std::vector<Poly> frob(t);
      frob[0].assign(t, 0), frob[0][0] = 1;
      for (size_t i = 1; i < t; i++)
        frob[i] = poly_mulmod(frob[i - 1], h, f);
      Poly cur = x; // x^(p^k)
      for (size_t k = 1; k <= t; k++) {
        Poly next(t, 0);
        for (size_t i = 0; i < t; i++)
          if (cur[i])
            for (size_t j = 0; j < t; j++)
              next[j] = addmod(next[j], mulmod(cur[i], frob[i][j]));
        cur = next;
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
            diff[j] = submod(cur[j], x[j]);
          Poly g = diff;
          poly_trim(g);
          if (g.empty() || !poly_coprime(f, diff)) return false;
        }
      }
      return cur == x;
    }

    using Matrix = std::vector<uint64_t>; // t x t
    inline Matrix mat_mul(const Matrix& a, const Matrix& b, size_t t)
    {
      Matrix c(t * t);
      for (size_t i = 0; i < t; i++)
        for (size_t j = 0; j < t; j++) {
          uint64_t s = 0;
          for (size_t k = 0; k < t; k++)
            s = addmod(s, mulmod(a[i * t + k], b[k * t + j]));
          c[i * t + j] = s;
        }
      return c;
    }
    // the characteristic polynomial of a, if it can be irreducible: false when e_0, a e_0, .., a^(t-1) e_0 are dependent
    inline bool char_poly_if_cyclic(const Matrix& a, size_t t, Poly* f)
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
            s = addmod(s, mulmod(a[i * t + j], v[j]));
          w[i] = s;
        }
        v = w;
      }
      for (size_t col = 0; col < t; col++) {
        size_t piv = col;
        while (piv < t && rows[piv][col] == 0)
          piv++;
        if (piv == t) return false;
        std::swap(rows[piv], rows[col]);
        const uint64_t inv = invmod(rows[col][col]);
        for (size_t j = col; j <= t; j++)
          rows[col][j] = mulmod(rows[col][j], inv);
        for (size_t i = 0; i < t; i++) {
          const uint64_t m = rows[i][col];
          if (i == col || m == 0) continue;
          for (size_t j = col; j <= t; j++)
            rows[i][j] = submod(rows[i][j], mulmod(m, rows[col][j]));
        }
      }
      f->assign(t + 1, 0); // x^t - sum c_k x^k
      for (size_t k = 0; k < t; k++)
        (*f)[k] = submod(0, rows[k][t]);
      (*f)[t] = 1;
      return true;
    }
    inline bool diagonal_is_good(const std::vector<uint64_t>& diag)
    {
      const size_t t = diag.size();
      Matrix m(t * t, 1);
      for (size_t i = 0; i < t; i++)
        m[i * t + i] = diag[i];
      Matrix cur = m;
      Poly f;
      for (size_t i = 1; i <= 2 * t; i++) {
        if (!char_poly_if_cyclic(cur, t, &f) || !is_irreducible(f)) return false;
        if (i < 2 * t) cur = mat_mul(m, cur, t);
      }
      return true;
    }

    struct Params {
      int t = 0, alpha = 0, r_f = 0, r_p = 0;
      int draws = 0;              // diagonals drawn, 0 where the specification fixes it
      std::vector<uint64_t> rc;   // r_f t + r_p canonical residues, round order
      std::vector<uint64_t> diag; // t canonical residues: the diagonal of M_I
    };

    inline Params derive(int t)
    {
      Params Q;
      const int n = goldilocks_params::NBITS;
      Q.t = t, Q.alpha = 3;
      while (poseidon2::gcd_u64((uint64_t)Q.alpha, P - 1) != 1)
        Q.alpha++;
      poseidon2::round_numbers(n, std::log2((double)P), t, Q.alpha, &Q.r_f, &Q.r_p);
      poseidon2::Grain g(n, t, Q.r_f, Q.r_p);
      const size_t count = (size_t)Q.r_f * t + Q.r_p;
      while (Q.rc.size() < count) {
        const uint64_t v = draw(g);
        if (v < P) Q.rc.push_back(v);
      }
      if (t == 2) {
        Q.diag = {2, 3};
      } else if (t == 3) {
        Q.diag = {2, 2, 3};
      } else {
        Q.diag.resize((size_t)t);
        do {
          for (int i = 0; i < t; i++) {
            const uint64_t v = draw(g);
            Q.diag[(size_t)i] = v >= P ? v - P : v;
          }
          Q.draws++;
        } while (!diagonal_is_good(Q.diag));
      }
      return Q;
    }

    // the parameters of t, derived once per process; nullptr for a width outside the eight
    inline std::shared_ptr<const Params> params(unsigned t)
    {
      if (!width_supported(t)) return nullptr;
      static std::mutex mtx;
      static std::map<unsigned, std::shared_ptr<const Params>> cache;
      std::lock_guard<std::mutex> lk(mtx);
      auto& slot = cache[t];
      if (!slot) slot = std::make_shared<const Params>(derive((int)t));
      return slot;
    }

  } // namespace poseidon2_gold
} // namespace icicle_hip
