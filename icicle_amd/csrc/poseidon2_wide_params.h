// Poseidon2 parameters over a 256-bit scalar field for a width t in {2, 3, 4, 8}, derived from the specification when the first
// hasher of a (field, t) is created. Host only, no HIP: the CPU tests compile it with g++ (tests/poseidon2_wide_host_harness.cpp).
// Nothing here is a table: every number below follows from p, t and the security level.
//
// The derivation is that of poseidon2_params.h, which states it and its sources. What depends on p only through its bit length,
// log2 p and alpha -- the round-number search and the Grain LFSR -- is that header's code, called from here. What computes in F_p
// -- the rejection sampling, the diagonal of M_I and the irreducibility test of its characteristic polynomials -- is written
// here over the host big-field helper of poseidon_params.h (HostField<PR>: Montgomery form on 29-bit limbs, every result
// reduced to [0, p)), with the 8-word p itself as the exponent of the Frobenius map.
//   alpha        smallest a >= 3 with gcd(a, p - 1) = 1: 5 for BN254, Grumpkin and BLS12-381, 11 for BLS12-377, 3 for stark252
//   R_F, R_P     8 and 56, 56, 56, 57 (alpha 5), 37 (alpha 11), 83, 83, 84, 84 (alpha 3) for t = 2, 3, 4, 8
//   constants    Grain seeded with n = the bit length of p (Grumpkin's scalar field: 254 -- unlike the reference's Poseidon tables,
//                which poseidon_params.h has to follow to 255), n bits MSB first per value, values >= p rejected
//   M_I          diagonal (2, 3), (2, 2, 3), or t draws of n bits reduced mod p (one subtraction: 2^n < 2 p), redrawn until the
//                characteristic polynomial of M_I^i is irreducible for i = 1 .. 2t: between 1 and 31 draws for the pairs built
// tests/poseidon2_model_wide.py holds the same derivation in Python integers; tests/golden/poseidon2_vectors_wide.json holds
// digests of the reference, which prove both. profiles/poseidon2_notes.md has the time each pair takes.
#pragma once
#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <vector>
#include "poseidon2_params.h"
#include "poseidon_params.h"

namespace icicle_hip {
  namespace poseidon2_wide {

    using poseidon::HostField;

    inline bool width_supported(unsigned t) { return t == 2 || t == 3 || t == 4 || t == 8; }

    // (p - 1) mod a for a small a, from the words of p
    template <class PR>
    inline uint32_t p_minus_1_mod(uint32_t a)
    {
      uint64_t r = 0;
      for (int i = PR::NL32 - 1; i >= 0; i--)
        r = ((r << 32) | PR::P32[i]) % a;
      return (uint32_t)((r + a - 1) % a);
    }
    template <class PR>
    inline int alpha_of()
    {
      uint32_t a = 3;
      while (poseidon2::gcd_u64(a, p_minus_1_mod<PR>(a)) != 1) // gcd(a, p - 1) = gcd(a, (p - 1) mod a); gcd(a, 0) = a
        a++;
      return (int)a;
    }
    template <class PR>
    inline double log2_p()
    {
      long double v = 0;
      for (int i = PR::NL32 - 1; i >= 0; i--)
        v = v * 4294967296.0L + (long double)PR::P32[i];
      return (double)std::log2(v);
    }

    // n bits of the stream, MSB first, as little-endian words
    template <class PR>
    inline void draw(poseidon2::Grain& g, int n, uint32_t* w)
    {
      for (int i = PR::NL32 - 1; i >= 0; i--) {
        const int bits = n - 32 * i >= 32 ? 32 : n - 32 * i > 0 ? n - 32 * i : 0;
        w[i] = bits ? g.bits(bits) : 0;
      }
    }
    // w -= p, for p <= w < 2 p
    template <class PR>
    inline void sub_p(uint32_t* w)
    {
      uint64_t borrow = 0;
      for (int i = 0; i < PR::NL32; i++) {
        const uint64_t d = (uint64_t)w[i] - PR::P32[i] - borrow;
        w[i] = (uint32_t)d;
        borrow = d >> 63;
      }
    }

    // ---- polynomials over F_p (coefficients low first) and matrices (row-major), entries reduced Montgomery elements ------------------
    template <class PR>
    using Poly = std::vector<Fe<PR>>;

    template <class PR>
    inline bool fe_equal(const Fe<PR>& a, const Fe<PR>& b)
    {
      for (int i = 0; i < PR::NL; i++)
        if (a.l[i] != b.l[i]) return false;
      return true;
    }
    template <class PR>
    inline Fe<PR> fe_one()
    {
      return FieldOps<PR>::reduce(FieldOps<PR>::one());
    }

    // a b mod f, f monic of degree t, a and b of degree < t
    template <class PR>
    inline Poly<PR> poly_mulmod(const Poly<PR>& a, const Poly<PR>& b, const Poly<PR>& f)
    {
      using H = HostField<PR>;
      const size_t t = f.size() - 1;
      Poly<PR> c(2 * t - 1, FieldOps<PR>::zero());
      for (size_t i = 0; i < t; i++)
        for (size_t j = 0; j < t; j++)
          c[i + j] = H::add(c[i + j], H::mul(a[i], b[j]));
      for (size_t k = 2 * t - 2; k >= t; k--) { // x^k = -(f_0 + .. + f_(t-1) x^(t-1)) x^(k-t)
        const Fe<PR> top = c[k];
        if (!H::is_zero(top))
          for (size_t i = 0; i < t; i++)
            c[k - t + i] = H::sub(c[k - t + i], H::mul(top, f[i]));
      }
      c.resize(t);
      return c;
    }
    template <class PR>
    inline void poly_trim(Poly<PR>& a)
    {
      while (!a.empty() && HostField<PR>::is_zero(a.back()))
        a.pop_back();
    }
    template <class PR>
    inline Poly<PR> poly_rem(Poly<PR> a, const Poly<PR>& b) // b trimmed, not zero
    {
      using H = HostField<PR>;
      const Fe<PR> inv = H::inv(b.back());
      while (a.size() >= b.size()) {
        const Fe<PR> q = H::mul(a.back(), inv);
        const size_t off = a.size() - b.size();
        if (!H::is_zero(q))
          for (size_t i = 0; i < b.size(); i++)
            a[off + i] = H::sub(a[off + i], H::mul(q, b[i]));
        a.pop_back();
      }
      poly_trim<PR>(a);
      return a;
    }
    template <class PR>
    inline bool poly_coprime(Poly<PR> a, Poly<PR> b)
    {
      poly_trim<PR>(a), poly_trim<PR>(b);
      while (!b.empty()) {
        Poly<PR> r = poly_rem<PR>(a, b);
        a = std::move(b), b = std::move(r);
      }
      return a.size() == 1;
    }
    // Rabin's test for a monic f of degree t >= 2
    template <class PR>
    inline bool is_irreducible(const Poly<PR>& f)
    {
      using H = HostField<PR>;
      const size_t t = f.size() - 1;
      const Fe<PR> zero = FieldOps<PR>::zero(), one = fe_one<PR>();
      Poly<PR> x(t, zero), h(t, zero);
      x[1] = one;
      // h = x^p mod f, the exponent word by word from the top
      h[0] = one;
      for (int wi = PR::NL32 - 1; wi >= 0; wi--)
        for (int b = 31; b >= 0; b--) {
          h = poly_mulmod<PR>(h, h, f);
          if (PR::P32[wi] >> b & 1) h = poly_mulmod<PR>(h, x, f);
        }
      // the Frobenius map g -> g^p is linear: row i of its matrix is x^(i p) = h^i
      std::vector<Poly<PR>> frob(t);
      frob[0].assign(t, zero), frob[0][0] = one;
      for (size_t i = 1; i < t; i++)
        frob[i] = poly_mulmod<PR>(frob[i - 1], h, f);
      Poly<PR> cur = x; // x^(p^k)
      for (size_t k = 1; k <= t; k++) {
        Poly<PR> next(t, zero);
        for (size_t i = 0; i < t; i++)
          if (!H::is_zero(cur[i]))
            for (size_t j = 0; j < t; j++)
              next[j] = H::add(next[j], H::mul(cur[i], frob[i][j]));
        cur = next;
        bool wanted = false; // k = t / q for a prime q | t
        if (k < t && t % k == 0) {
          const size_t q = t / k;
          wanted = true;
          for (size_t d = 2; d * d <= q; d++)
            if (q % d == 0) wanted = false;
        }
        if (wanted) {
          Poly<PR> diff(t);
          for (size_t j = 0; j < t; j++)
            diff[j] = H::sub(cur[j], x[j]);
          Poly<PR> g = diff;
          poly_trim<PR>(g);
          if (g.empty() || !poly_coprime<PR>(f, diff)) return false;
        }
      }
      for (size_t j = 0; j < t; j++)
        if (!fe_equal<PR>(cur[j], x[j])) return false;
      return true;
    }

    // the characteristic polynomial of a, if it can be irreducible: false when e_0, a e_0, .., a^(t-1) e_0 are dependent
    template <class PR>
    inline bool char_poly_if_cyclic(const poseidon::Vec<PR>& a, size_t t, Poly<PR>* f)
    {
      using H = HostField<PR>;
      const Fe<PR> zero = FieldOps<PR>::zero(), one = fe_one<PR>();
      // columns k < t: a^k e_0; column t: a^t e_0. Solve K c = a^t e_0.
      std::vector<Poly<PR>> rows(t, Poly<PR>(t + 1, zero));
      Poly<PR> v(t, zero), w(t, zero);
      v[0] = one;
      for (size_t k = 0; k <= t; k++) {
        for (size_t i = 0; i < t; i++)
          rows[i][k] = v[i];
        for (size_t i = 0; i < t; i++) {
          Fe<PR> s = zero;
          for (size_t j = 0; j < t; j++)
            s = H::add(s, H::mul(a[i * t + j], v[j]));
          w[i] = s;
        }
        v = w;
      }
      for (size_t col = 0; col < t; col++) {
        size_t piv = col;
        while (piv < t && H::is_zero(rows[piv][col]))
          piv++;
        if (piv == t) return false;
        std::swap(rows[piv], rows[col]);
        const Fe<PR> inv = H::inv(rows[col][col]);
        for (size_t j = col; j <= t; j++)
          rows[col][j] = H::mul(rows[col][j], inv);
        for (size_t i = 0; i < t; i++) {
          const Fe<PR> m = rows[i][col];
          if (i == col || H::is_zero(m)) continue;
          for (size_t j = col; j <= t; j++)
            rows[i][j] = H::sub(rows[i][j], H::mul(m, rows[col][j]));
        }
      }
      f->assign(t + 1, zero); // x^t - sum c_k x^k
      for (size_t k = 0; k < t; k++)
        (*f)[k] = H::sub(zero, rows[k][t]);
      (*f)[t] = one;
      return true;
    }
    template <class PR>
    inline bool diagonal_is_good(const poseidon::Vec<PR>& diag)
    {
      const size_t t = diag.size();
      poseidon::Vec<PR> m(t * t, fe_one<PR>());
      for (size_t i = 0; i < t; i++)
        m[i * t + i] = diag[i];
      poseidon::Vec<PR> cur = m;
      Poly<PR> f;
      for (size_t i = 1; i <= 2 * t; i++) {
        if (!char_poly_if_cyclic<PR>(cur, t, &f) || !is_irreducible<PR>(f)) return false;
        if (i < 2 * t) cur = poseidon::mat_mul<PR>(m, cur, t);
      }
      return true;
    }

    // Everything in Montgomery form, reduced to [0, p).
    template <class PR>
    struct Params {
      int t = 0, alpha = 0, r_f = 0, r_p = 0;
      int draws = 0;           // diagonals drawn, 0 where the specification fixes it
      poseidon::Vec<PR> rc;   // r_f t + r_p, round order
      poseidon::Vec<PR> diag; // t: the diagonal of M_I
    };

    template <class PR>
    Params<PR> derive(int t)
    {
      using H = HostField<PR>;
      using F = FieldOps<PR>;
      Params<PR> P;
      const int n = PR::NBITS;
      P.t = t, P.alpha = alpha_of<PR>();
      poseidon2::round_numbers(n, log2_p<PR>(), t, P.alpha, &P.r_f, &P.r_p);
      poseidon2::Grain g(n, t, P.r_f, P.r_p);
      const size_t count = (size_t)P.r_f * t + P.r_p;
      uint32_t w[PR::NL32];
      while (P.rc.size() < count) {
        draw<PR>(g, n, w);
        if (H::below_p(w)) P.rc.push_back(F::reduce(F::from_canonical(w)));
      }
      if (t == 2) {
        P.diag = {H::from_small(2), H::from_small(3)};
      } else if (t == 3) {
        P.diag = {H::from_small(2), H::from_small(2), H::from_small(3)};
      } else {
        P.diag.resize((size_t)t);
        do {
          for (int i = 0; i < t; i++) {
            draw<PR>(g, n, w);
            if (!H::below_p(w)) sub_p<PR>(w);
            P.diag[(size_t)i] = F::reduce(F::from_canonical(w));
          }
          P.draws++;
        } while (!diagonal_is_good<PR>(P.diag));
      }
      return P;
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

  } // namespace poseidon2_wide
} // namespace icicle_hip
