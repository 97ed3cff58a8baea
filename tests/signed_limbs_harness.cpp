// TEST-ONLY stand-alone program (its own main) over the signed layer of bigfield.hpp and the mixed addition of ec.hpp that runs
// on it, built for the host with the bound tracker on (-DBIGFIELD_BOUNDS) and driven by tests/test_signed_limbs_cpu.py through
// stdin / stdout. Being a program, it can be built once more with -fsanitize=address,undefined and run as it is.
//
// One request per line, one answer line each:
//   F <field> <op> <flag> <a: N limbs> <b: N limbs> <c: N limbs> <d: N limbs>    limbs as signed decimal integers
//       -> "R <N limbs of the result, signed>"
//       field 0 = bn254's Fq, 1 = grumpkin's Fq (bn254's Fr); ops: add sub neg add2 cneg norm mul sqr mul_add mul_inplace
//       mul_add_inplace_c tou1 tou2 tou8 (to_unsigned<K>). The tracker's record of every operand is claimed from the limbs
//       themselves (their exact value, their smallest and largest limb), so a request outside what an operation can take aborts.
//   C <curve> <n>  followed by n lines "<x: 8 words> <y: 8 words> <negate> <mode>"    curve 0 = bn254, 1 = grumpkin
//       -> "P <24 words: canonical projective X, Y, Z>" of the madd() chain over the points, as k_accumulate runs it:
//       (0, 0) skipped, load_plain, the sign applied by cneg_madd (mode 0) or by cneg (mode 1), madd, to_proj at the end.
//       madd() asserts its invariant and re-imposes it on the tracker at the top of every addition (the fixed point).
//   T <k>  -> a madd() whose operand has one limb at 2^29 - 1 + k: "T ok" for k = 0, the tracker's abort for k = 1
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../icicle_amd/csrc/ec.hpp"

#ifndef BIGFIELD_BOUNDS
  #error "build with -DBIGFIELD_BOUNDS"
#endif

using namespace icicle_hip;

namespace {
  template <class PR>
  typename FieldOps<PR>::fe from_limbs(const long long* v)
  {
    using F = FieldOps<PR>;
    constexpr int N = F::N;
    typename F::fe r;
    long double val = 0, p = 0, w = 1;
    double llo = 0, lhi = 0;
    for (int i = 0; i < N; i++) {
      r.l[i] = (uint32_t)(int32_t)v[i];
      val += (long double)v[i] * w;
      p += (long double)PR::P[i] * w;
      w *= (long double)(1u << RB);
      if (i < N - 1) {
        llo = (i == 0 || (double)v[i] < llo) ? (double)v[i] : llo;
        lhi = (i == 0 || (double)v[i] > lhi) ? (double)v[i] : lhi;
      }
    }
    const double q = (double)(val / p), eps = 1e-9 * ((q < 0 ? -q : q) + 1.0);
    F::sclaim(r, q - eps, q + eps, llo, lhi, (double)v[N - 1], (double)v[N - 1]);
    return r;
  }

  template <class PR>
  int field_request(const std::string& op, int flag, const long long* in, long long* out)
  {
    using F = FieldOps<PR>;
    constexpr int N = F::N;
    typename F::fe a = from_limbs<PR>(in), b = from_limbs<PR>(in + N), c = from_limbs<PR>(in + 2 * N), d = from_limbs<PR>(in + 3 * N), r;
    if (op == "add") r = F::sadd(a, b);
    else if (op == "sub") r = F::ssub(a, b);
    else if (op == "neg") r = F::sneg(a);
    else if (op == "add2") r = F::sadd2(a, b);
    else if (op == "cneg") r = F::scneg(a, flag != 0);
    else if (op == "norm") r = F::snormalise(a);
    else if (op == "mul") r = F::smul(a, b);
    else if (op == "sqr") r = F::ssqr(a);
    else if (op == "mul_add") r = F::smul_add(a, b, c, d);
    else if (op == "mul_inplace") { r = a; F::smul_inplace(r, b); }
    else if (op == "mul_add_inplace_c") { r = c; F::smul_add_inplace_c(r, a, b, d); }
    else if (op == "tou1") r = F::template to_unsigned<1>(a);
    else if (op == "tou2") r = F::template to_unsigned<2>(a);
    else if (op == "tou8") r = F::template to_unsigned<8>(a);
    else return -1;
    for (int i = 0; i < N; i++)
      out[i] = (long long)(int32_t)r.l[i];
    return 0;
  }

  template <class C>
  void chain_request(const std::vector<uint32_t>& rows, int n, uint32_t* out)
  {
    using E = EC<C>;
    static_assert(E::SIGNED_MADD, "the chains are about the signed madd");
    constexpr int PW = 2 * E::N32;
    typename E::XYZZ acc;
    bool empty = true;
    for (int i = 0; i < n; i++) {
      const uint32_t* w = rows.data() + (size_t)i * (PW + 2);
      if (E::words_are_zero(w)) continue;
      const bool negate = w[PW] != 0;
      const typename E::Aff a = w[PW + 1] ? E::cneg(E::load_plain(w), negate) : E::cneg_madd(E::load_plain(w), negate);
      E::madd(acc, empty, a);
    }
    E::store_proj_canonical(out, E::to_proj(acc, empty));
  }

  // one limb of the operand's y at 2^29 - 1 + k: k = 0 is the edge madd() states for its operand, k = 1 is outside it
  int trip_request(int k)
  {
    using E = EC<bn254_g1>;
    using F = E::F;
    E::Aff b;
    E::XYZZ acc;
    bool empty = true;
    long long x[F::N] = {5, 4, 3, 2, 1, 0, 0, 0, 1}, y[F::N] = {7, 0, (long long)RB_MASK + k, 1, 2, 3, 4, 5, 1};
    b.x = from_limbs<bn254_fq_params>(x);
    b.y = from_limbs<bn254_fq_params>(y);
    E::madd(acc, empty, b); // (the operand is checked before the first-point path as well)
    return empty ? 1 : 0;
  }
} // namespace

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    std::string kind;
    if (!(ss >> kind)) continue;
    if (kind == "F") {
      int field, flag;
      std::string op;
      long long in[4 * 9], out[9];
      ss >> field >> op >> flag;
      for (auto& v : in)
        ss >> v;
      if (!ss) return 2;
      const int e = field == 0 ? field_request<bn254_fq_params>(op, flag, in, out) : field_request<bn254_fr_params>(op, flag, in, out);
      if (e) return 3;
      std::printf("R");
      for (long long v : out)
        std::printf(" %lld", v);
      std::printf("\n");
    } else if (kind == "C") {
      int curve, n;
      ss >> curve >> n;
      if (!ss || n < 0) return 2;
      std::vector<uint32_t> rows((size_t)n * 18);
      for (int i = 0; i < n; i++) {
        if (!std::getline(std::cin, line)) return 2;
        std::istringstream rs(line);
        for (int k = 0; k < 18; k++)
          rs >> rows[(size_t)i * 18 + k];
        if (!rs) return 2;
      }
      uint32_t out[24];
      if (curve == 0)
        chain_request<bn254_g1>(rows, n, out);
      else
        chain_request<grumpkin_g1>(rows, n, out);
      std::printf("P");
      for (uint32_t v : out)
        std::printf(" %u", v);
      std::printf("\n");
    } else if (kind == "T") {
      int k;
      ss >> k;
      trip_request(k);
      std::printf("T ok\n");
    } else {
      return 2;
    }
  }
  std::fflush(stdout);
  return 0;
}
