// TEST-ONLY stand-alone program (its own main) over ec.hpp's add_signed -- the complete projective addition on the signed layer
// of bigfield.hpp that the bucket reduction of bn254 and grumpkin uses -- and the small-constant step under it, built for the host
// with the bound tracker on (-DBIGFIELD_BOUNDS) and driven by tests/test_signed_add_cpu.py through stdin / stdout. Being a
// program, it can be built once more with -fsanitize=address,undefined and run as it is.
//
// One request per line, one answer line each; limbs as signed decimal integers, a point as 27 limbs (X, Y, Z in Montgomery form,
// any representative). The tracker's record of every operand is claimed from the limbs themselves (exact value, smallest and
// largest limb), so a request outside what add_signed states for its operands aborts.
//   S <field> <K> <a: 9 limbs>           -> "R <9 limbs>" of smul_small<K>(a); field 0 = bn254's Fq, 1 = grumpkin's Fq; K in 3 9 12 -9 64 -64
//   A <curve> <p: 27 limbs> <q: 27 limbs> -> "P <24 words: canonical projective X, Y, Z>" of add_signed(p, q); curve 0 = bn254, 1 = grumpkin
//   L <curve> <n>  followed by n lines "<bucket: 27 limbs>"
//       -> "P <24 words of tri> <24 words of line>" after the loop of k_reduce_wave over the buckets in the order given:
//       tri = add_signed(tri, line); line = add_signed(line, bucket), both from the identity. add_signed asserts its operand
//       contract and re-imposes it on the tracker at the top of every addition and asserts the loop value at the end (the fixed point).
//   T <k>  -> an add_signed whose second operand has one limb at 2^29 - 1 + k: "T ok" for k = 0, the tracker's abort for k = 1
#include <cstdint>
#include <cstdio>
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
  int small_request(int K, const long long* in, long long* out)
  {
    using F = FieldOps<PR>;
    typename F::fe a = from_limbs<PR>(in), r;
    switch (K) {
    case 3: r = F::template smul_small<3>(a); break;
    case 9: r = F::template smul_small<9>(a); break;
    case 12: r = F::template smul_small<12>(a); break;
    case -9: r = F::template smul_small<-9>(a); break;
    case 64: r = F::template smul_small<64>(a); break;
    case -64: r = F::template smul_small<-64>(a); break;
    default: return -1;
    }
    for (int i = 0; i < F::N; i++)
      out[i] = (long long)(int32_t)r.l[i];
    return 0;
  }

  template <class C>
  typename EC<C>::Proj point_from_limbs(const long long* v)
  {
    using PR = typename C::fq;
    typename EC<C>::Proj p;
    p.x = from_limbs<PR>(v);
    p.y = from_limbs<PR>(v + 9);
    p.z = from_limbs<PR>(v + 18);
    return p;
  }
  template <class C>
  void store(uint32_t* out, const typename EC<C>::Proj& p)
  {
    EC<C>::store_proj_canonical(out, EC<C>::signed_to_unsigned(p));
  }

  template <class C>
  void add_request(const long long* in, uint32_t* out)
  {
    store<C>(out, EC<C>::add_signed(point_from_limbs<C>(in), point_from_limbs<C>(in + 27)));
  }

  template <class C>
  void loop_request(const std::vector<long long>& rows, int n, uint32_t* out)
  {
    using E = EC<C>;
    typename E::Proj line = E::proj_identity(), tri = E::proj_identity();
    for (int i = 0; i < n; i++) {
      tri = E::add_signed(tri, line);
      line = E::add_signed(line, point_from_limbs<C>(rows.data() + (size_t)i * 27));
    }
    store<C>(out, tri);
    store<C>(out + 24, line);
  }

  // one limb of the second operand's x at 2^29 - 1 + k: k = 0 is the edge add_signed states, k = 1 is outside it
  void trip_request(int k)
  {
    using E = EC<bn254_g1>;
    long long q[27] = {5, 4, (long long)RB_MASK + k, 2, 1, 0, 0, 0, 1, 7, 0, 9, 1, 2, 3, 4, 5, 1, 1, 2, 3, 4, 5, 6, 7, 8, 0};
    (void)E::add_signed(E::proj_identity(), point_from_limbs<bn254_g1>(q));
  }
} // namespace

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    std::string kind;
    if (!(ss >> kind)) continue;
    if (kind == "S") {
      int field, K;
      long long in[9], out[9];
      ss >> field >> K;
      for (auto& v : in)
        ss >> v;
      if (!ss) return 2;
      const int e = field == 0 ? small_request<bn254_fq_params>(K, in, out) : small_request<bn254_fr_params>(K, in, out);
      if (e) return 3;
      std::printf("R");
      for (long long v : out)
        std::printf(" %lld", v);
      std::printf("\n");
    } else if (kind == "A") {
      int curve;
      long long in[54];
      ss >> curve;
      for (auto& v : in)
        ss >> v;
      if (!ss) return 2;
      uint32_t out[24];
      if (curve == 0)
        add_request<bn254_g1>(in, out);
      else
        add_request<grumpkin_g1>(in, out);
      std::printf("P");
      for (uint32_t v : out)
        std::printf(" %u", v);
      std::printf("\n");
    } else if (kind == "L") {
      int curve, n;
      ss >> curve >> n;
      if (!ss || n < 0) return 2;
      std::vector<long long> rows((size_t)n * 27);
      for (int i = 0; i < n; i++) {
        if (!std::getline(std::cin, line)) return 2;
        std::istringstream rs(line);
        for (int k = 0; k < 27; k++)
          rs >> rows[(size_t)i * 27 + k];
        if (!rs) return 2;
      }
      uint32_t out[48];
      if (curve == 0)
        loop_request<bn254_g1>(rows, n, out);
      else
        loop_request<grumpkin_g1>(rows, n, out);
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
