// Host harness for icicle_amd/csrc/vecops_ext_elem.hpp: the element code a lane of the shared kernels (k_vec2, k_vec_inv of
// vecops_tile.hpp) and of vecops_ext.hip's k_ext_mixed_mul runs for an extension element, compiled with plain g++.
//
//   harness cases <file>            every line of <file> is one fixture case, "field op size batch columns a_hex b_hex|- out_hex"
//                                   (tests/test_vecops_ext_cpu.py writes it from tests/golden/vecops_ext_vectors.json); each is
//                                   computed here the way the kernels compute it and compared with out_hex
//   harness random <seed> <n> <m>   n seeded random pairs per field: a * inv(a) = 1, a * conj_times(a) = norm(a),
//                                   norm(a b) = norm(a) norm(b), (a b) / b = a are checked here; the first m pairs are printed as
//                                   "field a b a*b inv(a)", words in hex, for the Python model to compare
//
// The shared inversion of a tile is linear in the one inverse it computes, so here each norm is inverted on its own with the same
// powers of R taken off (two for an inverse, one where a product with a numerator follows).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <fstream>
#include <sstream>

#include "../icicle_amd/csrc/vecops_ext_elem.hpp"

using namespace icicle_hip;

template <class EL>
struct Base;
template <class PR>
struct Base<SmallExtElem<PR>> {
  using S = SmallField<PR>;
  static uint32_t inv(uint32_t n, int unscales) // SmallElem: inv_raw, then unscale
  {
    uint32_t r = S::inv(n);
    for (int k = 0; k < unscales; k++)
      r = S::from_mont(r);
    return r;
  }
  static uint32_t mul(uint32_t a, uint32_t b) { return S::mul(a, b); }
  static uint64_t below(uint64_t r) { return r % PR::P; }
  static uint32_t make(uint64_t v) { return (uint32_t)v; }
  static void words(uint32_t v, uint32_t* w) { w[0] = v; }
};
template <>
struct Base<GoldExtElem> {
  using F = FieldOps<goldilocks_params>;
  static GoldFe inv(const GoldFe& n, int) { return F::inv(n); }
  static GoldFe mul(const GoldFe& a, const GoldFe& b) { return F::mul(a, b); }
  static uint64_t below(uint64_t r) { return r % goldilocks_params::P; }
  static GoldFe make(uint64_t v) { return F::make(v); }
  static void words(const GoldFe& v, uint32_t* w) { F::pack(w, v); }
};

static std::vector<uint32_t> unhex(const std::string& s)
{
  std::vector<uint8_t> b(s.size() / 2);
  for (size_t i = 0; i < b.size(); i++)
    b[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
  std::vector<uint32_t> w(b.size() / 4);
  if (!w.empty()) memcpy(w.data(), b.data(), w.size() * 4);
  return w;
}

// what k_vec_inv computes for one extension element (InvTile<> of vecops_ext.hip): conj_times(a) / norm(a), times num where DIV
template <class EL>
static typename EL::T inverse(const typename EL::T& den, const typename EL::T* num)
{
  if (EL::is_zero(den)) return EL::zero();
  typename EL::T c;
  const typename EL::BT n = EL::norm_conj(den, c);
  typename EL::T o = EL::mul_base_raw(c, Base<EL>::inv(n, num ? 1 : 2));
  if (num) o = EL::mul_raw(o, *num);
  return o;
}

template <class EL>
static bool run_case(const std::string& op, uint64_t size, uint32_t batch, bool columns, const std::vector<uint32_t>& a, const std::vector<uint32_t>& b,
                     const std::vector<uint32_t>& want)
{
  using T = typename EL::T;
  const uint64_t total = size * batch;
  std::vector<uint32_t> out(want.size(), 0xA5A5A5A5u);
  auto at = [&](uint64_t j, uint64_t k) { return columns ? j * batch + k : k * size + j; };
  if (op == "vector_add" || op == "vector_sub" || op == "vector_mul" || op.rfind("scalar_", 0) == 0) {
    const bool a_scalar = op[0] == 's';
    const int o = op.find("add") != std::string::npos ? VOP_ADD : op.find("sub") != std::string::npos ? VOP_SUB : VOP_MUL;
    for (uint64_t i = 0; i < total; i++) {
      const uint64_t ai = !a_scalar ? i : (columns ? i % batch : i / size); // k_vec2
      EL::store(&out[i * 4], EL::apply(o, EL::load(&a[ai * 4]), EL::load(&b[i * 4])));
    }
  } else if (op == "vector_mixed_mul") {
    for (uint64_t i = 0; i < total; i++)
      EL::store(&out[i * 4], EL::apply_mixed(EL::load(&a[i * 4]), EL::load_base(&b[i * EL::BW])));
  } else if (op == "vector_inv" || op == "vector_div") {
    for (uint64_t i = 0; i < total; i++) {
      const T num = EL::load(&a[i * 4]);
      EL::store(&out[i * 4], op == "vector_inv" ? inverse<EL>(num, nullptr) : inverse<EL>(EL::load(&b[i * 4]), &num));
    }
  } else if (op == "vector_sum" || op == "vector_product") {
    const bool prod = op == "vector_product";
    for (uint32_t k = 0; k < batch; k++) {
      T acc = prod ? EL::one() : EL::zero();
      for (uint64_t j = 0; j < size; j++) {
        const T x = EL::load(&a[at(j, k) * 4]);
        acc = prod ? EL::mul_raw(acc, x) : EL::sum(acc, x);
      }
      if (prod) acc = EL::scale_pow(acc, size);
      EL::store(&out[k * 4], acc);
    }
  } else if (op == "bit_reverse") {
    uint32_t logn = 0;
    while (((uint64_t)1 << logn) < size)
      logn++;
    for (uint32_t k = 0; k < batch; k++)
      for (uint64_t j = 0; j < size; j++) {
        uint64_t r = 0;
        for (uint32_t t = 0; t < logn; t++)
          r |= ((j >> t) & 1) << (logn - 1 - t);
        memcpy(&out[at(r, k) * 4], &a[at(j, k) * 4], 16);
      }
  } else {
    return false;
  }
  return out == want;
}

static int run_cases(const char* path)
{
  std::ifstream in(path);
  std::string line;
  int n = 0, bad = 0;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string field, op, ah, bh, oh;
    uint64_t size;
    uint32_t batch;
    int columns;
    if (!(ss >> field >> op >> size >> batch >> columns >> ah >> bh >> oh)) continue;
    const std::vector<uint32_t> a = unhex(ah), b = bh == "-" ? std::vector<uint32_t>() : unhex(bh), want = unhex(oh);
    bool ok = false;
    if (field == "babybear") ok = run_case<SmallExtElem<babybear_params>>(op, size, batch, columns, a, b, want);
    if (field == "koalabear") ok = run_case<SmallExtElem<koalabear_params>>(op, size, batch, columns, a, b, want);
    if (field == "goldilocks") ok = run_case<GoldExtElem>(op, size, batch, columns, a, b, want);
    n++;
    if (!ok) {
      bad++;
      printf("MISMATCH %s %s size %llu batch %u columns %d\n", field.c_str(), op.c_str(), (unsigned long long)size, batch, columns);
    }
  }
  printf("cases %d mismatches %d\n", n, bad);
  return bad || !n;
}

static uint64_t rng_state;
static uint64_t next_u64() // xorshift64*
{
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

template <class EL>
static std::string hex_of(const typename EL::T& x)
{
  uint32_t w[4];
  EL::store(w, x);
  char buf[40];
  snprintf(buf, sizeof buf, "%08x%08x%08x%08x", w[0], w[1], w[2], w[3]); // word by word, not byte order: the test reads it so
  return buf;
}

template <class EL>
static typename EL::T random_elem()
{
  uint32_t w[4];
  constexpr int D = 4 / EL::BW;
  for (int c = 0; c < D; c++)
    Base<EL>::words(Base<EL>::make(Base<EL>::below(next_u64())), w + c * EL::BW);
  return EL::load(w);
}

template <class EL>
static int run_random(const char* field, uint64_t seed, int n, int emit)
{
  using T = typename EL::T;
  rng_state = seed;
  int bad = 0;
  uint32_t one_w[4] = {1, 0, 0, 0}; // canonical 1 in either layout
  for (int i = 0; i < n; i++) {
    const T a = random_elem<EL>(), b = random_elem<EL>();
    const T ab = EL::apply(VOP_MUL, a, b), ia = inverse<EL>(a, nullptr);
    uint32_t w[4], v[4];
    // a * inv(a) = 1 (zero has no inverse: inv gives zero)
    EL::store(w, EL::apply(VOP_MUL, a, ia));
    if (EL::is_zero(a) ? (w[0] | w[1] | w[2] | w[3]) != 0 : memcmp(w, one_w, 16) != 0) bad++, printf("BAD inverse %s %d\n", field, i);
    // a * conj_times(a) = norm(a), as representatives
    T c;
    const typename EL::BT na = EL::norm_conj(a, c);
    const T nc = EL::mul_raw(a, c);
    uint32_t nw[4] = {0, 0, 0, 0};
    Base<EL>::words(na, nw);
    EL::store(w, nc);
    if (memcmp(w, nw, 16) != 0) bad++, printf("BAD conj %s %d\n", field, i);
    // norm(a b) = norm(a) norm(b) on raw products
    const typename EL::BT nab = EL::norm(EL::mul_raw(a, b));
    uint32_t x[2] = {0, 0}, y[2] = {0, 0};
    Base<EL>::words(nab, x);
    Base<EL>::words(Base<EL>::mul(na, EL::norm(b)), y);
    if (memcmp(x, y, 8) != 0) bad++, printf("BAD norm %s %d\n", field, i);
    // (a b) / b = a
    if (!EL::is_zero(b)) {
      EL::store(w, inverse<EL>(b, &ab));
      EL::store(v, a);
      if (memcmp(w, v, 16) != 0) bad++, printf("BAD quotient %s %d\n", field, i);
    }
    if (i < emit)
      printf("%s %s %s %s %s\n", field, hex_of<EL>(a).c_str(), hex_of<EL>(b).c_str(), hex_of<EL>(ab).c_str(), hex_of<EL>(ia).c_str());
  }
  return bad;
}

int main(int argc, char** argv)
{
  if (argc == 3 && !strcmp(argv[1], "cases")) return run_cases(argv[2]);
  if (argc == 5 && !strcmp(argv[1], "random")) {
    const uint64_t seed = strtoull(argv[2], nullptr, 10);
    const int n = atoi(argv[3]), emit = atoi(argv[4]);
    int bad = run_random<SmallExtElem<babybear_params>>("babybear", seed, n, emit);
    bad += run_random<SmallExtElem<koalabear_params>>("koalabear", seed + 1, n, emit);
    bad += run_random<GoldExtElem>("goldilocks", seed + 2, n, emit);
    printf("random %d per field, failures %d\n", n, bad);
    return bad != 0;
  }
  fprintf(stderr, "usage: %s cases <file> | random <seed> <n> <emit>\n", argv[0]);
  return 2;
}
