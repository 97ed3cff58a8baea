// Host build of the Poseidon2 code over the 256-bit fields: icicle_amd/csrc/poseidon2_wide_params.h (the derivation) and
// poseidon2_wide.hpp (the hash a lane computes), compiled with g++ by tests/test_poseidon2_wide_cpu.py -- plainly, with
// -DBIGFIELD_BOUNDS (the bound tracker of bigfield.hpp asserts the precondition of every field operation the lane code performs)
// and with -fsanitize=address,undefined.
//   poseidon2_wide_host_harness params         for every (field, t): "params <field> <t> <alpha> <R_F> <R_P> <draws>", then "rc" and "diag"
//                                              lines of canonical hex values
//   poseidon2_wide_host_harness times          for every (field, t): "<field> <t> <milliseconds the derivation took>"
//   poseidon2_wide_host_harness hash <file>    <file> holds one case per line: <field> <t> <tag or -> <size> <batch> <hex element> ..;
//                                              per case one line of hex digests through the word reader and one through the padded-leaf reader
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../icicle_amd/csrc/poseidon2_wide.hpp"
#include "../icicle_amd/csrc/poseidon2_wide_params.h"

using namespace icicle_hip;

static const char* const FIELDS[5] = {"bn254", "bls12_381", "bls12_377", "grumpkin", "stark252"};
static const unsigned WIDTHS[4] = {2, 3, 4, 8};

static std::string hex_of(const uint32_t* w)
{
  char buf[72];
  int top = 7;
  while (top > 0 && w[top] == 0)
    top--;
  int n = snprintf(buf, sizeof buf, "%x", w[top]);
  for (int i = top - 1; i >= 0; i--)
    n += snprintf(buf + n, sizeof buf - n, "%08x", w[i]);
  return buf;
}

static bool words_of(const std::string& hex, uint32_t* w)
{
  memset(w, 0, 32);
  if (hex.empty() || hex.size() > 64) return false;
  for (size_t i = 0; i < hex.size(); i++) {
    const char ch = hex[hex.size() - 1 - i];
    const int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
    if (d < 0) return false;
    w[i / 8] |= (uint32_t)d << (4 * (i % 8));
  }
  return true;
}

template <class PR>
static void print_line(const char* name, const std::vector<Fe<PR>>& v)
{
  printf("%s", name);
  for (const Fe<PR>& e : v) {
    uint32_t w[8];
    poseidon::to_words<PR>(e, w);
    printf(" %s", hex_of(w).c_str());
  }
  printf("\n");
}

template <class PR>
static int print_field(int f, bool times)
{
  for (unsigned t : WIDTHS) {
    const auto t0 = std::chrono::steady_clock::now();
    const auto P = poseidon2_wide::params<PR>(t);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!P) return 1;
    if (times) {
      printf("%s %u %.1f\n", FIELDS[f], t, ms);
      continue;
    }
    printf("params %s %u %d %d %d %d\n", FIELDS[f], t, P->alpha, P->r_f, P->r_p, P->draws);
    print_line<PR>("rc", P->rc);
    print_line<PR>("diag", P->diag);
    if (P->alpha != poseidon2_wide_alpha<PR>()) return 1; // the S-box the lane code is compiled with
  }
  for (unsigned t : {0u, 1u, 5u, 6u, 7u, 9u, 12u, 16u, 20u, 24u})
    if (poseidon2_wide::params<PR>(t)) return 1;
  return 0;
}

template <class PR, int T>
static void hash_case(const Poseidon2WideCtx& c, const std::vector<uint32_t>& in, uint64_t size, uint64_t batch, std::string* words, std::string* padded)
{
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(in.data());
  for (uint64_t b = 0; b < batch; b++) {
    uint32_t d[8];
    Poseidon2Wide<PR, T>::hash(PoseidonWords{in.data() + 8 * b * size}, size, c, d);
    *words += (b ? " " : "") + hex_of(d);
    // the same message as a layer-0 chunk that lies wholly inside the leaves
    Poseidon2Wide<PR, T>::hash(PoseidonPadded{ReadPadded{bytes, 32 * b * size, 32 * size * batch, nullptr, 32}}, size, c, d);
    *padded += (b ? " " : "") + hex_of(d);
  }
}

template <class PR>
static bool hash_field(unsigned t, const std::string& tag, const std::vector<uint32_t>& in, uint64_t size, uint64_t batch, std::string* w, std::string* p)
{
  const auto P = poseidon2_wide::params<PR>(t);
  if (!P || size == 0 || in.size() != 8 * batch * size) return false;
  const std::vector<uint32_t> consts = poseidon2_wide_device_constants<PR>(P->rc, P->diag);
  Poseidon2WideCtx c{consts.data(), P->r_f / 2, P->r_p, 0, {0}};
  if (tag != "-") {
    uint32_t tw[8];
    if (!words_of(tag, tw) || !poseidon::HostField<PR>::below_p(tw)) return false;
    const Fe<PR> m = FieldOps<PR>::reduce(FieldOps<PR>::from_canonical(tw));
    c.has_tag = 1;
    memcpy(c.tag, m.l, sizeof c.tag);
  }
  switch (t) {
  case 2: hash_case<PR, 2>(c, in, size, batch, w, p); return true;
  case 3: hash_case<PR, 3>(c, in, size, batch, w, p); return true;
  case 4: hash_case<PR, 4>(c, in, size, batch, w, p); return true;
  case 8: hash_case<PR, 8>(c, in, size, batch, w, p); return true;
  }
  return false;
}

static int hash_file(const char* path)
{
  std::ifstream file(path);
  if (!file) return 1;
  std::string line;
  while (std::getline(file, line)) {
    std::istringstream ls(line);
    std::string field, tag, tok;
    unsigned t = 0;
    uint64_t size = 0, batch = 0;
    if (!(ls >> field >> t >> tag >> size >> batch)) continue;
    std::vector<uint32_t> in;
    while (ls >> tok) {
      uint32_t w[8];
      if (!words_of(tok, w)) return 1;
      in.insert(in.end(), w, w + 8);
    }
    std::string words, padded;
    bool ok = false;
    if (field == FIELDS[0]) ok = hash_field<bn254_fr_params>(t, tag, in, size, batch, &words, &padded);
    if (field == FIELDS[1]) ok = hash_field<bls12_381_fr_params>(t, tag, in, size, batch, &words, &padded);
    if (field == FIELDS[2]) ok = hash_field<bls12_377_fr_params>(t, tag, in, size, batch, &words, &padded);
    if (field == FIELDS[3]) ok = hash_field<bn254_fq_params>(t, tag, in, size, batch, &words, &padded);
    if (field == FIELDS[4]) ok = hash_field<stark252_fr_params>(t, tag, in, size, batch, &words, &padded);
    if (!ok) return 1;
    printf("%s\n%s\n", words.c_str(), padded.c_str());
  }
  return 0;
}

int main(int argc, char** argv)
{
  const bool params = argc == 2 && !strcmp(argv[1], "params"), times = argc == 2 && !strcmp(argv[1], "times");
  if (params || times)
    return print_field<bn254_fr_params>(0, times) || print_field<bls12_381_fr_params>(1, times) || print_field<bls12_377_fr_params>(2, times) ||
           print_field<bn254_fq_params>(3, times) || print_field<stark252_fr_params>(4, times);
  if (argc == 3 && !strcmp(argv[1], "hash")) return hash_file(argv[2]);
  fprintf(stderr, "usage: %s params | times | hash <file>\n", argv[0]);
  return 2;
}
