// Host build of the Poseidon code: icicle_amd/csrc/poseidon_params.h (the derivation) and poseidon.hpp (the hash a lane computes),
// compiled with g++ by tests/test_poseidon_cpu.py -- plainly, with -DBIGFIELD_BOUNDS (the bound tracker of bigfield.hpp asserts the
// precondition of every field operation the lane code performs) and with -fsanitize=address,undefined.
//   poseidon_host_harness params         for every built (field, t): "params <field> <t> <R_F> <R_P>", then "rc", "mds", "pre" and "sparse"
//                                        lines of canonical hex values (the matrices row-major)
//   poseidon_host_harness hash <file>    <file> holds one case per line: <field> <t> <tag or -> <batch> <hex element> ..;
//                                        per case one line of hex digests through the word reader and one through the padded-leaf reader
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../icicle_amd/csrc/poseidon.hpp"
#include "../icicle_amd/csrc/poseidon_params.h"

using namespace icicle_hip;

static const char* const FIELDS[4] = {"bn254", "bls12_381", "bls12_377", "grumpkin"};
static const unsigned WIDTHS[4] = {3, 5, 9, 12};

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
static int print_field(int f)
{
  for (unsigned t : WIDTHS) {
    if (f == 1 && t == 3) continue; // not built
    const auto P = poseidon::params<PR>(t);
    if (!P) return 1;
    printf("params %s %u %d %d\n", FIELDS[f], t, P->r_f, P->r_p);
    print_line<PR>("rc", P->rc);
    print_line<PR>("mds", P->mds);
    print_line<PR>("pre", P->pre);
    print_line<PR>("sparse", P->sparse);
  }
  for (unsigned t : {0u, 1u, 2u, 4u, 6u, 8u, 10u, 11u, 13u})
    if (poseidon::params<PR>(t)) return 1;
  return 0;
}

template <class PR, int T>
static void hash_case(const PoseidonCtx& c, const std::vector<uint32_t>& in, uint64_t batch, std::string* words, std::string* padded)
{
  const uint64_t arity = T - c.has_tag;
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(in.data());
  for (uint64_t b = 0; b < batch; b++) {
    uint32_t d[8];
    Poseidon<PR, T>::hash(PoseidonWords{in.data() + 8 * b * arity}, c, d);
    *words += (b ? " " : "") + hex_of(d);
    // the same message as a layer-0 chunk that lies wholly inside the leaves
    Poseidon<PR, T>::hash(PoseidonPadded{ReadPadded{bytes, 32 * b * arity, 32 * arity * batch, nullptr, 32}}, c, d);
    *padded += (b ? " " : "") + hex_of(d);
  }
}

template <class PR>
static bool hash_field(unsigned t, const std::string& tag, const std::vector<uint32_t>& in, uint64_t batch, std::string* w, std::string* p)
{
  const auto P = poseidon::params<PR>(t);
  if (!P) return false;
  const std::vector<uint32_t> tab = poseidon_device_tables<Fe<PR>>((int)t, P->rc, P->mds, P->pre, P->sparse);
  PoseidonCtx c{tab.data(), P->r_p, 0, {0}};
  if (tag != "-") {
    uint32_t tw[8];
    if (!words_of(tag, tw) || !poseidon::HostField<PR>::below_p(tw)) return false;
    const Fe<PR> m = FieldOps<PR>::reduce(FieldOps<PR>::from_canonical(tw));
    c.has_tag = 1;
    memcpy(c.tag, m.l, sizeof c.tag);
  }
  if (in.size() != 8 * batch * (t - c.has_tag)) return false;
  switch (t) {
  case 3: hash_case<PR, 3>(c, in, batch, w, p); return true;
  case 5: hash_case<PR, 5>(c, in, batch, w, p); return true;
  case 9: hash_case<PR, 9>(c, in, batch, w, p); return true;
  case 12: hash_case<PR, 12>(c, in, batch, w, p); return true;
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
    uint64_t batch = 0;
    if (!(ls >> field >> t >> tag >> batch)) continue;
    std::vector<uint32_t> in;
    while (ls >> tok) {
      uint32_t w[8];
      if (!words_of(tok, w)) return 1;
      in.insert(in.end(), w, w + 8);
    }
    std::string words, padded;
    bool ok = false;
    if (field == FIELDS[0]) ok = hash_field<bn254_fr_params>(t, tag, in, batch, &words, &padded);
    if (field == FIELDS[1]) ok = t != 3 && hash_field<bls12_381_fr_params>(t, tag, in, batch, &words, &padded);
    if (field == FIELDS[2]) ok = hash_field<bls12_377_fr_params>(t, tag, in, batch, &words, &padded);
    if (field == FIELDS[3]) ok = hash_field<bn254_fq_params>(t, tag, in, batch, &words, &padded);
    if (!ok) return 1;
    printf("%s\n%s\n", words.c_str(), padded.c_str());
  }
  return 0;
}

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "params"))
    return print_field<bn254_fr_params>(0) || print_field<bls12_381_fr_params>(1) || print_field<bls12_377_fr_params>(2) || print_field<bn254_fq_params>(3);
  if (argc == 3 && !strcmp(argv[1], "hash")) return hash_file(argv[2]);
  fprintf(stderr, "usage: %s params | hash <file>\n", argv[0]);
  return 2;
}
