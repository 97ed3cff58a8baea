// Host build of the Poseidon2 code: icicle_amd/csrc/poseidon2_params.h (the derivation) and poseidon2.hpp (the hash a lane computes),
// compiled with g++ by tests/test_poseidon2_cpu.py -- once plainly, once with -fsanitize=address,undefined.
//   poseidon2_host_harness params         for every (field, width): "params <field> <t> <alpha> <R_F> <R_P>", "rc <hex> ..", "diag <hex> .."
//   poseidon2_host_harness hash <file>    <file> holds one case per line: <field> <t> <tag or -> <size> <batch> <hex element> ..;
//                                         per case one line of hex digests through the word reader and one through the padded-leaf reader
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../icicle_amd/csrc/poseidon2.hpp"
#include "../icicle_amd/csrc/poseidon2_params.h"

using namespace icicle_hip;

static const int WIDTHS[8] = {2, 3, 4, 8, 12, 16, 20, 24};
static const char* const FIELDS[2] = {"babybear", "koalabear"};
static uint32_t prime_of(int field) { return field == 0 ? babybear_params::P : koalabear_params::P; }

template <class PR, int T>
static void hash_case(const Poseidon2Ctx& c, const std::vector<uint32_t>& in, uint64_t size, uint64_t batch, std::vector<uint32_t>* words, std::vector<uint32_t>* padded)
{
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(in.data());
  for (uint64_t b = 0; b < batch; b++) {
    words->push_back(Poseidon2<PR, T>::hash(Poseidon2Words{in.data() + b * size}, size, c));
    // the same message as a layer-0 chunk that lies wholly inside the leaves
    padded->push_back(Poseidon2<PR, T>::hash(Poseidon2Padded{ReadPadded{bytes, 4 * b * size, 4 * size * batch, nullptr, 4}}, size, c));
  }
}

template <class PR>
static bool hash_field(int t, const Poseidon2Ctx& c, const std::vector<uint32_t>& in, uint64_t size, uint64_t batch, std::vector<uint32_t>* w, std::vector<uint32_t>* p)
{
  switch (t) {
  case 2: hash_case<PR, 2>(c, in, size, batch, w, p); return true;
  case 3: hash_case<PR, 3>(c, in, size, batch, w, p); return true;
  case 4: hash_case<PR, 4>(c, in, size, batch, w, p); return true;
  case 8: hash_case<PR, 8>(c, in, size, batch, w, p); return true;
  case 12: hash_case<PR, 12>(c, in, size, batch, w, p); return true;
  case 16: hash_case<PR, 16>(c, in, size, batch, w, p); return true;
  case 20: hash_case<PR, 20>(c, in, size, batch, w, p); return true;
  case 24: hash_case<PR, 24>(c, in, size, batch, w, p); return true;
  }
  return false;
}

static int print_params()
{
  for (int f = 0; f < 2; f++)
    for (int t : WIDTHS) {
      const auto P = poseidon2::params(prime_of(f), (unsigned)t);
      if (!P) return 1;
      printf("params %s %d %d %d %d\nrc", FIELDS[f], t, P->alpha, P->r_f, P->r_p);
      for (uint32_t v : P->rc)
        printf(" %" PRIx32, v);
      printf("\ndiag");
      for (uint32_t v : P->diag)
        printf(" %" PRIx32, v);
      printf("\n");
    }
  // widths outside the eight have no parameters
  for (unsigned t : {0u, 1u, 5u, 6u, 28u})
    if (poseidon2::params(prime_of(0), t)) return 1;
  return 0;
}

static int hash_file(const char* path)
{
  std::ifstream file(path);
  if (!file) return 1;
  std::string line;
  while (std::getline(file, line)) {
    std::istringstream ls(line);
    std::string field, tag, tok;
    int t = 0;
    uint64_t size = 0, batch = 0;
    if (!(ls >> field >> t >> tag >> size >> batch)) continue;
    std::vector<uint32_t> in;
    while (ls >> tok)
      in.push_back((uint32_t)strtoul(tok.c_str(), nullptr, 16));
    const int f = field == FIELDS[0] ? 0 : 1;
    if (in.size() != size * batch) return 1;
    const auto P = poseidon2::params(prime_of(f), (unsigned)t);
    if (!P) return 1;
    const std::vector<uint32_t> consts =
      f == 0 ? poseidon2_device_constants<babybear_params>(P->rc, P->diag) : poseidon2_device_constants<koalabear_params>(P->rc, P->diag);
    Poseidon2Ctx c{consts.data(), P->r_f / 2, P->r_p, 0, 0};
    if (tag != "-") {
      const uint32_t v = (uint32_t)strtoul(tag.c_str(), nullptr, 16);
      c.has_tag = 1;
      c.tag = f == 0 ? SmallField<babybear_params>::to_mont(v) : SmallField<koalabear_params>::to_mont(v);
    }
    std::vector<uint32_t> words, padded;
    const bool ok = f == 0 ? hash_field<babybear_params>(t, c, in, size, batch, &words, &padded) : hash_field<koalabear_params>(t, c, in, size, batch, &words, &padded);
    if (!ok) return 1;
    for (const auto* v : {&words, &padded}) {
      for (size_t i = 0; i < v->size(); i++)
        printf("%s%" PRIx32, i ? " " : "", (*v)[i]);
      printf("\n");
    }
  }
  return 0;
}

int main(int argc, char** argv)
{
  if (argc == 2 && !strcmp(argv[1], "params")) return print_params();
  if (argc == 3 && !strcmp(argv[1], "hash")) return hash_file(argv[2]);
  fprintf(stderr, "usage: %s params | hash <file>\n", argv[0]);
  return 2;
}
