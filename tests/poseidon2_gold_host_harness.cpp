// Host build of the Poseidon2 code over Goldilocks: icicle_amd/csrc/poseidon2_gold_params.h (the derivation) and poseidon2_gold.hpp
// (the hash a lane computes), compiled with g++ by tests/test_poseidon2_gold_cpu.py -- once plainly, once with
// -fsanitize=address,undefined.
//   poseidon2_gold_host_harness params         for every width: "params <t> <alpha> <R_F> <R_P> <draws>", "rc <hex> ..", "diag <hex> .."
//   poseidon2_gold_host_harness hash <file>    <file> holds one case per line: <t> <tag or -> <size> <batch> <hex element> ..;
//                                              per case one line of hex digests through the word reader and one through the padded-leaf reader
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../icicle_amd/csrc/poseidon2_gold.hpp"
#include "../icicle_amd/csrc/poseidon2_gold_params.h"

using namespace icicle_hip;

static const int WIDTHS[8] = {2, 3, 4, 8, 12, 16, 20, 24};

template <int T>
static void hash_case(const Poseidon2GoldCtx& c, const std::vector<uint64_t>& in, uint64_t size, uint64_t batch, std::vector<uint64_t>* words, std::vector<uint64_t>* padded)
{
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(in.data());
  for (uint64_t b = 0; b < batch; b++) {
    words->push_back(Poseidon2Gold<T>::hash(Poseidon2GoldWords{bytes + 8 * b * size}, size, c));
    // the same message as a layer-0 chunk that lies wholly inside the leaves
    padded->push_back(Poseidon2Gold<T>::hash(Poseidon2GoldPadded{ReadPadded{bytes, 8 * b * size, 8 * size * batch, nullptr, 8}}, size, c));
  }
}

static bool hash_width(int t, const Poseidon2GoldCtx& c, const std::vector<uint64_t>& in, uint64_t size, uint64_t batch, std::vector<uint64_t>* w, std::vector<uint64_t>* p)
{
  switch (t) {
  case 2: hash_case<2>(c, in, size, batch, w, p); return true;
  case 3: hash_case<3>(c, in, size, batch, w, p); return true;
  case 4: hash_case<4>(c, in, size, batch, w, p); return true;
  case 8: hash_case<8>(c, in, size, batch, w, p); return true;
  case 12: hash_case<12>(c, in, size, batch, w, p); return true;
  case 16: hash_case<16>(c, in, size, batch, w, p); return true;
  case 20: hash_case<20>(c, in, size, batch, w, p); return true;
  case 24: hash_case<24>(c, in, size, batch, w, p); return true;
  }
  return false;
}

static int print_params()
{
  for (int t : WIDTHS) {
    const auto P = poseidon2_gold::params((unsigned)t);
    if (!P) return 1;
    printf("params %d %d %d %d %d\nrc", t, P->alpha, P->r_f, P->r_p, P->draws);
    for (uint64_t v : P->rc)
      printf(" %" PRIx64, v);
    printf("\ndiag");
    for (uint64_t v : P->diag)
      printf(" %" PRIx64, v);
    printf("\n");
  }
  // widths outside the eight have no parameters
  for (unsigned t : {0u, 1u, 5u, 6u, 7u, 9u, 28u, 32u})
    if (poseidon2_gold::params(t)) return 1;
  return 0;
}

static int hash_file(const char* path)
{
  std::ifstream file(path);
  if (!file) return 1;
  std::string line;
  while (std::getline(file, line)) {
    std::istringstream ls(line);
    std::string tag, tok;
    int t = 0;
    uint64_t size = 0, batch = 0;
    if (!(ls >> t >> tag >> size >> batch)) continue;
    std::vector<uint64_t> in;
    while (ls >> tok)
      in.push_back((uint64_t)strtoull(tok.c_str(), nullptr, 16));
    if (in.size() != size * batch) return 1;
    const auto P = poseidon2_gold::params((unsigned)t);
    if (!P) return 1;
    const std::vector<uint64_t> consts = poseidon2_gold_device_constants(P->rc, P->diag);
    Poseidon2GoldCtx c{consts.data(), P->r_f / 2, P->r_p, 0, 0};
    if (tag != "-") c.has_tag = 1, c.tag = (uint64_t)strtoull(tag.c_str(), nullptr, 16);
    std::vector<uint64_t> words, padded;
    if (!hash_width(t, c, in, size, batch, &words, &padded)) return 1;
    for (const auto* v : {&words, &padded}) {
      for (size_t i = 0; i < v->size(); i++)
        printf("%s%" PRIx64, i ? " " : "", (*v)[i]);
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
