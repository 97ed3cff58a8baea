// Test infrastructure: a stand-alone program over the host-compilable parts of FRI over the wide fields -- F(digest) of
// icicle_amd/csrc/fri_plan.h and the fold arithmetic of icicle_amd/csrc/fri_fold_wide.hpp, the very functions the kernel and the host
// verifier of fri_wide.hip call -- compiled with g++ by tests/test_fri_wide_cpu.py (with the bound tracker of bigfield.hpp on, once
// plainly and once with -fsanitize=address,undefined) and compared with Python integers. It reads one command per line from standard
// input and answers each with one line; elements are the hex of their canonical little-endian bytes.
//   kind = goldilocks | goldilocks_extension | stark252 | bn254 | bls12_381 | bls12_377
//   digest kind hex          -> F(digest)
//   fold kind lo hi tw alpha -> (lo + hi)/2 + alpha * ((lo - hi)/2 * tw); lo, hi, alpha elements, tw a scalar of the base field
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../icicle_amd/csrc/fri_plan.h"
#include "../icicle_amd/csrc/fri_fold_wide.hpp"

using namespace icicle_hip;

static std::vector<uint8_t> unhex(const std::string& s)
{
  std::vector<uint8_t> v;
  for (size_t i = 0; i + 1 < s.size(); i += 2)
    v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return v;
}

static std::string hex(const uint32_t* w, int words)
{
  static const char* d = "0123456789abcdef";
  std::string s;
  for (int i = 0; i < words; i++)
    for (int b = 0; b < 4; b++) {
      const uint8_t v = (uint8_t)(w[i] >> (8 * b));
      s += d[v >> 4], s += d[v & 15];
    }
  return s;
}

static void words_of(const std::string& h, uint32_t* w, int words)
{
  const std::vector<uint8_t> b = unhex(h);
  std::memset(w, 0, 4 * words);
  for (size_t i = 0; i < b.size() && i < (size_t)(4 * words); i++)
    w[i / 4] |= (uint32_t)b[i] << (8 * (i % 4));
}

template <class PR, int COEFFS>
static std::string run(const std::string& cmd, std::istringstream& in)
{
  using F = FieldOps<PR>;
  using fe = typename F::fe;
  constexpr int W = F::N32;
  uint32_t out[8] = {0};
  if (cmd == "digest") {
    std::string digest;
    in >> digest;
    const std::vector<uint8_t> d = unhex(digest);
    if constexpr (COEFFS == 1)
      fri_wide_from_digest(d.data(), d.size(), PR::P32, W, out);
    else
      fri_gold_ext_from_digest(d.data(), d.size(), PR::P32, out);
    return hex(out, W * COEFFS);
  }
  std::string s[4];
  in >> s[0] >> s[1] >> s[2] >> s[3];
  uint32_t lo[8], hi[8], tw[8], alpha[8];
  words_of(s[0], lo, W * COEFFS), words_of(s[1], hi, W * COEFFS), words_of(s[2], tw, W), words_of(s[3], alpha, W * COEFFS);
  const fe t = F::from_canonical(tw);
  if constexpr (COEFFS == 1) {
    F::pack(out, FriWideFold<PR>::fold1(F::unpack(lo), F::unpack(hi), t, F::from_canonical(alpha)));
  } else {
    const uint32_t nonres[2] = {7, 0};
    const fe l2[2] = {F::unpack(lo), F::unpack(lo + W)}, h2[2] = {F::unpack(hi), F::unpack(hi + W)};
    const fe a1 = F::from_canonical(alpha + W);
    fe o[2];
    FriWideFold<PR>::fold2(l2, h2, t, F::from_canonical(alpha), a1, F::mul(a1, F::from_canonical(nonres)), o);
    F::pack(out, o[0]), F::pack(out + W, o[1]);
  }
  return hex(out, W * COEFFS);
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, kind, out;
    if (!(in >> cmd >> kind)) continue;
    if (cmd != "digest" && cmd != "fold")
      out = "unknown command";
    else if (kind == "goldilocks")
      out = run<goldilocks_params, 1>(cmd, in);
    else if (kind == "goldilocks_extension")
      out = run<goldilocks_params, 2>(cmd, in);
    else if (kind == "stark252")
      out = run<stark252_fr_params, 1>(cmd, in);
    else if (kind == "bn254")
      out = run<bn254_fr_params, 1>(cmd, in);
    else if (kind == "bls12_381")
      out = run<bls12_381_fr_params, 1>(cmd, in);
    else if (kind == "bls12_377")
      out = run<bls12_377_fr_params, 1>(cmd, in);
    else
      out = "unknown kind";
    std::printf("%s\n", out.c_str());
  }
  return 0;
}
