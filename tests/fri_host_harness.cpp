// Test infrastructure: a stand-alone program over icicle_amd/csrc/fri_plan.h (no HIP), compiled with g++ by tests/test_fri_cpu.py --
// once plainly and once with -fsanitize=address,undefined -- and compared with the Python model (tests/fri_model.py). It reads one
// command per line from standard input and answers each with one line; byte strings are hex, "-" is the empty string.
//   plan n folding_factor stopping_degree nof_queries compress_chunk compress_out -> rc log_n rounds final_size total_elements (size:layers)*
//   mt seed count                -> count outputs of MT19937
//   mt_nth seed k                -> the k-th output (k = 1: the first)
//   draw digest count final_size n -> the queries
//   field p words digest         -> the words of F(digest)
//   leaf q round_size symmetric  -> the leaf index
//   transcript ds round commit nonce_label public log_n prev root alpha nonce -> entry0 round_input pow_challenge query_input(pow) query_input(no pow)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../icicle_amd/csrc/fri_plan.h"

using namespace icicle_hip;

static std::vector<uint8_t> unhex(const std::string& s)
{
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2)
    v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return v;
}

static std::string hex(const std::vector<uint8_t>& v)
{
  if (v.empty()) return "-";
  static const char* d = "0123456789abcdef";
  std::string s;
  for (uint8_t b : v)
    s += d[b >> 4], s += d[b & 15];
  return s;
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    std::ostringstream out;
    if (cmd == "plan") {
      uint64_t n, ff, sd, nq, chunk, o;
      in >> n >> ff >> sd >> nq >> chunk >> o;
      FriPlan p;
      const int rc = fri_make_plan(n, ff, sd, nq, chunk, o, &p);
      out << rc;
      if (rc == 0) {
        uint64_t total = 0; // elements of all layers, the final polynomial included
        for (uint32_t r = 0; r <= p.rounds; r++)
          total += p.round_size(r);
        out << " " << p.log_n << " " << p.rounds << " " << p.final_size << " " << total;
        for (uint32_t r = 0; r < p.rounds; r++)
          out << " " << p.round_size(r) << ":" << p.tree_layers(r);
      }
    } else if (cmd == "mt" || cmd == "mt_nth") {
      uint32_t seed;
      uint64_t k;
      in >> seed >> k;
      FriMt19937 mt(seed);
      uint32_t last = 0;
      for (uint64_t i = 0; i < k; i++) {
        last = mt.next();
        if (cmd == "mt") out << (i ? " " : "") << last;
      }
      if (cmd == "mt_nth") out << last;
    } else if (cmd == "draw") {
      std::string digest;
      uint64_t count, fs, n;
      in >> digest >> count >> fs >> n;
      const std::vector<uint8_t> d = unhex(digest);
      const std::vector<uint64_t> q = fri_draw_queries(d.data(), count, fs, n);
      for (size_t i = 0; i < q.size(); i++)
        out << (i ? " " : "") << q[i];
    } else if (cmd == "field") {
      uint32_t p;
      int words;
      std::string digest;
      in >> p >> words >> digest;
      const std::vector<uint8_t> d = unhex(digest);
      uint32_t w[4] = {0, 0, 0, 0};
      fri_field_from_digest(d.data(), d.size(), p, words, w);
      for (int i = 0; i < words; i++)
        out << (i ? " " : "") << w[i];
    } else if (cmd == "leaf") {
      uint64_t q, size;
      int sym;
      in >> q >> size >> sym;
      out << fri_leaf_index(q, size, sym != 0);
    } else if (cmd == "transcript") {
      std::string f[5], prev, root, alpha;
      uint32_t log_n;
      uint64_t nonce;
      in >> f[0] >> f[1] >> f[2] >> f[3] >> f[4] >> log_n >> prev >> root >> alpha >> nonce;
      std::vector<uint8_t> b[5];
      for (int i = 0; i < 5; i++)
        b[i] = unhex(f[i]);
      // empty strings come as null pointers, as a caller may pass them
      const FriLabels l{b[0].empty() ? nullptr : b[0].data(), b[1].empty() ? nullptr : b[1].data(), b[2].empty() ? nullptr : b[2].data(),
                        b[3].empty() ? nullptr : b[3].data(), b[4].empty() ? nullptr : b[4].data(), b[0].size(), b[1].size(), b[2].size(), b[3].size(), b[4].size()};
      const FriTranscriptBytes t(l, log_n);
      const std::vector<uint8_t> pv = unhex(prev), rt = unhex(root), al = unhex(alpha);
      out << hex(t.entry0()) << " " << hex(t.round_input(pv.data(), pv.size(), rt.data(), rt.size())) << " " << hex(t.pow_challenge(al.data(), al.size())) << " "
          << hex(t.query_input(true, al.data(), al.size(), nonce)) << " " << hex(t.query_input(false, al.data(), al.size(), nonce));
    } else {
      out << "unknown command";
    }
    std::printf("%s\n", out.str().c_str());
  }
  return 0;
}
