// Drives the host-only sumcheck code (icicle_amd/csrc/sumcheck_plan.h, program_plan.h) from commands on stdin, one answer line per
// command, for tests/test_sumcheck_cpu.py to compare with the Python model. Built with g++, plainly and with the sanitizers.
// An element is the hex of its canonical little-endian bytes; "-" is the empty byte string.
//   transcript <ds> <poly> <challenge> <rounds> <degree> <field> <claimed> <seed> <round> <alpha> <round poly bytes>
//        -> entry0, the round's hash input
//   digest <field> <digest>                       -> F(digest)
//   arith <field> <a> <b>                         -> a + b, a - b, a b, 1 / a
//   lagrange <field> <x> <eval> ...               -> the interpolated value at x
//   program <field> <nof_polys> <nof_inputs> <node,node,..> <input> ...
//        node = in:i | const:<element> | add:a:b | sub:a:b | mul:a:b | inv:a, a and b indices of earlier nodes; the last is returned
//        -> "refused" (the compiler), else degree, variables, instructions, acceptable for nof_polys (0 / 1), value ("-": an inverse)
//   predefined <field> <id> <nof_polys> <input> ... -> the same columns
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../icicle_amd/csrc/field_consts.h"
#include "../icicle_amd/csrc/sumcheck_plan.h"

using namespace icicle_hip;

static std::vector<uint8_t> unhex(const std::string& s)
{
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2)
    v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return v;
}
static std::string hex(const uint8_t* p, size_t n)
{
  if (!n) return "-";
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; i++)
    s += d[p[i] >> 4], s += d[p[i] & 15];
  return s;
}
static std::string hex(const std::vector<uint8_t>& v) { return hex(v.data(), v.size()); }

static HostField field_of(const std::string& name)
{
  if (name == "babybear") {
    const uint32_t p = babybear_params::P;
    return HostField(&p, 1);
  }
  if (name == "koalabear") {
    const uint32_t p = koalabear_params::P;
    return HostField(&p, 1);
  }
  if (name == "bn254") return HostField(bn254_fr_params::P32, 8);
  return HostField(bls12_381_fr_params::P32, 8);
}
static std::vector<uint32_t> element(const HostField& f, const std::string& s)
{
  std::vector<uint8_t> b = unhex(s);
  b.resize(4 * f.words, 0);
  std::vector<uint32_t> w(f.words);
  std::memcpy(w.data(), b.data(), b.size());
  return w;
}
static std::string show(const HostField& f, const uint32_t* w) { return hex(reinterpret_cast<const uint8_t*>(w), 4 * f.words); }

static void report(const HostField& f, const CompiledProgram& prog, uint64_t nof_polys, std::istringstream& in)
{
  std::vector<uint32_t> inputs;
  std::string tok;
  while (in >> tok) {
    const auto e = element(f, tok);
    inputs.insert(inputs.end(), e.begin(), e.end());
  }
  inputs.resize((size_t)(prog.nof_inputs() > 0 ? prog.nof_inputs() : 0) * f.words, 0);
  uint32_t out[8];
  const bool ok = program_eval(f, prog, inputs.data(), out);
  std::cout << prog.degree << " " << prog.nof_vars() << " " << prog.ins.size() << " " << (program_check_for_sumcheck(prog, nof_polys) == 0 ? 1 : 0) << " "
            << (ok ? show(f, out) : "-") << "\n";
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, a, b, c;
    in >> cmd;
    if (cmd == "transcript") {
      std::string field, claimed, seed, alpha, poly;
      uint32_t rounds, degree, round;
      in >> a >> b >> c >> rounds >> degree >> field >> claimed >> seed >> round >> alpha >> poly;
      const HostField f = field_of(field);
      const std::vector<uint8_t> ds = unhex(a), pl = unhex(b), ch = unhex(c), rp = unhex(poly);
      const auto cs = element(f, claimed), sd = element(f, seed), al = element(f, alpha);
      const SumcheckLabels labels{ds.data(), pl.data(), ch.data(), ds.size(), pl.size(), ch.size()};
      const SumcheckTranscriptBytes t(labels, rounds, degree, reinterpret_cast<const uint8_t*>(cs.data()), reinterpret_cast<const uint8_t*>(sd.data()), 4 * (size_t)f.words);
      std::cout << hex(t.entry0()) << " " << hex(t.round_input(round, reinterpret_cast<const uint8_t*>(al.data()), rp.data())) << "\n";
    } else if (cmd == "digest") {
      in >> a >> b;
      const HostField f = field_of(a);
      const std::vector<uint8_t> d = unhex(b);
      uint32_t out[8];
      f.from_digest(d.data(), d.size(), out);
      std::cout << show(f, out) << "\n";
    } else if (cmd == "arith") {
      in >> a >> b >> c;
      const HostField f = field_of(a);
      const auto x = element(f, b), y = element(f, c);
      uint32_t r[4][8];
      f.add(x.data(), y.data(), r[0]), f.sub(x.data(), y.data(), r[1]), f.mul(x.data(), y.data(), r[2]), f.inv(x.data(), r[3]);
      std::cout << show(f, r[0]) << " " << show(f, r[1]) << " " << show(f, r[2]) << " " << show(f, r[3]) << "\n";
    } else if (cmd == "lagrange") {
      in >> a >> b;
      const HostField f = field_of(a);
      const auto x = element(f, b);
      std::vector<uint32_t> evals;
      int count = 0;
      while (in >> c) {
        const auto e = element(f, c);
        evals.insert(evals.end(), e.begin(), e.end());
        count++;
      }
      uint32_t out[8];
      sumcheck_lagrange_eval(f, evals.data(), count, x.data(), out);
      std::cout << show(f, out) << "\n";
    } else if (cmd == "program") {
      uint64_t nof_polys;
      int nof_inputs;
      in >> a >> nof_polys >> nof_inputs >> b;
      const HostField f = field_of(a);
      std::vector<SymRef> nodes;
      std::istringstream spec(b);
      std::string node;
      while (std::getline(spec, node, ',')) {
        std::istringstream ns(node);
        std::string kind, p1, p2;
        std::getline(ns, kind, ':'), std::getline(ns, p1, ':'), std::getline(ns, p2, ':');
        if (kind == "in")
          nodes.push_back(sym_input(std::stoi(p1)));
        else if (kind == "const")
          nodes.push_back(sym_const(element(f, p1).data(), f.words));
        else if (kind == "inv")
          nodes.push_back(sym_op(PROG_INV, nodes[std::stoi(p1)], nullptr));
        else
          nodes.push_back(sym_op(kind == "add" ? PROG_ADD : kind == "sub" ? PROG_SUB : PROG_MUL, nodes[std::stoi(p1)], nodes[std::stoi(p2)]));
      }
      std::vector<SymRef> params;
      for (int i = 0; i < nof_inputs; i++)
        params.push_back(sym_input(i));
      params.push_back(nodes.back());
      CompiledProgram prog;
      if (!ProgramCompiler().run(params, f.words, &prog))
        std::cout << "refused\n";
      else
        report(f, prog, nof_polys, in);
    } else if (cmd == "predefined") {
      int id;
      uint64_t nof_polys;
      in >> a >> id >> nof_polys;
      CompiledProgram prog;
      if (!program_predefined(id, &prog))
        std::cout << "refused\n";
      else
        report(field_of(a), prog, nof_polys, in);
    } else if (!cmd.empty()) {
      std::cout << "?\n";
    }
  }
  return 0;
}
