// Drives the host-only part of execute_program (icicle_amd/csrc/program_plan.h in its general mode, program_lower.h) from commands on
// stdin, one answer line per command, for tests/test_execute_program_cpu.py to compare with the Python model
// (tests/execute_program_model.py). Built with g++, plainly and with the sanitizers.
// An element is the hex of its canonical little-endian bytes.
//   lower <field> <cap> <nof_parameters> <node,node,..> <param,param,..> <value> ...
//        node = in:i | const:<element> | add:a:b | sub:a:b | mul:a:b | inv:a, a and b indices of earlier nodes; param = the node
//        whose value the parameter has afterwards; value = the parameters' elements in memory, in order
//        -> "refused" (the compiler), "invalid" or "overcap" (the lowering), else
//           <variables> <op:a:b:dst,..> <slots> <use,use,..> <op:a:b:dst,..> <constant,..> <value,..>
//           the compiled list, then the lowered one with its constants (Montgomery form) and the values in memory after it ran
//   predefined <field> <id> -> "refused", else <nof_parameters> <use,use,..>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../icicle_amd/csrc/field_consts.h"
#include "../icicle_amd/csrc/program_lower.h"

using namespace icicle_hip;

static HostField field_of(const std::string& name, int* mont_bits)
{
  *mont_bits = (name == "babybear" || name == "koalabear") ? 32 : 261; // ScSmall / ScBig::MONT_BITS (execute_program.hip asserts them)
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
  std::vector<uint8_t> b;
  for (size_t i = 0; i + 1 < s.size(); i += 2)
    b.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  b.resize(4 * f.words, 0);
  std::vector<uint32_t> w(f.words);
  std::memcpy(w.data(), b.data(), b.size());
  return w;
}
static std::string show(const HostField& f, const uint32_t* w)
{
  static const char* d = "0123456789abcdef";
  const uint8_t* p = reinterpret_cast<const uint8_t*>(w);
  std::string s;
  for (int i = 0; i < 4 * f.words; i++)
    s += d[p[i] >> 4], s += d[p[i] & 15];
  return s;
}
static std::string show_list(const uint32_t* code, size_t n)
{
  std::string s;
  for (size_t k = 0; k < n; k++) {
    const uint32_t i = code[k];
    s += (k ? "," : "") + std::to_string(i & 0xff) + ":" + std::to_string((i >> 8) & 0xff) + ":" + std::to_string((i >> 16) & 0xff) + ":" + std::to_string(i >> 24);
  }
  return n ? s : "-";
}

// the lowered list over canonical elements: `mem` holds the parameters' elements, `file` the slots
static bool run_lowered(const HostField& f, const LoweredProgram& l, const CompiledProgram& p, std::vector<uint32_t>& mem)
{
  const int w = f.words;
  std::vector<uint32_t> file((size_t)(l.nof_slots > 0 ? l.nof_slots : 1) * w, 0);
  for (int k = 0; k < l.nof_constants; k++)
    std::memcpy(&file[(size_t)k * w], p.constants[k].data(), 4 * w);
  for (uint32_t i : l.code) {
    const uint32_t op = i & 0xff, a = (i >> 8) & 0xff, b = (i >> 16) & 0xff, d = i >> 24;
    if (op == EP_LOAD) {
      if ((int)a >= l.nof_parameters || (int)d >= l.nof_slots) return false;
      std::memcpy(&file[(size_t)d * w], &mem[(size_t)a * w], 4 * w);
      continue;
    }
    if (op == EP_STORE) {
      if ((int)b >= l.nof_parameters || (int)a >= l.nof_slots) return false;
      std::memcpy(&mem[(size_t)b * w], &file[(size_t)a * w], 4 * w);
      continue;
    }
    if ((int)a >= l.nof_slots || (int)b >= l.nof_slots || (int)d >= l.nof_slots) return false;
    uint32_t x[8], y[8], r[8];
    std::memcpy(x, &file[(size_t)a * w], 4 * w), std::memcpy(y, &file[(size_t)b * w], 4 * w);
    switch (op) {
    case PROG_COPY: std::memcpy(r, x, 4 * w); break;
    case PROG_ADD: f.add(x, y, r); break;
    case PROG_SUB: f.sub(x, y, r); break;
    case PROG_MUL: f.mul(x, y, r); break;
    case PROG_INV: f.inv(x, r); break;
    default: return false;
    }
    std::memcpy(&file[(size_t)d * w], r, 4 * w);
  }
  return true;
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, name;
    in >> cmd >> name;
    int mont_bits = 0;
    if (cmd == "lower") {
      const HostField f = field_of(name, &mont_bits);
      int cap, nof_parameters;
      std::string nodes_s, params_s, tok;
      in >> cap >> nof_parameters >> nodes_s >> params_s;
      std::vector<SymRef> nodes, params;
      std::istringstream spec(nodes_s), pspec(params_s);
      while (std::getline(spec, tok, ',')) {
        std::istringstream ns(tok);
        std::string kind, p1, p2;
        std::getline(ns, kind, ':'), std::getline(ns, p1, ':'), std::getline(ns, p2, ':');
        if (kind == "in")
          nodes.push_back(sym_input(std::stoi(p1)));
        else if (kind == "const")
          nodes.push_back(sym_const(element(f, p1).data(), f.words));
        else if (kind == "inv")
          nodes.push_back(sym_op(PROG_INV, nodes.at(std::stoi(p1)), nullptr));
        else
          nodes.push_back(sym_op(kind == "add" ? PROG_ADD : kind == "sub" ? PROG_SUB : PROG_MUL, nodes.at(std::stoi(p1)), nodes.at(std::stoi(p2))));
      }
      while (std::getline(pspec, tok, ','))
        params.push_back(nodes.at(std::stoi(tok)));
      std::vector<uint32_t> mem;
      while (in >> tok) {
        const auto e = element(f, tok);
        mem.insert(mem.end(), e.begin(), e.end());
      }
      mem.resize((size_t)nof_parameters * f.words, 0);
      CompiledProgram prog;
      LoweredProgram low;
      if ((int)params.size() != nof_parameters || !ProgramCompiler().run(params, f.words, &prog, true)) {
        std::cout << "refused\n";
        continue;
      }
      const int rc = program_lower(f, mont_bits, prog, cap, &low);
      if (rc) {
        std::cout << (rc == 2 ? "overcap\n" : "invalid\n");
        continue;
      }
      if (low.nof_slots > cap || !run_lowered(f, low, prog, mem)) {
        std::cout << "broken\n";
        continue;
      }
      std::vector<uint32_t> compiled;
      for (const ProgInstr& i : prog.ins)
        compiled.push_back((uint32_t)i.op | (uint32_t)i.a << 8 | (uint32_t)i.b << 16 | (uint32_t)i.dst << 24);
      std::cout << prog.nof_vars() << " " << show_list(compiled.data(), compiled.size()) << " " << low.nof_slots << " ";
      for (int j = 0; j < nof_parameters; j++)
        std::cout << (j ? "," : "") << (int)low.param_use[j];
      std::cout << " " << show_list(low.code.data(), low.code.size()) << " ";
      for (size_t k = 0; k < low.constants.size(); k++)
        std::cout << (k ? "," : "") << show(f, low.constants[k].data());
      if (low.constants.empty()) std::cout << "-";
      std::cout << " ";
      for (int j = 0; j < nof_parameters; j++)
        std::cout << (j ? "," : "") << show(f, &mem[(size_t)j * f.words]);
      std::cout << "\n";
    } else if (cmd == "predefined") {
      const HostField f = field_of(name, &mont_bits);
      int id;
      in >> id;
      CompiledProgram prog;
      LoweredProgram low;
      if (!program_predefined(id, &prog) || program_lower(f, mont_bits, prog, 1, &low)) {
        std::cout << "refused\n";
        continue;
      }
      std::cout << low.nof_parameters << " ";
      for (int j = 0; j < low.nof_parameters; j++)
        std::cout << (j ? "," : "") << (int)low.param_use[j];
      std::cout << "\n";
    } else if (!cmd.empty()) {
      std::cout << "?\n";
    }
  }
  return 0;
}
