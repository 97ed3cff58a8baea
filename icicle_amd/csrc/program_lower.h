// Host-only lowering of a compiled program (program_plan.h) into the list the execute_program kernel runs (execute_program.hip). No
// HIP in here, so tests/execute_program_host_harness.cpp compiles it with g++ and compares it with the Python model
// (tests/execute_program_model.py).
//
// Reference: backend/cpu/include/cpu_program_executor.h and backend/cpu/src/field/cpu_vec_ops.cpp:635-678. Per element, the variables
// are the parameters' values, then the constants, then the intermediates; the instructions run in order; every parameter that an
// instruction wrote is stored back. A parameter that is read after it was overwritten therefore sees the new value.
//
// The lowered list names slots of a fixed variable file instead of variables. Constant k lives in slot k for the whole launch. Every
// other value gets the lowest free slot when it is made and gives it back after its last use, so the cap is on the number of values
// alive at once (constants included), not on the length of the program. A parameter is loaded right before the first instruction
// that reads its value from memory and not at all when none does; the written parameters are stored after the last instruction, so
// every load of an element precedes every store of it and a pointer may be passed for two parameters.
#pragma once
#include <algorithm>
#include <bitset>
#include "sumcheck_plan.h"

namespace icicle_hip {

  // beside ProgOp's PROG_COPY .. PROG_INV. EP_LOAD: slot dst = parameter a's element, into Montgomery form. EP_STORE: parameter b's
  // element = slot a, out of Montgomery form.
  enum EpOp : uint8_t { EP_LOAD = 8, EP_STORE = 9 };
  constexpr uint8_t EP_READ = 1, EP_WRITTEN = 2;

  // Slots of the variable file per lane. One wave per block, a wave's lanes on consecutive words. A slot of a one-word field holds
  // four elements per lane (the interpreter works on four at once): 1 KiB of LDS, 64 KiB for 64 slots. A slot of an eight-word field
  // holds one element of 9 limbs: 2304 bytes, 54 KiB for 24 slots. A block may have 64 KiB.
  constexpr int EP_CAP_SMALL = 64, EP_CAP_BIG = 24;
  inline int program_live_cap(int words) { return words == 1 ? EP_CAP_SMALL : EP_CAP_BIG; }

  struct LoweredProgram {
    int predefined = -1; // PROG_AB_MINUS_C, PROG_EQ_X_AB_MINUS_C, or -1: `code`
    int nof_parameters = 0, nof_constants = 0, nof_slots = 0;
    std::vector<uint32_t> code;                   // op | a << 8 | b << 16 | dst << 24
    std::vector<uint8_t> param_use;               // EP_READ | EP_WRITTEN per parameter
    std::vector<std::vector<uint32_t>> constants; // c 2^mont_bits mod p, canonical words
  };

  // 0: lowered. 1: not a program the compiler makes (a variable out of range, a constant written, an intermediate read before it is
  // written, an opcode that is none). 2: more than `cap` values alive at once.
  inline int program_lower(const HostField& f, int mont_bits, const CompiledProgram& p, int cap, LoweredProgram* out)
  {
    *out = LoweredProgram{};
    out->predefined = p.predefined, out->nof_parameters = p.nof_parameters, out->nof_constants = p.nof_constants;
    if (p.nof_parameters < 1 || p.nof_parameters > 255) return 1;
    out->param_use.assign(p.nof_parameters, 0);
    if (p.predefined >= 0) {
      for (int j = 0; j + 1 < p.nof_parameters; j++)
        out->param_use[j] = EP_READ;
      out->param_use[p.nof_parameters - 1] = EP_WRITTEN;
      return 0;
    }
    const int nv = p.nof_vars(), np = p.nof_parameters, nc = p.nof_constants;
    if (nv > 256 || (int)p.constants.size() != nc) return 1;
    for (const auto& c : p.constants) {
      if ((int)c.size() != f.words) return 1;
      std::vector<uint32_t> wide((size_t)f.words + (mont_bits + 31) / 32 + 1, 0), m(f.words);
      for (int i = 0; i < f.words; i++) { // c << mont_bits
        const int at = mont_bits / 32, sh = mont_bits % 32;
        wide[i + at] |= c[i] << sh;
        if (sh) wide[i + at + 1] |= c[i] >> (32 - sh);
      }
      f.reduce(wide.data(), (int)wide.size(), m.data());
      out->constants.push_back(m);
    }
    const auto is_const = [&](int v) { return v >= np && v < np + nc; };

    // the list over variables, with the loads and stores in it
    struct Op {
      uint8_t op;
      int a, b, dst; // variables; -1: none. EP_LOAD: a = dst = the parameter. EP_STORE: a = b = the parameter.
    };
    std::vector<Op> ops;
    std::vector<bool> defined(nv, false);
    for (int v = np; v < np + nc; v++)
      defined[v] = true;
    for (const ProgInstr& i : p.ins) {
      if (i.op > PROG_INV) return 1;
      const bool unary = i.op == PROG_COPY || i.op == PROG_INV;
      const int srcs[2] = {i.a, unary ? -1 : (int)i.b};
      if (i.dst >= nv || is_const(i.dst)) return 1;
      for (int v : srcs) {
        if (v < 0) continue;
        if (v >= nv) return 1;
        if (defined[v]) continue;
        if (v >= np) return 1; // an intermediate nobody wrote
        ops.push_back(Op{EP_LOAD, v, -1, v});
        out->param_use[v] |= EP_READ, defined[v] = true;
      }
      ops.push_back(Op{i.op, srcs[0], srcs[1], (int)i.dst});
      defined[i.dst] = true;
      if (i.dst < np) out->param_use[i.dst] |= EP_WRITTEN;
    }
    for (int j = 0; j < np; j++)
      if (out->param_use[j] & EP_WRITTEN) ops.push_back(Op{EP_STORE, j, j, -1});

    // alive after each op, backwards; the constants are alive throughout and never listed
    std::vector<std::bitset<256>> after(ops.size());
    std::bitset<256> live;
    for (size_t k = ops.size(); k-- > 0;) {
      after[k] = live;
      const Op& o = ops[k];
      if (o.dst >= 0) live.reset(o.dst);
      if (o.op != EP_LOAD) {
        if (o.a >= 0 && !is_const(o.a)) live.set(o.a);
        if (o.b >= 0 && o.op != EP_STORE && !is_const(o.b)) live.set(o.b);
      }
    }
    std::vector<int> slot(nv, -1);
    std::vector<bool> used(256, false);
    int peak = nc;
    for (int k = 0; k < nc; k++)
      slot[np + k] = k, used[k] = true;
    if (nc > cap) return 2;
    for (size_t k = 0; k < ops.size(); k++) {
      const Op& o = ops[k];
      uint32_t a = 0, b = 0, d = 0;
      if (o.op == EP_LOAD) {
        a = (uint32_t)o.a;
      } else {
        a = (uint32_t)slot[o.a];
        if (o.op == EP_STORE)
          b = (uint32_t)o.b;
        else if (o.b >= 0)
          b = (uint32_t)slot[o.b];
        // operands that nobody reads again give their slots back before the result takes one: the kernel reads both operands
        // into registers before it writes
        const int srcs[2] = {o.a, o.op == EP_STORE ? -1 : o.b};
        for (int v : srcs)
          if (v >= 0 && !is_const(v) && v != o.dst && !after[k][v] && slot[v] >= 0) used[slot[v]] = false, slot[v] = -1;
      }
      if (o.dst >= 0) {
        if (slot[o.dst] < 0) {
          int s = 0;
          while (s < 256 && used[s])
            s++;
          if (s >= cap) return 2;
          slot[o.dst] = s, used[s] = true;
          peak = std::max(peak, s + 1);
        }
        d = (uint32_t)slot[o.dst];
        if (!after[k][o.dst]) used[slot[o.dst]] = false, slot[o.dst] = -1; // a value nobody reads
      }
      out->code.push_back((uint32_t)o.op | a << 8 | b << 16 | d << 24);
    }
    out->nof_slots = peak;
    return 0;
  }

} // namespace icicle_hip
