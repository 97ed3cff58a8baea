// Host-only part of the program / symbol API (sumcheck.hip): the symbol graph a caller builds through <field>_create_input_symbol,
// _add_symbols, ... and its compiler into the instruction list the device interpreter runs. No HIP in here, so
// tests/sumcheck_host_harness.cpp compiles it with g++ and compares it with the Python model (tests/sumcheck_model.py).
//
// Reference: include/icicle/program/symbol.h (the graph and its degree rule), program.h (allocation of the variables: parameters,
// then constants, then one intermediate per operation node; the node a parameter stands for is computed into that parameter's slot),
// returning_value_program.h (the last parameter is the return value, its degree the program's). The graph and the instruction
// encoding are this project's own: a proof depends on the function, not on how it is encoded.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <set>
#include <vector>

namespace icicle_hip {

  enum ProgOp : uint8_t { PROG_COPY = 0, PROG_ADD = 1, PROG_MUL = 2, PROG_SUB = 3, PROG_INV = 4, PROG_INPUT = 5, PROG_CONST = 6 };

  constexpr int PROG_MAX_DEGREE = 6; // include/icicle/sumcheck/sumcheck.h:12-14
  constexpr int PROG_MAX_INPUTS = 8;
  constexpr int PROG_MAX_VARS = 20;
  constexpr int PROG_AB_MINUS_C = 0, PROG_EQ_X_AB_MINUS_C = 1; // PreDefinedPrograms

  struct SymNode {
    ProgOp op = PROG_INPUT;
    std::shared_ptr<SymNode> a, b;
    int input_idx = -1;             // PROG_INPUT
    std::vector<uint32_t> constant; // PROG_CONST: one canonical element
    int degree = 0;                 // -1: undefined (an inverse somewhere below)
  };
  using SymRef = std::shared_ptr<SymNode>;

  inline SymRef sym_input(int idx)
  {
    auto n = std::make_shared<SymNode>();
    n->op = PROG_INPUT, n->input_idx = idx, n->degree = 1;
    return n;
  }
  inline SymRef sym_const(const uint32_t* words, int nof_words)
  {
    auto n = std::make_shared<SymNode>();
    n->op = PROG_CONST, n->constant.assign(words, words + nof_words), n->degree = 0;
    return n;
  }
  // input 1, constant 0, add / sub the larger, multiply the sum, inverse -1; -1 below gives -1
  inline SymRef sym_op(ProgOp op, const SymRef& a, const SymRef& b)
  {
    auto n = std::make_shared<SymNode>();
    n->op = op, n->a = a, n->b = b;
    if (a->degree < 0 || (b && b->degree < 0) || op == PROG_INV)
      n->degree = -1;
    else if (op == PROG_MUL)
      n->degree = a->degree + b->degree;
    else
      n->degree = a->degree > b->degree ? a->degree : b->degree;
    return n;
  }

  struct ProgInstr {
    uint8_t op, a, b, dst; // variables[dst] = variables[a] op variables[b]; PROG_COPY and PROG_INV read a only
  };

  struct CompiledProgram {
    int predefined = -1; // PROG_AB_MINUS_C, PROG_EQ_X_AB_MINUS_C, or -1: `ins`
    int nof_parameters = 0, nof_constants = 0, nof_intermediates = 0, degree = 0;
    std::vector<ProgInstr> ins;
    std::vector<std::vector<uint32_t>> constants; // constant k is variable nof_parameters + k
    int nof_inputs() const { return nof_parameters - 1; }
    int nof_vars() const { return nof_parameters + nof_constants + nof_intermediates; }
  };

  inline bool program_predefined(int id, CompiledProgram* out)
  {
    if (id != PROG_AB_MINUS_C && id != PROG_EQ_X_AB_MINUS_C) return false;
    *out = CompiledProgram{};
    out->predefined = id;
    out->nof_parameters = id == PROG_AB_MINUS_C ? 4 : 5;
    out->degree = id == PROG_AB_MINUS_C ? 2 : 3;
    return true;
  }

  class ProgramCompiler
  {
  public:
    // params: the inputs' symbols followed by the return value's. false: an input index outside the inputs, a constant of another
    // width, or more than 255 variables. general: a program with any number of outputs (program.h), in which every parameter is
    // an input as well; the instruction list is made the same way.
    bool run(const std::vector<SymRef>& params, int words, CompiledProgram* out, bool general = false)
    {
      m_out = out, m_words = words, m_ok = true, m_general = general;
      *out = CompiledProgram{};
      out->nof_parameters = (int)params.size();
      if (params.empty()) return false;
      for (const auto& p : params)
        if (!p) return false;
      for (const auto& p : params)
        constants(p);
      m_seen.clear();
      for (int i = 0; i < (int)params.size() && m_ok; i++) {
        SymNode* n = params[i].get();
        if (n->op == PROG_INPUT) m_var[n] = n->input_idx;
        auto it = m_var.find(n);
        if (it == m_var.end()) {
          m_var[n] = i;
          emit(params[i]);
        } else if (it->second != i) {
          push(PROG_COPY, it->second, 0, i);
        }
      }
      out->degree = params.back()->degree;
      return m_ok && out->nof_vars() <= 255;
    }

  private:
    void constants(const SymRef& n)
    {
      if (!n || !m_seen.insert(n.get()).second) return;
      constants(n->a);
      constants(n->b);
      if (n->op == PROG_CONST) {
        if ((int)n->constant.size() != m_words) m_ok = false;
        m_out->constants.push_back(n->constant);
        m_var[n.get()] = m_out->nof_parameters + m_out->nof_constants++;
      } else if (n->op == PROG_INPUT) {
        if (n->input_idx < 0 || n->input_idx >= (m_general ? m_out->nof_parameters : m_out->nof_inputs())) m_ok = false;
        m_var[n.get()] = n->input_idx;
      }
    }
    void emit(const SymRef& n)
    {
      if (!n || n->op == PROG_INPUT || n->op == PROG_CONST || !m_seen.insert(n.get()).second) return;
      emit(n->a);
      emit(n->b);
      if (m_var.find(n.get()) == m_var.end()) m_var[n.get()] = m_out->nof_parameters + m_out->nof_constants + m_out->nof_intermediates++;
      push(n->op, m_var[n->a.get()], n->b ? m_var[n->b.get()] : 0, m_var[n.get()]);
    }
    void push(ProgOp op, int a, int b, int dst)
    {
      if (a > 255 || b > 255 || dst > 255) {
        m_ok = false;
        return;
      }
      m_out->ins.push_back(ProgInstr{(uint8_t)op, (uint8_t)a, (uint8_t)b, (uint8_t)dst});
    }
    CompiledProgram* m_out = nullptr;
    int m_words = 1;
    bool m_ok = true, m_general = false;
    std::map<SymNode*, int> m_var;
    std::set<SymNode*> m_seen;
  };

  // 0 = a combine function the prover runs, 1 = invalid argument: the polynomial count is not the program's input count or is above
  // 8, the degree is below 1 (a constant, or an inverse: -1) or above 6, more than 20 variables
  inline int program_check_for_sumcheck(const CompiledProgram& p, uint64_t nof_polys)
  {
    if (nof_polys > (uint64_t)PROG_MAX_INPUTS || (int64_t)nof_polys != p.nof_inputs()) return 1;
    if (p.degree < 1 || p.degree > PROG_MAX_DEGREE) return 1;
    return p.nof_vars() > PROG_MAX_VARS ? 1 : 0;
  }

} // namespace icicle_hip
